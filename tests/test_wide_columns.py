"""tests/wide_columns.py without a GPU: the 11-transform shortcut equals the oracle applied column by column, and first_bad_column
names the first column that each kind of split error touches, so the GPU comparison built on the two cannot hide one."""
import numpy as np
import pytest

import wide_columns as wc

W = 70_001
SPLIT = wc.LAUNCH_MAX

TRANSFORMS = {
    "fft": lambda o: o.fft,
    "ifft": lambda o: o.ifft,
    "coset_ifft": lambda o: (lambda c: o.coset_ifft(c, 7)),
    "lde": lambda o: (lambda c: o.lde(c, 2, 7)),
}


def test_the_stride_is_coprime_to_every_split():
    for per in (65535, 65536, 65535 >> 1, 65535 >> 2, 65535 >> 3, 65535 >> 4):
        assert np.gcd(wc.DISTINCT, per) == 1, per


@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_expected_is_the_oracle_column_by_column(oracle, name):
    T = TRANSFORMS[name](oracle)
    rng = np.random.default_rng(40)
    data, base, scale = wc.columns(oracle, rng, 40, 8)
    assert data.shape == (40, 8) and base.shape == (11, 8) and scale.shape == (40,)
    assert len(set(int(s) for s in scale)) == 40 and (scale != 0).all()
    for j in range(40):
        assert [int(v) for v in data[j]] == [int(scale[j]) * int(b) % wc.P for b in base[j % 11]], j
    want = np.stack([T(c) for c in data])
    got = wc.expected(oracle, T, base, scale, 40)
    assert got.shape == want.shape and (got == want).all()
    assert wc.first_bad_column(got, want) is None
    assert len(set(c.tobytes() for c in got)) == 40, "two columns are equal"


@pytest.fixture(scope="module")
def wide(oracle):
    """a correct expected array of W columns (the identity transform), left unchanged by the tests that share it"""
    data, base, scale = wc.columns(oracle, np.random.default_rng(41), W, 2)
    want = wc.expected(oracle, lambda c: c, base, scale, W)
    assert (want == data).all()
    want.setflags(write=False)
    return want


def test_an_equal_array_has_no_bad_column(wide):
    assert wc.first_bad_column(wide.copy(), wide) is None
    wc.check(wide.copy(), wide)


def test_second_launch_shifted_by_one_column(wide):
    got = wide.copy()
    got[SPLIT:-1] = wide[SPLIT + 1:]
    assert wc.first_bad_column(got, wide) == SPLIT


def test_second_launch_reads_the_first_launchs_columns(wide):
    got = wide.copy()
    got[SPLIT:] = wide[:W - SPLIT]
    assert wc.first_bad_column(got, wide) == SPLIT


def test_last_column_zeroed(wide):
    got = wide.copy()
    got[W - 1] = 0
    assert wc.first_bad_column(got, wide) == W - 1


def test_columns_on_either_side_of_the_split_swapped(wide):
    got = wide.copy()
    got[[SPLIT, SPLIT + 1]] = wide[[SPLIT + 1, SPLIT]]
    assert wc.first_bad_column(got, wide) == SPLIT


def test_the_message_names_the_column_and_its_side_of_the_split(wide):
    got = wide.copy()
    got[SPLIT + 2, 1] ^= np.uint64(1)
    with pytest.raises(AssertionError) as e:
        wc.check(got, wide, what="fft")
    assert "column %d = column 2 of launch 1" % (SPLIT + 2) in str(e.value) and "split at column %d" % SPLIT in str(e.value)
    assert "the first launch" in wc.where(SPLIT - 1) and "launch 2" in wc.where(2 * 4095 + 1, 4095)
    assert wc.first_bad_column(wide[:-1], wide) == 0          # a short result is wrong from the start
