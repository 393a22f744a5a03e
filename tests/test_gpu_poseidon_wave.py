"""The one-state-per-lane Poseidon kernels run their seven full-round linear layers on the matrix pipe (pos::permute_wave,
poseidon.h): an int8 matrix instruction acts on the whole wave, lanes l and l + 32 share one column of it, and the state bytes
enter as signed values.  Against the CPU oracle, bit for bit: batch sizes around the wave and workgroup edges (the lanes past the
end run the permutation too and only their store is masked), special words in the state that ENTERS the permutation, batches in
which lane l + 32 alone differs from lane l, and the leaf-hash and tree-level kernels that call the same function.

What this file does not reach is the byte range of the matrix layer itself: an entering word gets round 0's constant added and passes
an S-box before the first linear layer sees it, so all seven layers receive what are in effect uniformly random bytes.  States of
0x00 / 0x7f / 0x80 / 0xff bytes and non-canonical words are fed to pos::mds_add_wave directly, in every lane, by the group
`poseidon_layers` of tests/test_gpu_field_probe.py (operand sets and their reach: tests/field_model.py, tests/test_field_probe.py)."""
import os

import numpy as np
import pytest

import plonky2_lib_amd as glp

pytestmark = pytest.mark.gpu
P = glp.P
COUNTS = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000]
# 0, p - 1, and words whose bytes are all 0x00 / 0x7f / 0x80 / 0xff (reduced where they are not field elements).  They exercise the state
# path (loads, round 0's additions, lanes, stores); they do not survive round 0's S-boxes, so they are not the matrix layer's byte extremes
SPECIAL = [0, P - 1, 0x7F7F7F7F7F7F7F7F, 0x8080808080808080, 0xFFFFFFFFFFFFFFFF % P, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF,
           0x7F7F7F7F80808080, 0x80808080FFFFFFFF, 0xFFFFFFFF7F7F7F7F % P, 0x000000007F7F7F7F, 0x8080808000000000]


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def states(oracle):
    """1000 states and their permutations, computed once: [0, 12 * len(SPECIAL)) hold one special value in one element of a random state,
    then len(SPECIAL) uniform special states, then states mixing special and random words, then random ones."""
    rng = np.random.default_rng(950)
    st = oracle.rand_field(rng, (1000, 12))
    k = 0
    for v in SPECIAL:
        for e in range(12):
            st[k, e] = v
            k += 1
    for v in SPECIAL:
        st[k, :] = v
        k += 1
    sp = np.array(SPECIAL, dtype=np.uint64)
    mask = rng.random((300, 12)) < 0.5
    blk = st[k:k + 300]
    blk[mask] = sp[rng.integers(0, len(sp), size=int(mask.sum()))]
    assert (st < np.uint64(P)).all()
    ref = np.stack([oracle.poseidon_permute(r) for r in st])
    st.setflags(write=False)
    ref.setflags(write=False)
    return st, ref


@pytest.mark.parametrize("count", COUNTS)
def test_permute_counts(ctx, states, count):
    st, ref = states
    got = ctx.poseidon_permute(np.ascontiguousarray(st[:count]))
    assert got.shape == (count, 12)
    bad = np.nonzero((got != ref[:count]).any(axis=1))[0]
    assert bad.size == 0, "count %d: first mismatching state %d" % (count, bad[0])


def test_special_states_in_every_lane(ctx, states):
    """Each uniform special state and each one-element special state in all 64 lane positions of a wave"""
    st, ref = states
    n = 12 * len(SPECIAL) + len(SPECIAL)
    for shift in (0, 17, 32, 45):
        idx = (np.arange(256) + shift) % n
        got = ctx.poseidon_permute(np.ascontiguousarray(st[idx]))
        assert (got == ref[idx]).all(), shift


@pytest.mark.parametrize("count", [64, 65, 257])
def test_lane_pairs_do_not_leak(ctx, oracle, states, count):
    """Lanes l and l + 32 supply the same column of the matrix instruction from disjoint K blocks.  Every lane holds the same state except
    that lane l + 32 (and nothing else) differs in one element: every other lane must still produce the common result."""
    st, ref = states
    base, base_ref = st[999], ref[999]
    for l, e in [(0, 0), (5, 3), (31, 11), (17, 7)]:
        batch = np.tile(base, (count, 1))
        batch[l + 32, e] = np.uint64((int(base[e]) ^ 0x80FF7F01) % P)
        got = ctx.poseidon_permute(batch)
        want = np.tile(base_ref, (count, 1))
        want[l + 32] = oracle.poseidon_permute(batch[l + 32])
        assert (want[l + 32] != base_ref).any()
        assert (got == want).all(), (l, e, np.nonzero((got != want).any(axis=1))[0][:4])


def _lane_form_context():
    keys = ("GLP_MERKLE_COOP_MAX", "GLP_MERKLE_QUAD_MAX")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update({k: "0" for k in keys})
    try:
        return glp.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def lane_ctx():
    c = _lane_form_context()
    yield c
    c.close()


# rows = 2^(lg + rb) = 2^5 .. 2^8: half a wave, one wave, two, one whole workgroup
@pytest.mark.parametrize("lg,rb", [(5, 0), (5, 1), (6, 1), (7, 1)])
@pytest.mark.parametrize("ncols", [5, 8, 9, 20])
def test_leaf_hash_one_state_per_lane(lane_ctx, oracle, ncols, lg, rb):
    rng = np.random.default_rng(ncols * 1009 + 16 * lg + rb)
    vals = oracle.rand_field(rng, (ncols, 1 << lg))
    vals[:, 0] = np.array(SPECIAL, dtype=np.uint64)[np.arange(ncols) % len(SPECIAL)]
    ch = 2
    ref = oracle.batch_from_values(vals, rb, ch)
    b = lane_ctx.batch_from_values(vals, rb, ch)
    try:
        assert (b.digests() == ref.digests).all()
        assert (b.cap() == ref.cap).all()
    finally:
        b.free()


def test_tree_level_one_state_per_lane(lane_ctx, oracle):
    """2^15 leaves: the level of 2^14 parents is above the 12-lane form's limit and, with the quad form switched off, runs k_merkle_level;
    cap height 3 is odd, so the levels below it end on an odd count."""
    rng = np.random.default_rng(415)
    vals = oracle.rand_field(rng, (5, 1 << 12))
    ref = oracle.batch_from_values(vals, 3, 3)
    b = lane_ctx.batch_from_values(vals, 3, 3)
    try:
        assert (b.digests() == ref.digests).all()
        assert (b.cap() == ref.cap).all()
        for j in (0, 1, 12345, (1 << 15) - 1):
            assert (b.prove(j) == ref.prove(j)).all()
    finally:
        b.free()
