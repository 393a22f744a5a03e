"""Inputs of more columns than one launch carries, and what a per-column linear transform makes of them, without running the oracle
once per column.  The kernels of csrc/ntt.hip keep the column in grid.y (at most GRID_YZ_MAX = 65535 of them, ntt.h); a wider input
goes through in several launches, each with its own pointer offsets.  An offset that is wrong sends a launch to other columns, so
the columns here are made to differ from one another in a way the comparison can name:

    data[j] = scale[j] * base[j % distinct]

with `distinct` = 11 random base columns and ncols distinct non-zero scales.  Every transform under test (fft, ifft, coset_ifft, lde)
is linear per column, so column j of the result is scale[j] * T(base[j % distinct]): T runs 11 times, not ncols times.  11 is
coprime to 65535, 65536 and to every 65535 >> rate_bits (32767, 16383, 8191, 4095): a launch that starts at the wrong column, or reads
the first launch's columns again, lands on another base column and on another scale.  Test infrastructure:
tests/test_wide_columns.py holds the shortcut to the oracle column by column and shows that first_bad_column names the first column a
split error touches; tests/test_gpu_wide_columns.py takes its inputs and expected outputs from here."""
import numpy as np

P = 0xFFFFFFFF00000001
DISTINCT = 11
LAUNCH_MAX = 65535                  # GRID_YZ_MAX of csrc/ntt.h, restated


def _scaled(oracle, cols, scale, distinct):
    """out[j] = scale[j] * cols[j % distinct]: one vector multiplication"""
    ncols, m = scale.size, cols.shape[1]
    return oracle.vec_mul(np.repeat(scale, m), cols[np.arange(ncols) % distinct].reshape(-1)).reshape(ncols, m)


def columns(oracle, rng, ncols, n, distinct=DISTINCT):
    """(data [ncols][n], base [distinct][n], scale [ncols]): data[j] = scale[j] * base[j % distinct]"""
    base = oracle.rand_field(rng, (distinct, n))
    scale = oracle.rand_field(rng, (ncols,))
    while True:                                             # distinct and non-zero: redraw what is not (2^-64 events, but cheap to rule out)
        _, first = np.unique(scale, return_index=True)
        bad = np.ones(ncols, bool)
        bad[first] = False
        bad |= scale == 0
        if not bad.any():
            break
        scale[bad] = oracle.rand_field(rng, (int(bad.sum()),))
    return _scaled(oracle, base, scale, distinct), base, scale


def expected(oracle, T, base, scale, ncols):
    """[ncols][len(T(column))]: column j is scale[j] * T(base[j % distinct]), from len(base) calls of T"""
    assert scale.size == ncols
    return _scaled(oracle, np.stack([T(b) for b in base]), scale, base.shape[0])


def first_bad_column(got, want):
    """the first column (first index) in which got and want differ anywhere, None if they are equal; a shape mismatch is column 0"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return 0
    bad = (got != want).reshape(got.shape[0], -1).any(axis=1)
    return int(np.argmax(bad)) if bad.any() else None


def where(col, per=LAUNCH_MAX):
    """column `col` of an input that goes through `per` columns to a launch, in words for an assertion message"""
    launch, at = divmod(int(col), int(per))
    side = "the first launch" if launch == 0 else "launch %d (0-based), past the split at column %d" % (launch, launch * per)
    return "column %d = column %d of %s (%d columns per launch)" % (col, at, side, per)


def check(got, want, per=LAUNCH_MAX, what=""):
    """assert got == want column by column, naming the first wrong column and which side of which split it is on"""
    j = first_bad_column(got, want)
    assert j is None, "%s: shapes %s / %s, first wrong %s" % (what, np.shape(got), np.shape(want), where(j, per))
