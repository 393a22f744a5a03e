"""Column counts past what one launch carries, on every transform path.  The kernels of csrc/ntt.hip keep the column (or column x
coset plane x outer block) in grid.y, so an input of more than GRID_YZ_MAX = 65535 columns (ntt.h) goes through in several launches;
the pointer offsets of each split run from the second launch on only.  Many proofs in lock step are K * ncols columns (512 zkdsa
proofs of 135 wires: 69 120), so this is inside the advertised workload.  Which test reaches the second launch of which split:

  bitrev_copy, lde_to_natural (ntt.hip)           test_small_transforms, test_mid_transforms, test_tiled_* at W columns
  lde_coeffs -> lde_coeffs_chunk                  test_tiled_lde_across_the_split (4095 at rate_bits 4, 8191 at 3), test_tiled_fft_wide
                                                  (65535), test_many_proofs_tiled (member 60 straddles column 8191)
  intt_values_to_coeffs -> intt_chunk             test_tiled_inverse_wide (ifft, and coset_ifft through coset_planes_to_chunk_coeffs),
                                                  test_many_proofs_tiled_past_the_inverse_split (70 200 columns of 2^9 rows)
  batch_build, natural coefficients               test_many_proofs_small[coeffs] (70 200 columns)
  batch_build, strided copy after the wide LDE    test_many_proofs_small_salted
  glp_batch_coeffs                                test_one_wide_member_coeffs
  lde_sub_coset_rows, column-major                test_one_wide_member_lde_values
  coset_values_to_planes, k_quotient_combine      test_one_wide_member_from_coset_values (and coset_ifft at W columns for the latter)
  k_open_dot launches of one range                test_one_wide_member_openings
  host-upload chunks of unequal width             test_ragged_upload_chunks

Inputs and expected outputs: tests/wide_columns.py (every column different, 11 oracle transforms per case).  Everything is bit-exact
field arithmetic: no tolerance.  W = 70 001 is odd, past 65535 and 65536, and leaves a ragged last launch.

Out of scope: the row-major form of glp_batch_lde_values has a second loop, over row tiles, that starts a second launch only past
2^23 / column tiles rows: about 2^19 rows at this width, far more memory than a test should take."""
import time

import numpy as np
import pytest

import plonky2_lib_amd as glp
import fri_restate as fr
import wide_columns as wc

pytestmark = pytest.mark.gpu

P = glp.P
ROW, COL = glp.LDE_ROW_MAJOR, glp.LDE_COL_MAJOR
W = 70_001
TRIO = (65535, 65536, 65537)
SPLIT = wc.LAUNCH_MAX
SEED = [5, 6, 7, 8]


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    print("\n[wall] %s: %.2f s" % (request.node.name, time.perf_counter() - t0))


_CASES = {}


def _case(oracle, ncols, log_n):
    """(data, base, scale) of wide_columns.columns for this shape, made once and shared: nothing writes to it.  Only the latest
    large case is kept."""
    key = (ncols, log_n)
    if key not in _CASES:
        if ncols << log_n > 1 << 22:
            for k in [k for k in _CASES if k[0] << k[1] > 1 << 22]:
                del _CASES[k]
        data, base, scale = wc.columns(oracle, np.random.default_rng(1000 * log_n + ncols % 1000), ncols, 1 << log_n)
        for a in (data, base, scale):
            a.setflags(write=False)
        _CASES[key] = (data, base, scale)
    return _CASES[key]


def _transform(ctx, oracle, name, ncols, log_n, rate_bits=0, per=SPLIT):
    data, base, scale = _case(oracle, ncols, log_n)
    if name == "fft":
        got, T = ctx.fft(data), oracle.fft
    elif name == "ifft":
        got, T = ctx.ifft(data), oracle.ifft
    elif name == "coset_ifft":
        got, T = ctx.coset_ifft(data, 7), lambda c: oracle.coset_ifft(c, 7)
    else:
        got, T = ctx.lde(data, rate_bits, 7), lambda c: oracle.lde(c, rate_bits, 7)
    wc.check(got, wc.expected(oracle, T, base, scale, ncols), per, "%s, %d columns of 2^%d, rate_bits %d" % (name, ncols, log_n, rate_bits))


# ------------------------------------------------------------------ public transforms
@pytest.mark.parametrize("ncols", TRIO + (W,))
@pytest.mark.parametrize("log_n", [0, 1, 3, 4])
def test_small_transforms(ctx, oracle, log_n, ncols):
    """k_lde_small / k_intt_small, one thread per column in grid.x: the splits are those of bitrev_copy and k_quotient_combine"""
    for name in ("fft", "ifft", "coset_ifft"):
        _transform(ctx, oracle, name, ncols, log_n)


def test_small_lde_wide(ctx, oracle):
    _transform(ctx, oracle, "lde", W, 3, 3)


@pytest.mark.parametrize("name,rate_bits", [("fft", 0), ("ifft", 0), ("lde", 1)])
@pytest.mark.parametrize("log_n", [5, 8])
def test_mid_transforms(ctx, oracle, log_n, name, rate_bits):
    """k_lde_mid (column groups in grid.x) / k_intt_contig (column in grid.y: intt_chunk)"""
    _transform(ctx, oracle, name, W, log_n, rate_bits)


@pytest.mark.parametrize("rate_bits,ncols", [(4, 4095), (4, 4096), (4, 4100), (3, 8200)])
def test_tiled_lde_across_the_split(ctx, oracle, rate_bits, ncols):
    """log_n = 9, the smallest tiled size: lde_coeffs sends 65535 >> rate_bits columns to a launch"""
    _transform(ctx, oracle, "lde", ncols, 9, rate_bits, per=SPLIT >> rate_bits)


def test_tiled_fft_wide(ctx, oracle):
    _transform(ctx, oracle, "fft", W, 9)


@pytest.mark.parametrize("name", ["ifft", "coset_ifft"])
def test_tiled_inverse_wide(ctx, oracle, name):
    _transform(ctx, oracle, name, W, 9)


# ------------------------------------------------------------------ the commit path, K * ncols columns
def _members(oracle, K, ncols, log_n, tag):
    """[K][ncols][n], member k from a generator seeded with k: no two members are equal"""
    return np.stack([oracle.rand_field(np.random.default_rng([tag, k]), (ncols, 1 << log_n)) for k in range(K)])


def _same_words(a, b, what):
    assert (a.ncols, a.log_n, a.rate_bits, a.cap_height, a.leaf_len) == (b.ncols, b.log_n, b.rate_bits, b.cap_height, b.leaf_len), what
    wc.check(a.coeffs(), b.coeffs(), what="%s: coeffs()" % (what,))
    assert (a.digests() == b.digests()).all(), (what, "digests")
    assert (a.cap() == b.cap()).all(), (what, "cap")


def _many(ctx, oracle, kind, K, ncols, log_n, rb, ch, per, tag):
    """batch_many_from_<kind> against the K = 1 call on each probed member: member 0, the last, the member that holds column `per`
    (the first of the second launch) and its neighbours; member 0 against the oracle as well"""
    data = _members(oracle, K, ncols, log_n, tag)
    straddle = per // ncols
    assert straddle * ncols < per < (straddle + 1) * ncols < K * ncols, "no member straddles column %d" % per
    many = ctx.batch_many_from_values if kind == "values" else ctx.batch_many_from_coeffs
    one = ctx.batch_from_values if kind == "values" else ctx.batch_from_coeffs
    b = many(data, rb, ch)
    assert b.num_proofs == K
    for k in (0, straddle - 1, straddle, straddle + 1, K - 1):
        ref = one(data[k], rb, ch)
        _same_words(b.member(k), ref, (kind, "member", k, "columns from", k * ncols, "split at", per))
        ref.free()
    o = oracle.batch_from_values(data[0], rb, ch) if kind == "values" else oracle.batch_from_coeffs(data[0], rb, ch)
    m = b.member(0)
    assert (m.coeffs() == o.coeffs).all() and (m.digests() == o.digests).all() and (m.cap() == o.cap).all()
    b.free()


@pytest.mark.parametrize("kind", ["values", "coeffs"])
def test_many_proofs_small(ctx, oracle, kind):
    """520 members of 135 columns, 2^3 rows: 70 200 columns.  Natural coefficients go through bitrev_copy, split at 65535 (member 485)"""
    _many(ctx, oracle, kind, 520, 135, 3, 3, 2, SPLIT, 31)


@pytest.mark.parametrize("kind", ["values", "coeffs"])
def test_many_proofs_tiled(ctx, oracle, kind):
    """64 members of 135 columns, 2^9 rows: 8640 columns, the LDE split at 65535 >> 3 = 8191 inside member 60"""
    _many(ctx, oracle, kind, 64, 135, 9, 3, 4, SPLIT >> 3, 32)


def test_many_proofs_tiled_past_the_inverse_split(ctx, oracle):
    """520 members of 135 columns, 2^9 rows, rate_bits 0: 70 200 columns through intt_chunk and lde_coeffs_chunk, both split at 65535
    inside member 485.  Here alone the inverse transform's split stands without bitrev_copy's in front of or behind it: a member's
    coeffs() converts 135 columns."""
    _many(ctx, oracle, "values", 520, 135, 9, 0, 2, SPLIT, 34)


def test_many_proofs_small_salted(ctx, oracle):
    """the shape of test_many_proofs_small with salts: one wide LDE into scratch, then the strided copy into the salted leaves.
    Member k is salted with seed word 3 advanced by k."""
    K, ncols, log_n, rb, ch = 520, 135, 3, 3, 2
    data = _members(oracle, K, ncols, log_n, 33)
    b = ctx.batch_many_from_values(data, rb, ch, 0, SEED)
    assert b.num_proofs == K and b.leaf_len == ncols + 4
    straddle = SPLIT // ncols
    for k in (0, straddle - 1, straddle, straddle + 1, K - 1):
        ref = ctx.batch_from_values_salted(data[k], SEED[:3] + [(SEED[3] + k) % P], rb, ch)
        _same_words(b.member(k), ref, ("salted member", k))
        ref.free()
    b.free()


# ------------------------------------------------------------------ one member wider than a launch
@pytest.fixture(scope="module")
def wide_member(ctx, oracle):
    """batch_from_coeffs of W columns of two coefficients, rate_bits 1, cap_height 1: leaves of W words.
    (batch, coeffs [W][2], base, scale)"""
    co, base, scale = _case(oracle, W, 1)
    b = ctx.batch_from_coeffs(co, 1, 1)
    yield b, co, base, scale
    b.free()


def test_one_wide_member_coeffs(wide_member):
    b, co, _base, _scale = wide_member
    assert b.ncols == W and b.leaf_len == W
    wc.check(b.coeffs(), co, what="coeffs()")
    assert (b.coeffs(65530, 20) == co[65530:65550]).all()


def test_one_wide_member_tree(oracle, wide_member):
    """the four leaves of W words each, hashed by the oracle: every digest and the cap"""
    b, _co, base, scale = wide_member
    lde = wc.expected(oracle, lambda c: oracle.lde(c, 1), base, scale, W)              # [W][4], natural order
    leaves = np.ascontiguousarray(lde.T[oracle.bitrev_perm(2)])                      # leaf j is point bitrev(j)
    dig, cap = oracle.merkle_build(leaves, 1)
    assert (b.leaf(3) == leaves[3]).all()
    assert (b.digests() == dig).all() and (b.cap() == cap).all()


@pytest.mark.parametrize("sub_bits", [0, 1])
def test_one_wide_member_lde_values(oracle, wide_member, sub_bits):
    b, _co, base, scale = wide_member
    lde = wc.expected(oracle, lambda c: oracle.lde(c, 1), base, scale, W)              # [W][4], natural order
    exp = lde[:, ::1 << (1 - sub_bits)]                                              # exp[c][i] = p_c(g W_M^i), as test_gpu_coset_seam.py
    for cb, nc in ((0, W), (3, 65_990), (65_534, 4)):
        want = exp[cb:cb + nc]
        wc.check(b.lde_values(cb, nc, sub_bits, layout=COL), want, what="lde_values, column-major, columns from %d" % cb)
        got = b.lde_values(cb, nc, sub_bits, layout=ROW)
        assert got.shape == want.T.shape
        wc.check(got.T, want, what="lde_values, row-major, columns from %d" % cb)


def test_one_wide_member_from_coset_values(ctx, oracle, wide_member):
    """the same W polynomials given by their values on 7 <W_2> (sub_bits = 1, log_n = 0): W channels through coset_values_to_planes
    and k_quotient_combine, 2 W chunk columns through the commit, word for word what from_coeffs makes of the chunks"""
    _b, co, base, scale = wide_member
    values = wc.expected(oracle, lambda c: oracle.coset_fft(c, 7), base, scale, W)
    got = ctx.batch_from_coset_values(values, 1, 1, 1)
    want = ctx.batch_from_coeffs(co.reshape(2 * W, 1), 1, 1)
    assert got.num_proofs == 1 and got.ncols == 2 * W
    wc.check(got.coeffs(), co.reshape(2 * W, 1), what="from_coset_values: coeffs() against the polynomials")
    _same_words(got, want, "from_coset_values against from_coeffs on the chunks")
    got.free(); want.free()


def test_one_wide_member_openings(ctx, oracle, wide_member):
    """FriOpenings over the one oracle, one range of all W columns at one point: open() is c0 + c1 zeta in the quadratic extension"""
    b, co, _base, _scale = wide_member
    zeta = (0x123456789ABCDEF, 0xFEDCBA987654321)
    f = glp.FriOpenings(ctx, [b], [(zeta, [(0, 0, W)])], [], 0, 1)
    assert f.num_openings == W
    got = f.open()
    f.end()
    c0, c1 = np.ascontiguousarray(co[:, 0]), np.ascontiguousarray(co[:, 1])
    want = np.stack([oracle.vec_add(c0, oracle.vec_scale(c1, zeta[0])), oracle.vec_scale(c1, zeta[1])], axis=1)
    for j in (0, 1, SPLIT - 1, SPLIT, SPLIT + 1, W - 1):      # the vector form above is Horner's rule of tests/fri_restate.py
        assert tuple(int(v) for v in want[j]) == fr.eval_ext([int(v) for v in co[j]], zeta), j
    wc.check(got, want, what="open()")


# ------------------------------------------------------------------ host-upload chunks of unequal width
def test_ragged_upload_chunks(ctx, oracle):
    """11 columns of 2^20 rows are 88 MB: batch_build uploads them in min(8, ncols) chunks of ceil(11 / 8) = 2 columns: 2,2,2,2,2,1"""
    ncols, log_n, rb, ch = 11, 20, 1, 4
    vals = oracle.rand_field(np.random.default_rng(20), (ncols, 1 << log_n))
    b = ctx.batch_from_values(vals, rb, ch)
    d = ctx.dev_alloc(vals.nbytes)
    try:
        ctx.dev_upload(d, vals)
        ref = ctx.batch_from_values_device(d, ncols, log_n, rb, ch)
        _same_words(b, ref, "host upload in chunks against device input")
        ref.free()
    finally:
        ctx.dev_free(d)
    # against the oracle: the coefficients (the last chunk is column 10 alone), and two leaves as the polynomials' values at the
    # leaf's point, each with a Merkle path the oracle's verifier takes to the cap.  (The oracle's whole tree of 2^21 leaves takes
    # four times as long as everything else here.)
    co = np.stack([oracle.ifft(v) for v in vals])
    assert (b.coeffs(10, 1)[0] == co[10]).all()
    wc.check(b.coeffs(), co, 2, "coeffs() against the oracle")
    cap, lgN = b.cap(), log_n + rb
    for j in (1, (1 << lgN) - 2):
        leaf = b.leaf(j)
        x = fr.GEN * pow(oracle.root_of_unity(lgN), fr.brev(j, lgN), P) % P         # leaf j is point bitrev(j) of 7 <W_N>
        assert [int(v) for v in leaf] == _eval_columns(oracle, co, x), j
        assert oracle.merkle_verify(leaf, j, cap, b.prove(j)), j
    b.free()


def _eval_columns(oracle, coeffs, x):
    """[p_c(x)] for coeffs [ncols][n] in natural order: the powers of x by doubling, one vector product and one sum per column"""
    n = coeffs.shape[1]
    pw = np.ones(1, np.uint64)
    while pw.size < n:
        pw = np.concatenate([pw, oracle.vec_scale(pw, pow(x, pw.size, P))])
    out = []
    for c in coeffs:
        t = oracle.vec_mul(c, pw)                           # the sum of n < 2^32 words, taken in 32-bit halves so that neither overflows
        out.append((int((t & np.uint64(0xFFFFFFFF)).sum()) + (int((t >> np.uint64(32)).sum()) << 32)) % P)
    return out
