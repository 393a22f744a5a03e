"""glp_running_columns (include/glp.h) against tests/running_restate.py: helper columns, running column and totals, every word.  Fixed
seeds.  The boundaries of the implementation (csrc/running_columns.inc) each n hits:
    n = 2       k_run_small with 62 of its 64 lanes past the last row (they enter the scan as the identity)
    n = 16      k_run_small, one partly filled wave
    n = 256     k_run_small at its edge: the largest column one workgroup owns, four full waves, a scan of eight steps
    n = 512     the three-step scan at its smallest: k_run_terms, two block totals, k_run_scan_tot, k_run_apply
    n = 2^17    512 block totals: k_run_scan_tot walks two totals per lane, so the scan of the totals itself is past one wave of blocks
with T = 1, 3, 64 terms, A = 1, 3 arguments, K = 1, 3 proofs, both kinds, nums NULL and given, packed and loose strides.
Then boundary values, zero denominators, refusals, and the permutation argument of the seam circuit: its product-kind Z, committed,
has the cap glp_perm_zs_commit returns for chunk_size = num_routed_wires.  (That circuit has 80 routed wires and num_terms is at
most 64, so term t is the product of the factors of wires 2 t and 2 t + 1; tests/test_running_columns.py pins that this is the same Z.)
The CPU side is tests/test_running_columns.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
import plonky2_lib_amd.gl_numpy as gl
import coset_quotient as cq
import running_restate as rr

pytestmark = pytest.mark.gpu

P = cq.P
SUM, PRODUCT = glp.RUN_SUM, glp.RUN_PRODUCT


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _rand(seed, shape):
    return gl.rand(np.random.default_rng(seed), shape)


def _nonzero(seed, shape):
    v = _rand(seed, shape)
    v[v == 0] = 1
    return v


def _first_diff(got, want):
    return "first mismatch at %s" % (tuple(np.argwhere(got != want)[0]) if (got != want).any() else None,)


def _want(kind, nums, dens):
    """the restatement, proof by proof: nums, dens [K][A][T][n]"""
    parts = [rr.running_columns(kind, None if nums is None else nums[k], dens[k]) for k in range(dens.shape[0])]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def _on_device(ctx, arr):
    a = np.ascontiguousarray(arr, np.uint64)
    d = ctx.dev_alloc(a.nbytes)
    ctx.dev_upload(d, a)
    return d


# (kind, log_n, K, A, T, nums given)
CASES = [
    (SUM, 1, 1, 1, 1, False), (PRODUCT, 1, 3, 3, 3, True),
    (SUM, 4, 3, 3, 3, True), (PRODUCT, 4, 1, 1, 1, False), (SUM, 4, 3, 1, 64, True),
    (SUM, 8, 1, 3, 3, False), (PRODUCT, 8, 3, 1, 3, True), (PRODUCT, 8, 1, 1, 64, True),
    (SUM, 9, 3, 3, 3, True), (PRODUCT, 9, 1, 3, 1, False), (PRODUCT, 9, 3, 1, 3, True), (SUM, 9, 1, 1, 64, False),
    (SUM, 17, 1, 1, 1, True), (PRODUCT, 17, 1, 1, 1, True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s n=2^%d K=%d A=%d T=%d nums %s" % ((("sum", "product")[c[0]],) + c[1:5] + (("NULL", "given")[c[5]],)))
def test_columns_and_totals_are_the_restatement(ctx, case):
    kind, lg, K, A, T, given = case
    n = 1 << lg
    dens = _nonzero(1000 * lg + 10 * T + A, (K, A, T, n))
    nums = _rand(2000 * lg + 10 * T + K, (K, A, T, n)) if given else None
    want, want_tot = _want(kind, nums, dens)
    got, tot = ctx.running_columns(kind, nums, dens)
    assert got.shape == want.shape == (K, A, T + 1, n) and tot.shape == (K, A)
    assert (got == want).all(), _first_diff(got, want)
    assert (tot == want_tot).all(), (tot, want_tot)
    ident = 0 if kind == SUM else 1
    assert (got[:, :, T, 0] == ident).all()


@pytest.mark.parametrize("lg", [4, 9], ids=["n = 16, one launch", "n = 512, three steps"])
@pytest.mark.parametrize("kind", [SUM, PRODUCT], ids=["sum", "product"])
def test_pass_through_layout_from_hbm_to_hbm_with_a_loose_stride(ctx, kind, lg):
    """dens then nums of a proof in one block, as a rows program that EMITs all denominators and then all numerators leaves them, the
    proofs 2 A T n + 24 words apart; words >= p among them; the output in HBM, as glp_batch_many_from_values takes it"""
    K, A, T, n = 3, 3, 3, 1 << lg
    per = A * T * n
    stride = 2 * per + 24
    buf = np.zeros((K, stride), np.uint64)                      # the slack stays zero: were it read, a zero denominator would be reported
    buf[:, :per] = _nonzero(70 + lg, (K, per))
    buf[:, per:2 * per] = _rand(80 + lg, (K, per))
    buf[:, :2 * per:5] &= np.uint64(0x7FFFFFFF)                 # values v with p + v < 2^64 ...
    buf[:, :per][buf[:, :per] == 0] = 1
    dens, nums = buf[:, :per].reshape(K, A, T, n).copy(), buf[:, per:2 * per].reshape(K, A, T, n).copy()
    want, want_tot = _want(kind, nums, dens)
    hb = buf.copy()
    buf[:, :2 * per:5] += np.uint64(P)                          # ... written as p + v in HBM
    assert (buf[:, :2 * per:5] >= np.uint64(P)).all()
    db = _on_device(ctx, buf)
    do = ctx.dev_alloc(want.nbytes)
    try:
        out, tot = ctx.running_columns(kind, None, None, K, A, T, lg, stride, nums_dev_ptr=db + 8 * per, dens_dev_ptr=db, out_dev_ptr=do)
        assert out is None and (tot == want_tot).all(), (tot, want_tot)
        back = np.empty_like(want)
        ctx.dev_download(do, back)
        assert (back == want).all(), _first_diff(back, want)
        b = ctx.batch_many_from_values(want.reshape(K, A * (T + 1), n), 3, 4)      # and the layout is the commitment's: [K][A (T + 1)][n]
        assert b.num_proofs == K and b.ncols == A * (T + 1)
        b.free()
        again = np.empty_like(buf)
        ctx.dev_download(db, again)
        assert (again == buf).all(), "the caller's inputs were written to"
    finally:
        ctx.dev_free(do); ctx.dev_free(db)
    # host memory with a loose stride: a raw call
    tot = np.zeros((K, A), np.uint64)
    out = np.zeros_like(want)
    p_ = binding._p
    binding._chk(glp.load_library().glp_running_columns(ctx._h, kind, K, A, T, lg, C.c_void_p(hb.ctypes.data + 8 * per), p_(hb), stride, 0, p_(out), 0, p_(tot)))
    assert (out == want).all() and (tot == want_tot).all()


@pytest.mark.parametrize("lg", [4, 9])
@pytest.mark.parametrize("kind", [SUM, PRODUCT], ids=["sum", "product"])
def test_boundary_values(ctx, kind, lg):
    n = 1 << lg
    pairs = [(num, den) for den in (1, P - 1) for num in (0, 1, P - 1)]
    dens = np.array([[den] * n for _num, den in pairs], np.uint64)
    nums = np.array([[num] * n for num, _den in pairs], np.uint64)
    if kind == PRODUCT:                                         # without the zero numerators too: a product that stays alive
        pairs += [(num, den) for den in (1, P - 1) for num in (1, P - 1)]
        dens = np.stack([dens, np.array([[den] * n for _num, den in pairs[6:]] + [[1] * n] * 2, np.uint64)])
        nums = np.stack([nums, np.array([[num] * n for num, _den in pairs[6:]] + [[P - 1] * n, [1] * n], np.uint64)])
    else:
        dens, nums = dens[None], nums[None]
    want, want_tot = rr.running_columns(kind, nums, dens)
    got, tot = ctx.running_columns(kind, nums, dens)
    assert (got == want).all(), _first_diff(got, want)
    assert (tot[0] == want_tot).all()
    for t, (num, den) in enumerate(pairs[:6]):                  # 1 / (p - 1) = p - 1, in plain integers
        assert (got[0, t] == np.uint64(num * den % P)).all(), (num, den)
    if kind == SUM:                                             # each row adds 0 + 1 - 1 + 0 - 1 + 1 = 0
        assert (got[0, 6] == 0).all() and tot[0, 0] == 0
    else:                                                       # the second argument's rows multiply by (-1)^3: Z alternates 1, -1
        assert (got[1, 6, 0::2] == 1).all() and (got[1, 6, 1::2] == np.uint64(P - 1)).all() and tot[0, 1] == 1 and (got[0, 6, 1:] == 0).all()


@pytest.mark.parametrize("lg", [4, 9], ids=["n = 16, one launch", "n = 512, three steps"])
def test_the_first_zero_denominator_is_named_and_a_repaired_call_succeeds(ctx, lg):
    K, A, T, n = 3, 3, 3, 1 << lg
    dens, nums = _nonzero(7, (K, A, T, n)), _rand(8, (K, A, T, n))
    row = n - 6
    bad = dens.copy()
    bad[1, 2, 0, row] = 0                                       # the smaller (k, a, t, i), though its row is the larger one
    bad[1, 2, 1, 5] = 0
    for kind in (SUM, PRODUCT):
        with pytest.raises(glp.GlpError) as e:
            ctx.running_columns(kind, nums, bad)
        assert e.value.code == -5, str(e.value)                 # GLP_ERR_PROVE
        assert "glp_running_columns" in str(e.value) and "proof 1, argument 2, term 0, row %d" % row in str(e.value), str(e.value)
        want, want_tot = _want(kind, nums, dens)
        got, tot = ctx.running_columns(kind, nums, dens)       # repaired: served
        assert (got == want).all() and (tot == want_tot).all()
    db = _on_device(ctx, bad + np.where(bad == 0, np.uint64(P), np.uint64(0)))      # in HBM, the zeros written as p
    do = ctx.dev_alloc(8 * K * A * (T + 1) * n)
    try:
        with pytest.raises(glp.GlpError) as e:
            ctx.running_columns(SUM, None, None, K, A, T, lg, dens_dev_ptr=db, out_dev_ptr=do)
        assert e.value.code == -5 and "proof 1, argument 2, term 0, row %d" % row in str(e.value), str(e.value)
    finally:
        ctx.dev_free(db); ctx.dev_free(do)


def test_the_permutation_arguments_z_has_the_cap_of_perm_zs_commit(ctx, oracle):
    desc = cq.seam_circuit(oracle)
    nch, nr, n = int(desc.num_challenges), int(desc.num_routed_wires), 1 << int(desc.degree_bits)
    rb, chh = int(desc.rate_bits), int(desc.cap_height)
    ch = _rand(31, (2, nch))
    one_chunk = SimpleNamespace(degree_bits=desc.degree_bits, num_wires=desc.num_wires, num_routed_wires=nr, num_challenges=nch,
                                quotient_degree_factor=nr, k_is=desc.k_is)
    assert glp.perm_num_polys(one_chunk) == nch
    zb = ctx.perm_zs_commit(one_chunk, desc.wires, desc.sigmas, ch[0], ch[1], rb, chh)
    terms = [rr.permutation_terms(desc, desc.wires, ch[0][a], ch[1][a], pair=True) for a in range(nch)]
    nums, dens = np.stack([t[0] for t in terms]), np.stack([t[1] for t in terms])
    assert dens.shape == (nch, nr // 2, n) and nr // 2 <= 64 < nr
    out, tot = ctx.running_columns(PRODUCT, nums, dens)
    assert (tot == 1).all()
    mine = ctx.batch_from_values(out[:, nr // 2], rb, chh)
    assert (mine.cap() == zb.cap()).all() and (mine.digests() == zb.digests()).all()
    mine.free(); zb.free()


def _refused(fn, *needles):
    with pytest.raises(glp.GlpError) as e:
        fn()
    assert e.value.code == -1, str(e.value)                # GLP_ERR_ARG
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def test_refusals(ctx):
    L = glp.load_library()
    name = "glp_running_columns"
    K, A, T, lg, n = 3, 3, 3, 4, 16
    per = A * T * n
    dens, nums = _nonzero(7, (K, A, T, n)), _rand(8, (K, A, T, n))
    out, tot = np.zeros((K, A, T + 1, n), np.uint64), np.zeros((K, A), np.uint64)
    p_ = binding._p
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.stage_reset()

    def raw(c=ctx._h, kind=SUM, K_=K, A_=A, T_=T, lg_=lg, nm=nums, dn=dens, stride=per, o=out, t=tot):
        binding._chk(L.glp_running_columns(c, kind, K_, A_, T_, lg_, None if nm is None else p_(nm), None if dn is None else p_(dn), stride, 0,
                                           None if o is None else p_(o), 0, None if t is None else p_(t)))

    def bad(v, i):
        v = np.array(v, np.uint64)
        v.reshape(-1)[i] = P + 3
        return v
    _refused(lambda: raw(c=None), name, "ctx", "null")
    _refused(lambda: raw(dn=None), name, "dens", "null")
    _refused(lambda: raw(o=None), name, "out", "null")
    _refused(lambda: raw(t=None), name, "totals_out", "null")
    _refused(lambda: raw(kind=2), name, "kind = 2", "GLP_RUN_")
    _refused(lambda: raw(K_=0), name, "num_proofs")
    _refused(lambda: raw(K_=4097), name, "num_proofs")
    _refused(lambda: raw(A_=0), name, "num_args = 0", "1..16")
    _refused(lambda: raw(A_=17), name, "num_args = 17", "1..16")
    _refused(lambda: raw(T_=0), name, "num_terms = 0", "1..64")
    _refused(lambda: raw(T_=65), name, "num_terms = 65", "1..64")
    _refused(lambda: raw(lg_=25), name, "log_n = 25")
    _refused(lambda: raw(K_=4096, A_=16, T_=64, lg_=24), name, "out too large")
    _refused(lambda: raw(stride=per - 1), name, "in_proof_stride = %d" % (per - 1), "%d" % per)
    _refused(lambda: raw(stride=(1 << 33) + 1), name, "in_proof_stride", "2^33")
    _refused(lambda: raw(dn=bad(dens, per + 7)), name, "dens", "proof 1", "word 7", "canonical")
    _refused(lambda: raw(nm=bad(nums, 2 * per + per - 1)), name, "nums", "proof 2", "word %d" % (per - 1), "canonical")
    assert ctx.stages() == [], "a refused call reached a launch: %s" % (ctx.stages(),)
    raw()                                                        # one launch at n = 16 ...
    assert [s[0] for s in ctx.stages()] == ["running.terms"]
    want, want_tot = _want(SUM, nums, dens)
    assert (out == want).all() and (tot == want_tot).all()
    ctx.stage_reset()
    ctx.running_columns(SUM, None, _nonzero(9, (1, 2, 512)))    # ... and the two stages of the three-step scheme above 256 rows
    assert [s[0] for s in ctx.stages()] == ["running.terms", "running.scan"]
    ctx.set_profiling(False)
