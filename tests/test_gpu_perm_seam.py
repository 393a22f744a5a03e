"""The permutation argument at the commitment seam on the GPU (include/glp.h: glp_perm_zs_commit, glp_perm_quotient_values).
1. Z and the partial products, committed, against glp_batch_from_values / glp_batch_many_from_values on the values tests/coset_quotient.py
   computes: every launch path of the K5 kernels, host and device inputs, K proofs with salts.
2. the same against the library's own session.
3. the quotient's permutation share against tests/perm_restate.py::perm_quotient over rows from Batch.lde_values: every shape of 1 at full
   planes, S = 1 and S = 2 with chunks that fit them, a sigma range at an offset, salted oracles, K proofs with shared and per-proof
   sigmas, gate sums absent / host / device, output to host / device, both k_is paths.
4. the seam end to end with no session: only the gate constraints are computed outside the library.
5. every refusal, by field name, none of them reaching a launch.
The CPU side (the restatement pinned against coset_quotient.quotient_values) is tests/test_perm_seam.py."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
import coset_quotient as cq
import fri_restate as fr
import perm_restate as pr

pytestmark = pytest.mark.gpu

ROW = glp.LDE_ROW_MAJOR
SEED = [11, 12, 13, 14]
RB = 3

# (lg, wires, routed, chunk, challenges, plonky2's k_is = powers of 7 (the k_ratio chain) or random shifts (the general path))
SHAPES = {
    "2^3 x 135/80 chunk 8 nch 2": (3, 135, 80, 8, 2, True),        # k_pp_rows_small; a block of k_perm_quotient wider than the coset
    "2^4 x 20/13 chunk 5 nch 3": (4, 20, 13, 5, 3, False),          # ragged last chunk
    "2^9 x 30/24 chunk 8 nch 2": (9, 30, 24, 8, 2, True),           # k_pp_rows, two row blocks: the block scan matters
    "2^9 x 30/24 chunk 8 nch 1": (9, 30, 24, 8, 1, False),
}
# sub_bits below rate_bits: a chunk check has degree chunk + 1, so chunk <= 2^sub_bits (larger is refused: test_refusals)
SMALL_S = {
    "S = 1, 2^4 x 20/13 chunk 1 nch 3": (4, 20, 13, 1, 3, True, 0),      # "next" is row i + 1
    "S = 1, 2^9 x 30/24 chunk 1 nch 2": (9, 30, 24, 1, 2, False, 0),
    "S = 2, 2^4 x 20/13 chunk 2 nch 3": (4, 20, 13, 2, 3, False, 1),
    "S = 2, 2^9 x 30/24 chunk 2 nch 4": (9, 30, 24, 2, 4, True, 1),
}


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _rand(seed, shape):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)) % np.uint64(cq.P)


@functools.lru_cache(maxsize=None)
def _case(lg, nw, nr, chunk, nch, plonky2_k, wires_seed=None):
    """(description, betas, gammas, alphas, the restated Z / partial-product values): computed once per shape"""
    desc = pr.synthetic(lg, nw, nr, chunk, nch, seed=1000 * lg + 10 * nr + chunk, k_is=pr.plonky2_k_is(nr) if plonky2_k else None,
                        wires_seed=wires_seed)
    ch = _rand(17 * lg + nch + (wires_seed or 0), (3, nch))
    zp = cq.zs_partial_products(desc, desc.wires, ch[0], ch[1])
    return desc, ch[0], ch[1], ch[2], zp


def _cap_h(lg):
    return min(4, lg + RB)


def _same_batch(a, b, nleaves=6):
    assert (a.ncols, a.log_n, a.rate_bits, a.cap_height, a.leaf_len) == (b.ncols, b.log_n, b.rate_bits, b.cap_height, b.leaf_len)
    assert (a.cap() == b.cap()).all()
    assert (a.digests() == b.digests()).all()
    assert (a.coeffs() == b.coeffs()).all()
    for i in np.random.default_rng(3).integers(0, a.num_leaves, nleaves):
        assert (a.leaf(int(i)) == b.leaf(int(i))).all() and (a.prove(int(i)) == b.prove(int(i))).all()


def _on_device(ctx, arr):
    a = np.ascontiguousarray(arr, np.uint64)
    d = ctx.dev_alloc(a.nbytes)
    ctx.dev_upload(d, a)
    return d


def _first_diff(got, want):
    return "first mismatch at %s" % (tuple(np.argwhere(got != want)[0]) if (got != want).any() else None,)


# ------------------------------------------------------------------ 1. Z and the partial products against the restatement
@pytest.mark.parametrize("shape", list(SHAPES))
def test_zs_commit_is_from_values_on_the_restated_values(ctx, shape):
    lg, nw, nr, chunk, nch, pk = SHAPES[shape]
    desc, betas, gammas, _al, zp = _case(lg, nw, nr, chunk, nch, pk)
    assert glp.perm_num_polys(desc) == zp.shape[0]
    want = ctx.batch_from_values(zp, RB, _cap_h(lg))
    got = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, betas, gammas, RB, _cap_h(lg))
    assert got.num_proofs == 1 and got.ncols == zp.shape[0]
    _same_batch(got, want)
    got.free()
    dw, ds = _on_device(ctx, desc.wires), _on_device(ctx, desc.sigmas)
    try:
        got = ctx.perm_zs_commit(desc, None, None, betas, gammas, RB, _cap_h(lg), wires_dev_ptr=dw, sigmas_dev_ptr=ds)
        _same_batch(got, want)
        back = np.empty_like(desc.wires)
        ctx.dev_download(dw, back)
        assert (back == desc.wires).all(), "the caller's device wires were written to"
        got.free()
        got = ctx.perm_zs_commit(desc, desc.wires, None, betas, gammas, RB, _cap_h(lg), hasher=1, sigmas_dev_ptr=ds)      # one of each, Keccak
        wk = ctx.batch_from_values(zp, RB, _cap_h(lg), 1)
        _same_batch(got, wk)
        got.free(); wk.free()
    finally:
        ctx.dev_free(dw); ctx.dev_free(ds)
    want.free()


def _three(shape):
    """three witnesses of one circuit with their own challenges: (descs, betas [3][nch], gammas, alphas, zp [3][..][n])"""
    cases = [_case(*shape, wires_seed=ws) for ws in (None, 5, 6)]
    return ([c[0] for c in cases], np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), np.stack([c[3] for c in cases]),
            np.stack([c[4] for c in cases]))


@pytest.mark.parametrize("shape", ["2^3 x 135/80 chunk 8 nch 2", "2^4 x 20/13 chunk 5 nch 3", "2^9 x 30/24 chunk 8 nch 2"])
def test_zs_commit_of_three_salted_proofs(ctx, shape):
    lg = SHAPES[shape][0]
    descs, betas, gammas, _al, zp = _three(SHAPES[shape])
    assert (betas[0] != betas[1]).all() and (descs[0].sigmas == descs[2].sigmas).all()
    wires = np.stack([d.wires for d in descs])
    want = ctx.batch_many_from_values(zp, RB, _cap_h(lg), 0, SEED)
    got = ctx.perm_zs_commit(descs[0], wires, descs[0].sigmas, betas, gammas, RB, _cap_h(lg), 0, SEED)
    assert got.num_proofs == 3 and got.leaf_len == zp.shape[1] + 4
    assert (got.caps() == want.caps()).all()
    for k in range(3):
        _same_batch(got.member(k), want.member(k), 3)
    got.free()
    dw = _on_device(ctx, wires)
    try:
        got = ctx.perm_zs_commit(descs[0], None, descs[0].sigmas, betas, gammas, RB, _cap_h(lg), 0, SEED, wires_dev_ptr=dw)
        assert (got.caps() == want.caps()).all()
        got.free()
    finally:
        ctx.dev_free(dw)
    want.free()


# ------------------------------------------------------------------ 2. against the library's own session
def test_zs_commit_cap_is_the_sessions(ctx, oracle):
    desc = cq.seam_circuit(oracle)
    nch = int(desc.num_challenges)
    gc = glp.Circuit(ctx, desc)
    s = glp.Session(gc)
    ch = _rand(90, (2, nch))
    want = s.partial_products(ch[0], ch[1])
    got = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, ch[0], ch[1], int(desc.rate_bits), int(desc.cap_height))
    assert (got.cap() == np.asarray(want).reshape(-1, 4)).all()
    assert (got.digests() == s.oracle(2).digests()).all()
    got.free(); s.end(); gc.free()


# ------------------------------------------------------------------ 3. the quotient's permutation share
def _oracles(ctx, desc, betas, gammas, lg, front=0, seed=None):
    """(sigma oracle with `front` random columns before the sigmas, wires oracle, zs oracle)"""
    sg = np.concatenate([_rand(4, (front, 1 << lg)), desc.sigmas]) if front else desc.sigmas
    sb = ctx.batch_from_values(sg, RB, _cap_h(lg))
    wb = ctx.batch_from_values_salted(desc.wires, seed, RB, _cap_h(lg)) if seed else ctx.batch_from_values(desc.wires, RB, _cap_h(lg))
    zb = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, betas, gammas, RB, _cap_h(lg), seed=seed)
    return sb, wb, zb


def _rows(b, sub_bits, col_begin=0, ncols=None):
    return b.lde_values(col_begin, b.ncols - col_begin if ncols is None else ncols, sub_bits, layout=ROW)


def _check_quotient(ctx, desc, chal, sub_bits, lg, seed=None):
    betas, gammas, alphas = chal
    nch, nr, M = int(desc.num_challenges), int(desc.num_routed_wires), 1 << (lg + sub_bits)
    s0, wb, zb = _oracles(ctx, desc, betas, gammas, lg, 0, seed)
    s2 = ctx.batch_from_values(np.concatenate([_rand(4, (2, 1 << lg)), desc.sigmas]), RB, _cap_h(lg))
    assert wb.ncols > nr and wb.leaf_len == wb.ncols + (4 if seed else 0)
    rows = [_rows(s0, sub_bits), _rows(wb, sub_bits), _rows(zb, sub_bits)]
    assert (_rows(s2, sub_bits, 2) == rows[0]).all()
    gs = _rand(8, (nch, M))
    want = pr.perm_quotient(desc, rows[0], rows[1], rows[2], sub_bits, betas, gammas, alphas)
    want_gs = pr.perm_quotient(desc, rows[0], rows[1], rows[2], sub_bits, betas, gammas, alphas, gs)
    got = ctx.perm_quotient_values(desc, s0, 0, wb, zb, sub_bits, betas, gammas, alphas)
    assert got.shape == want.shape and (got == want).all(), _first_diff(got, want)
    got = ctx.perm_quotient_values(desc, s2, 2, wb, zb, sub_bits, betas, gammas, alphas, gs)
    assert (got == want_gs).all(), _first_diff(got, want_gs)
    dg, do = _on_device(ctx, gs), ctx.dev_alloc(want.nbytes)
    try:
        assert ctx.perm_quotient_values(desc, s0, 0, wb, zb, sub_bits, betas, gammas, alphas, gate_sums_dev_ptr=dg, out_dev_ptr=do) is None
        back = np.empty_like(want)
        ctx.dev_download(do, back)
        assert (back == want_gs).all(), _first_diff(back, want_gs)
        ctx.dev_download(dg, back)
        assert (back == gs).all(), "the caller's gate sums were written to"
    finally:
        ctx.dev_free(dg); ctx.dev_free(do)
    for b in (s0, s2, wb, zb):
        b.free()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_quotient_values_on_full_planes(ctx, shape):
    lg, nw, nr, chunk, nch, pk = SHAPES[shape]
    desc, betas, gammas, alphas, _zp = _case(lg, nw, nr, chunk, nch, pk)
    _check_quotient(ctx, desc, (betas, gammas, alphas), RB, lg)


@pytest.mark.parametrize("shape", list(SMALL_S))
def test_quotient_values_on_one_and_two_planes(ctx, shape):
    lg, nw, nr, chunk, nch, pk, sub_bits = SMALL_S[shape]
    desc, betas, gammas, alphas, _zp = _case(lg, nw, nr, chunk, nch, pk)
    _check_quotient(ctx, desc, (betas, gammas, alphas), sub_bits, lg)


def test_quotient_values_over_salted_oracles(ctx):
    lg, nw, nr, chunk, nch, pk = SHAPES["2^4 x 20/13 chunk 5 nch 3"]
    desc, betas, gammas, alphas, zp = _case(lg, nw, nr, chunk, nch, pk)
    zb = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, betas, gammas, RB, _cap_h(lg), seed=SEED)
    want = ctx.batch_from_values_salted(zp, SEED, RB, _cap_h(lg))
    _same_batch(zb, want)
    zb.free(); want.free()
    _check_quotient(ctx, desc, (betas, gammas, alphas), RB, lg, seed=SEED)      # salted wires and zs beside an unsalted sigma oracle


@pytest.mark.parametrize("shape", ["2^3 x 135/80 chunk 8 nch 2", "2^4 x 20/13 chunk 5 nch 3"])
def test_quotient_values_of_three_proofs_shared_and_per_proof_sigmas(ctx, shape):
    lg, nw, nr, chunk, nch, pk = SHAPES[shape]
    descs, betas, gammas, alphas, _zp = _three(SHAPES[shape])
    M = 1 << (lg + RB)
    wires = np.stack([d.wires for d in descs])
    front = _rand(4, (2, 1 << lg))
    sg = np.concatenate([front, descs[0].sigmas])
    s1 = ctx.batch_from_values(sg, RB, _cap_h(lg))
    s3 = ctx.batch_many_from_values(np.stack([sg] * 3), RB, _cap_h(lg))
    wb = ctx.batch_many_from_values(wires, RB, _cap_h(lg), 0, SEED)
    zb = ctx.perm_zs_commit(descs[0], wires, descs[0].sigmas, betas, gammas, RB, _cap_h(lg), 0, [9, 9, 9, 9])
    gs = _rand(21, (3, nch, M))
    shared = ctx.perm_quotient_values(descs[0], s1, 2, wb, zb, RB, betas, gammas, alphas, gs)
    per_proof = ctx.perm_quotient_values(descs[0], s3, 2, wb, zb, RB, betas, gammas, alphas, gs)
    assert shared.shape == (3, nch, M) and (shared == per_proof).all()
    srows = _rows(s1, RB, 2)
    for k in range(3):
        wk, zk = wb.member(k), zb.member(k)
        want = pr.perm_quotient(descs[k], srows, _rows(wk, RB), _rows(zk, RB), RB, betas[k], gammas[k], alphas[k], gs[k])
        assert (shared[k] == want).all(), (k, _first_diff(shared[k], want))
        if k == 1:        # a member view is a batch of one
            one = ctx.perm_quotient_values(descs[0], s1, 2, wk, zk, RB, betas[k], gammas[k], alphas[k], gs[k])
            assert one.shape == (nch, M) and (one == want).all()
    do = ctx.dev_alloc(shared.nbytes)
    try:
        ctx.perm_quotient_values(descs[0], s3, 2, wb, zb, RB, betas, gammas, alphas, gs, out_dev_ptr=do)
        back = np.empty_like(shared)
        ctx.dev_download(do, back)
        assert (back == shared).all()
    finally:
        ctx.dev_free(do)
    for b in (s1, s3, wb, zb):
        b.free()


# ------------------------------------------------------------------ 4. end to end, no session
def test_the_seam_end_to_end_without_a_session(ctx, oracle):
    desc = cq.seam_circuit(oracle)
    rb, chh, nch, nc = int(desc.rate_bits), int(desc.cap_height), int(desc.num_challenges), int(desc.num_constants)
    sub_bits = int(desc.quotient_degree_factor).bit_length() - 1
    cap = 4 << chh
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    digest = gc.digest()
    gc.free()
    pih = oracle.hash_no_pad(np.asarray(desc.public_inputs, np.uint64))
    cs = ctx.batch_from_values(np.concatenate([np.asarray(desc.constants, np.uint64), np.asarray(desc.sigmas, np.uint64)]), rb, chh)
    wb = ctx.batch_from_values(desc.wires, rb, chh)
    assert (wb.cap().reshape(-1) == proof[:cap]).all(), "the wires cap differs from glp_prove's"
    ch = oracle.Challenger(0)
    ch.observe_hashes(digest)
    ch.observe(pih)
    ch.observe_hashes(wb.cap())
    betas, gammas = ch.get_n(nch), ch.get_n(nch)
    zb = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, betas, gammas, rb, chh)
    assert (zb.cap().reshape(-1) == proof[cap:2 * cap]).all(), "the zs / partial products cap differs from glp_prove's"
    ch.observe_hashes(zb.cap())
    alphas = ch.get_n(nch)
    gs = pr.gate_sums(desc, _rows(cs, sub_bits, 0, nc), _rows(wb, sub_bits), alphas, pih)      # the caller's share: gate constraints alone
    q = ctx.perm_quotient_values(desc, cs, nc, wb, zb, sub_bits, betas, gammas, alphas, gs)
    qb = ctx.batch_from_coset_values(q, sub_bits, rb, chh)
    assert (qb.cap().reshape(-1) == proof[2 * cap:3 * cap]).all(), "the quotient cap differs from glp_prove's"
    ch.observe_hashes(qb.cap())
    zeta = ch.get_ext()
    inst = fr.plonk_instance(desc, zeta, False)
    start = 3 * cap + 2 * inst.num_openings
    want_op = fr.plonk_openings_to_points(desc, proof[3 * cap:start])
    ch.observe(want_op)
    st, pend = fr.challenger_state(ch)
    op, tail = glp.fri_prove(ctx, [cs, wb, zb, qb], inst.points, desc.reduction_arity_bits, desc.proof_of_work_bits, desc.num_query_rounds, st, pend)
    assert (op == want_op).all(), "first mismatch at opening word %d" % int(np.argmax(np.asarray(op).reshape(-1) != np.asarray(want_op).reshape(-1)))
    want = proof[start:len(proof) - len(desc.public_inputs)]
    assert tail.size == want.size and (tail == want).all(), "first mismatch at FriProof word %d" % int(np.argmax(tail != want))
    for b in (cs, wb, zb, qb):
        b.free()


# ------------------------------------------------------------------ 5. refusals
def _refused(fn, *needles):
    with pytest.raises(glp.GlpError) as e:
        fn()
    assert e.value.code == -1, str(e.value)                # GLP_ERR_ARG
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def test_refusals(ctx):
    L = glp.load_library()
    lg, nw, nr, chunk, nch, pk = SHAPES["2^4 x 20/13 chunk 5 nch 3"]
    desc, betas, gammas, alphas, zp = _case(lg, nw, nr, chunk, nch, pk)
    n, P = 1 << lg, cq.P
    sb, wb, zb = _oracles(ctx, desc, betas, gammas, lg, front=2)
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.stage_reset()

    def bag(**kw):
        d = dict(degree_bits=lg, num_wires=nw, num_routed_wires=nr, num_challenges=nch, quotient_degree_factor=chunk, k_is=desc.k_is)
        d.update(kw)
        return SimpleNamespace(**d)

    def zs(d=desc, wires=desc.wires, sigmas=desc.sigmas, b=betas, g=gammas, rb=RB, cap_height=4, hasher=0, seed=None):
        ctx.perm_zs_commit(d, wires, sigmas, b, g, rb, cap_height, hasher, seed).free()

    def qv(d=desc, s=sb, col=2, w=wb, z=zb, sub_bits=RB, b=betas, g=gammas, a=alphas, gs=None):
        ctx.perm_quotient_values(d, s, col, w, z, sub_bits, b, g, a, gs)

    def bad(v, i=1):
        v = np.array(v, np.uint64)
        v.reshape(-1)[i] = P + 3
        return v
    bad_k = bad(desc.k_is, 4)
    for call, name in ((zs, "glp_perm_zs_commit"), (qv, "glp_perm_quotient_values")):
        _refused(lambda: call(d=bag(quotient_degree_factor=0)), name, "chunk_size")
        _refused(lambda: call(d=bag(k_is=bad_k)), name, "k_is[4]", "canonical")
        _refused(lambda: call(b=bad(betas)), name, "betas[0][1]", "canonical")
        _refused(lambda: call(g=bad(gammas, 2)), name, "gammas[0][2]", "canonical")
    _refused(lambda: qv(a=bad(alphas, 0)), "alphas[0][0]", "canonical")
    # num_routed_wires of 0 or above num_wires; log_n: raw descriptions (the binding sizes its arrays by these fields)
    h, z8 = C.c_void_p(), np.arange(1, 9, dtype=np.uint64)

    def raw_zs(d, K=1, wires=desc.wires, sigmas=desc.sigmas, b=betas, g=gammas, rb=RB, cap_height=4, hasher=0, outp=C.byref(h)):
        p = lambda a: None if a is None else binding._p(np.ascontiguousarray(a, np.uint64))      # noqa: E731
        binding._chk(L.glp_perm_zs_commit(ctx._h, None if d is None else C.byref(d), K, p(wires), 0, p(sigmas), 0, p(b), p(g), rb, cap_height, hasher,
                                          None, outp))

    def raw_qv(d, K=1, s=sb, col=2, w=wb, z=zb, sub_bits=RB, b=betas, g=gammas, a=alphas, out=np.zeros(nch << (lg + RB), np.uint64)):
        p = lambda v: None if v is None else binding._p(np.ascontiguousarray(v, np.uint64))      # noqa: E731
        hh = lambda o: None if o is None else o._h                                                # noqa: E731
        binding._chk(L.glp_perm_quotient_values(ctx._h, None if d is None else C.byref(d), K, hh(s), col, hh(w), hh(z), sub_bits, p(b), p(g), p(a),
                                                None, 0, p(out), 0))

    def cdesc(**kw):
        d, keep = glp.perm_desc(desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    good = cdesc()
    for raw in (raw_zs, raw_qv):
        _refused(lambda: raw(None), "desc", "null")
        _refused(lambda: raw(cdesc(num_challenges=0)), "num_challenges")
        _refused(lambda: raw(cdesc(num_challenges=5)), "num_challenges")
        _refused(lambda: raw(cdesc(chunk_size=0)), "chunk_size")
        _refused(lambda: raw(cdesc(num_routed_wires=0)), "num_routed_wires")
        _refused(lambda: raw(cdesc(num_routed_wires=nw + 1)), "num_routed_wires", "num_wires")
        _refused(lambda: raw(cdesc(log_n=25)), "log_n")
        _refused(lambda: raw(cdesc(k_is=None)), "k_is", "null")
        _refused(lambda: raw(good, K=0), "num_proofs")
        _refused(lambda: raw(good, K=4097), "num_proofs")
        _refused(lambda: raw(good, b=None), "betas", "null")
        _refused(lambda: raw(good, g=None), "gammas", "null")
    _refused(lambda: raw_zs(good, wires=None), "wires", "null")
    _refused(lambda: raw_zs(good, sigmas=None), "sigmas", "null")
    _refused(lambda: raw_zs(good, outp=None), "out", "null")
    _refused(lambda: raw_zs(good, rb=5), "rate_bits")
    _refused(lambda: raw_zs(good, cap_height=lg + RB + 1), "cap_height")
    _refused(lambda: raw_zs(good, hasher=2), "hasher")
    assert not h.value
    _refused(lambda: raw_qv(good, s=None), "sigmas_oracle", "null")
    _refused(lambda: raw_qv(good, w=None), "wires_oracle", "null")
    _refused(lambda: raw_qv(good, z=None), "zs_oracle", "null")
    _refused(lambda: raw_qv(good, a=None), "alphas", "null")
    _refused(lambda: raw_qv(good, out=None), "out", "null")
    _refused(lambda: qv(sub_bits=RB + 1), "sub_bits", "rate_bits")
    _refused(lambda: qv(sub_bits=2), "chunk_size", "sub_bits")                          # chunk 5 > 2^2
    _refused(lambda: qv(d=bag(quotient_degree_factor=13)), "chunk_size")                # one chunk of 13 > 2^3
    _refused(lambda: qv(col=3), "sigma_col_begin", "sigmas_oracle")                     # 3 + 13 > 15 polynomials
    _refused(lambda: qv(col=0xFFFFFFFF), "sigma_col_begin")                             # no 32-bit wrap
    _refused(lambda: qv(d=bag(num_wires=nw + 1)), "wires_oracle", "num_wires")
    _refused(lambda: qv(d=bag(quotient_degree_factor=4)), "zs_oracle", "glp_perm_num_polys")        # 4 chunks: 12 polynomials, the oracle has 9
    _refused(lambda: qv(z=wb), "zs_oracle")
    assert ctx.stages() == [], "a refused call reached a launch: %s" % (ctx.stages(),)
    other_lg = ctx.batch_from_values(_rand(1, (nw, 2 * n)), RB, 4)
    other_rb = ctx.batch_from_values(desc.wires, 2, 4)
    salted_s = ctx.batch_from_values_salted(desc.sigmas, SEED, RB, 4)                    # 13 polynomials and 4 salts: the salts are not sigmas
    many = ctx.batch_many_from_values(np.stack([desc.wires] * 2), RB, 4)
    ctx2 = glp.Context(0)
    foreign = ctx2.batch_from_values(desc.wires, RB, 4)
    ctx.stage_reset()                                                                    # the commits above are not under test
    _refused(lambda: qv(w=other_lg), "log_n")
    _refused(lambda: qv(d=bag(degree_bits=lg + 1)), "log_n")
    _refused(lambda: qv(w=other_rb), "rate_bits")
    _refused(lambda: qv(s=salted_s, col=2), "sigma_col_begin", "salts")
    _refused(lambda: qv(w=many), "wires_oracle", "members")
    _refused(lambda: qv(z=many), "zs_oracle")
    _refused(lambda: qv(s=many, col=0), "sigmas_oracle", "members")
    _refused(lambda: qv(w=foreign), "ctx")
    b3 = np.stack([betas] * 3)
    _refused(lambda: qv(b=b3, g=b3, a=b3), "members", "num_proofs")                      # K = 3 over batches of one
    assert ctx.stages() == [], "a refused call reached a launch: %s" % (ctx.stages(),)
    ctx.set_profiling(False)
    qv()                                                                                 # and the unrefused call is served
    foreign.free(); ctx2.close()
    for b in (other_lg, other_rb, salted_s, many, sb, wb, zb):
        b.free()
