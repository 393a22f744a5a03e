"""The caller's quotient at the commitment seam (include/glp.h): glp_batch_lde_values, glp_coset_ifft and
glp_batch_from_coset_values on the GPU.
1. lde_values against oracle.lde and against the Merkle leaves, every sub_bits, both layouts, ragged windows, host and device output.
2. many-proof batches: the parent call is the member views' calls stacked.
3. coset_ifft against oracle.coset_ifft, and glp_lde(rate_bits = 0) as its inverse.
4. from_coset_values word for word against from_coeffs on the chunks (one proof, K proofs with salts, Keccak, device input).
5. the prover's own quotient, read back and sent through from_coset_values, reproduces the session's quotient oracle.
6. the seam end to end: a quotient computed by tests/coset_quotient.py from lde_values rows, committed with from_coset_values and
   FRI-proved with glp_fri_prove, reproduces glp_prove's proof.  Nothing of the library's quotient runs.
7. refusals."""
import ctypes as C

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
import plonky2_lib_amd.synth as synth
import coset_quotient as cq
import fri_restate as fr

pytestmark = pytest.mark.gpu

ROW, COL = glp.LDE_ROW_MAJOR, glp.LDE_COL_MAJOR
SEED = [5, 6, 7, 8]


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def _dev_lde_values(ctx, b, K, col_begin, num_cols, sub_bits, row_begin, num_rows, layout):
    """the same call with out_on_device: glp_dev_alloc, the asynchronous call, glp_dev_download (which synchronises the stream)"""
    inner = (num_rows, num_cols) if layout == ROW else (num_cols, num_rows)
    out = np.zeros(((K,) + inner) if K > 1 else inner, np.uint64)
    d = ctx.dev_alloc(out.nbytes)
    try:
        assert b.lde_values(col_begin, num_cols, sub_bits, row_begin, num_rows, layout, dev_ptr=d) is None
        ctx.dev_download(d, out)
    finally:
        ctx.dev_free(d)
    return out


def _windows(M, ncols):
    """(col_begin, num_cols, row_begin, num_rows): full, unaligned (where it fits), ending at M, a column sub-range"""
    w = [(0, ncols, 0, M)]
    if M >= 40:
        w.append((0, ncols, 3, 37))
    w.append((0, ncols, M - min(M, 5), min(M, 5)))
    if ncols >= 3:
        w.append((1, ncols - 2, 1 if M > 1 else 0, M - 1 if M > 1 else 1))
    return w


# ------------------------------------------------------------------ 1. lde_values
LDE_CASES = {
    "2^2 x 1, rate 1": (2, 1, 1, None, 0),
    "2^5 x 3": (5, 3, 3, None, 0),
    "2^7 x 37": (7, 37, 3, None, 0),
    "2^9 x 18, rate 2, salted": (9, 18, 2, SEED, 0),
    "2^12 x 5, keccak": (12, 5, 3, None, 1),
    # beyond the issue's table: a coset shorter than the 128-row tile takes a tile of its own height (16, 32, 64 rows by 256, 128, 64
    # columns); 135 columns are ragged in each and more than one column tile in the last two
    "2^3 x 135, short cosets": (3, 135, 3, None, 0),
}


@pytest.mark.parametrize("case", list(LDE_CASES))
def test_lde_values_against_the_oracle_and_the_leaves(ctx, oracle, case):
    log_n, ncols, rb, seed, hasher = LDE_CASES[case]
    rng = np.random.default_rng(log_n * 100 + ncols)
    vals = oracle.rand_field(rng, (ncols, 1 << log_n))
    cap_h = min(4, log_n + rb)
    b = ctx.batch_from_values_salted(vals, seed, rb, cap_h, hasher) if seed else ctx.batch_from_values(vals, rb, cap_h, hasher)
    lde = np.stack([oracle.lde(oracle.ifft(v), rb) for v in vals])                  # [ncols][N], natural order
    assert b.leaf_len == ncols + (4 if seed else 0)
    for sub_bits in range(rb + 1):
        step, M = 1 << (rb - sub_bits), 1 << (log_n + sub_bits)
        exp = lde[:, ::step]                                                        # exp[c][i] = p_c(g W_M^i)
        for cb, nc, r0, nr in _windows(M, ncols):
            want = exp[cb:cb + nc, r0:r0 + nr]
            for layout in (ROW, COL):
                w = want.T if layout == ROW else want
                got = b.lde_values(cb, nc, sub_bits, r0, nr, layout)
                assert got.shape == w.shape and (got == w).all(), (sub_bits, cb, nc, r0, nr, layout)
                got = _dev_lde_values(ctx, b, 1, cb, nc, sub_bits, r0, nr, layout)
                assert (got == w).all(), ("device", sub_bits, cb, nc, r0, nr, layout)
        full = b.lde_values(0, ncols, sub_bits)                                     # defaults: every row, row-major
        for i in rng.integers(0, M, 16):
            leaf = b.leaf(_bitrev(int(i) * step, log_n + rb))
            assert (full[int(i)] == leaf[:ncols]).all(), (sub_bits, int(i))
    b.free()


# ------------------------------------------------------------------ 2. many-proof batches
def test_lde_values_of_a_many_proof_batch(ctx, oracle):
    K, log_n, ncols, rb = 3, 5, 6, 3
    vals = oracle.rand_field(np.random.default_rng(2), (K, ncols, 1 << log_n))
    b = ctx.batch_many_from_values(vals, rb, 4, 0, SEED)
    assert b.num_proofs == K and b.leaf_len == ncols + 4
    views = [b.member(k) for k in range(K)]
    for sub_bits in (0, 2, 3):
        step, M = 1 << (rb - sub_bits), 1 << (log_n + sub_bits)
        for layout in (ROW, COL):
            for cb, nc, r0, nr in ((0, ncols, 0, M), (2, 3, 3, min(37, M - 3))):
                got = b.lde_values(cb, nc, sub_bits, r0, nr, layout)
                stacked = np.stack([v.lde_values(cb, nc, sub_bits, r0, nr, layout) for v in views])
                assert got.shape == stacked.shape and (got == stacked).all(), (sub_bits, layout, cb, r0)
                assert (_dev_lde_values(ctx, b, K, cb, nc, sub_bits, r0, nr, layout) == stacked).all()
        want = np.stack([oracle.lde(oracle.ifft(v), rb)[::step] for v in vals[1]])  # member 1 against the oracle as well
        assert (views[1].lde_values(0, ncols, sub_bits, layout=COL) == want).all()
    b.free()


# ------------------------------------------------------------------ 3. coset_ifft
@pytest.mark.parametrize("ncols", [1, 5])
@pytest.mark.parametrize("log_n", [0, 1, 4, 8, 12, 13])
def test_coset_ifft(ctx, oracle, log_n, ncols):
    rng = np.random.default_rng(31 * log_n + ncols)
    vals = oracle.rand_field(rng, (ncols, 1 << log_n))
    for shift in (7, int(oracle.rand_field(rng, (1,))[0]) or 3):
        got = ctx.coset_ifft(vals, shift)
        want = np.stack([oracle.coset_ifft(v, shift) for v in vals])
        assert (got == want).all(), (log_n, ncols, shift)
        assert (ctx.lde(got, 0, shift) == vals).all()


# ------------------------------------------------------------------ 4. from_coset_values against from_coeffs
def _coset_case(oracle, rng, K, num_polys, log_n, sub_bits):
    """random polynomials of degree < M: (values on g <W_M> [K][num_polys][M], their chunks [K][num_polys << sub_bits][n])"""
    n, M = 1 << log_n, 1 << (log_n + sub_bits)
    coeffs = oracle.rand_field(rng, (K, num_polys, M))
    values = np.stack([np.stack([oracle.coset_fft(p, 7) for p in member]) for member in coeffs])
    return values, coeffs.reshape(K, num_polys << sub_bits, n)


def _same_batch(a, b, rng, nleaves=8):
    assert (a.ncols, a.log_n, a.rate_bits, a.cap_height, a.leaf_len) == (b.ncols, b.log_n, b.rate_bits, b.cap_height, b.leaf_len)
    assert (a.coeffs() == b.coeffs()).all()
    assert (a.cap() == b.cap()).all()
    assert (a.digests() == b.digests()).all()
    for i in rng.integers(0, a.num_leaves, nleaves):
        assert (a.leaf(int(i)) == b.leaf(int(i))).all() and (a.prove(int(i)) == b.prove(int(i))).all()


@pytest.mark.parametrize("log_n", [2, 5, 9, 12])
def test_from_coset_values_is_from_coeffs_on_the_chunks(ctx, oracle, log_n):
    rng = np.random.default_rng(400 + log_n)
    cases = [(p, s, 3) for p in (1, 2, 3) for s in (0, 1, 3)] + [(2, 2, 2)]
    for num_polys, sub_bits, rb in cases:
        values, chunks = _coset_case(oracle, rng, 1, num_polys, log_n, sub_bits)
        got = ctx.batch_from_coset_values(values[0], sub_bits, rb, 4)
        want = ctx.batch_from_coeffs(chunks[0], rb, 4)
        assert got.num_proofs == 1 and got.ncols == num_polys << sub_bits
        _same_batch(got, want, rng)
        got.free(); want.free()


def test_from_coset_values_many_proofs_salted(ctx, oracle):
    rng = np.random.default_rng(44)
    K, num_polys, log_n, sub_bits, rb = 4, 2, 5, 3, 3
    values, chunks = _coset_case(oracle, rng, K, num_polys, log_n, sub_bits)
    got = ctx.batch_from_coset_values(values, sub_bits, rb, 4, 0, SEED)
    want = ctx.batch_many_from_coeffs(chunks, rb, 4, 0, SEED)
    assert got.num_proofs == K and got.leaf_len == want.leaf_len == (num_polys << sub_bits) + 4
    assert (got.caps() == want.caps()).all()
    for k in range(K):
        _same_batch(got.member(k), want.member(k), rng, 4)
    # the result is a batch like any other: item 1 takes it, member by member and as a whole
    rows = got.lde_values(0, got.ncols, sub_bits, layout=COL)
    for k in range(K):
        lde = np.stack([oracle.lde(c, rb)[::1 << (rb - sub_bits)] for c in chunks[k]])
        assert (rows[k] == lde).all()
    got.free(); want.free()


def test_from_coset_values_keccak_and_device_input(ctx, oracle):
    rng = np.random.default_rng(45)
    num_polys, log_n, sub_bits, rb = 2, 9, 3, 3
    values, chunks = _coset_case(oracle, rng, 1, num_polys, log_n, sub_bits)
    got = ctx.batch_from_coset_values(values[0], sub_bits, rb, 4, hasher=1)
    want = ctx.batch_from_coeffs(chunks[0], rb, 4, hasher=1)
    _same_batch(got, want, rng)
    got.free(); want.free()
    want = ctx.batch_from_coeffs(chunks[0], rb, 4)
    for sb, vals, ref in ((sub_bits, values[0], want), (0, values[0][:, :1 << log_n], None)):
        v = np.ascontiguousarray(vals)
        d = ctx.dev_alloc(v.nbytes)
        ctx.dev_upload(d, v)
        got = ctx.batch_from_coset_values(None, sb, rb, 4, dev_ptr=d, shape=v.shape)
        back = np.empty_like(v)
        ctx.dev_download(d, back)
        assert (back == v).all(), "the caller's device values were written to"
        if ref is None:                                     # sub_bits = 0 reads the caller's buffer in place: a plain coset iFFT
            ref = ctx.batch_from_coeffs(np.stack([oracle.coset_ifft(p, 7) for p in v]), rb, 4)
        _same_batch(got, ref, rng)
        got.free(); ref.free()
        ctx.dev_free(d)


# ------------------------------------------------------------------ 5. the prover's own quotient
def _transcript_to_alphas(oracle, gc, s, desc):
    nch = desc.num_challenges
    ch = oracle.Challenger(int(getattr(desc, "hasher", 0)))
    ch.observe_hashes(gc.digest())
    ch.observe(s.public_inputs_hash)
    ch.observe_hashes(s.wires_cap)
    betas, gammas = ch.get_n(nch), ch.get_n(nch)
    ch.observe_hashes(s.partial_products(betas, gammas))
    return ch, betas, gammas, ch.get_n(nch)


def test_the_provers_quotient_through_from_coset_values(ctx, oracle):
    desc = synth.arith_circuit(6, synth.Config.standard_recursion_config(), seed=106)
    qdf, nch, n = int(desc.quotient_degree_factor), int(desc.num_challenges), 1 << int(desc.degree_bits)
    sub_bits = qdf.bit_length() - 1
    assert 1 << sub_bits == qdf
    gc = glp.Circuit(ctx, desc)
    s = glp.Session(gc)
    _ch, _b, _g, alphas = _transcript_to_alphas(oracle, gc, s, desc)
    s.quotient(alphas)
    q = s.oracle(3)
    polys = q.coeffs().reshape(nch, qdf * n)                # chunk j of polynomial p is column p * qdf + j
    values = np.stack([oracle.coset_fft(p, 7) for p in polys])
    got = ctx.batch_from_coset_values(values, sub_bits, int(desc.rate_bits), int(desc.cap_height))
    assert (got.cap() == q.cap()).all() and (got.digests() == q.digests()).all()
    got.free(); s.end(); gc.free()


# ------------------------------------------------------------------ 6. the seam end to end
def test_the_seam_end_to_end(ctx, oracle):
    desc = cq.seam_circuit(oracle)
    rb, chh, nch = int(desc.rate_bits), int(desc.cap_height), int(desc.num_challenges)
    sub_bits = int(desc.quotient_degree_factor).bit_length() - 1
    cap = 4 << chh
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    s = glp.Session(gc)
    ch, betas, gammas, alphas = _transcript_to_alphas(oracle, gc, s, desc)
    obs = [s.oracle(i) for i in range(3)]
    rows = [b.lde_values(0, b.ncols, sub_bits, layout=ROW) for b in obs]
    q = cq.quotient_values(desc, rows[0], rows[1], rows[2], sub_bits, betas, gammas, alphas, s.public_inputs_hash)
    qb = ctx.batch_from_coset_values(q, sub_bits, rb, chh)
    assert (qb.cap().reshape(-1) == proof[2 * cap:3 * cap]).all(), "the quotient cap differs from glp_prove's"
    ch.observe_hashes(qb.cap())
    zeta = ch.get_ext()
    inst = fr.plonk_instance(desc, zeta, False)
    start = 3 * cap + 2 * inst.num_openings
    want_op = fr.plonk_openings_to_points(desc, proof[3 * cap:start])
    ch.observe(want_op)
    st, pend = fr.challenger_state(ch)                     # where glp_fri_prove resumes
    op, tail = glp.fri_prove(ctx, obs + [qb], inst.points, desc.reduction_arity_bits, desc.proof_of_work_bits, desc.num_query_rounds, st, pend)
    assert (op == want_op).all()
    want = proof[start:len(proof) - len(desc.public_inputs)]
    assert tail.size == want.size and (tail == want).all(), "first mismatch at FriProof word %d" % int(np.argmax(tail != want))
    qb.free(); s.end(); gc.free()


# ------------------------------------------------------------------ 7. refusals
def _refused(fn, *needles):
    with pytest.raises(glp.GlpError) as e:
        fn()
    assert e.value.code == -1, str(e.value)                # GLP_ERR_ARG
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def test_refusals(ctx, oracle):
    L = glp.load_library()
    vals = oracle.rand_field(np.random.default_rng(7), (3, 32))
    b = ctx.batch_from_values_salted(vals, SEED, 3, 4)      # ncols = 3, leaves of 7 words, M up to 256
    out = np.zeros(4096, np.uint64)

    def raw(col_begin, num_cols, sub_bits, row_begin, num_rows, layout, o=out, batch=b):
        binding._chk(L.glp_batch_lde_values(batch._h if batch else None, col_begin, num_cols, sub_bits, row_begin, num_rows, layout,
                                            binding._p(o) if o is not None else None, 0))
    _refused(lambda: raw(0, 1, 0, 0, 1, ROW, batch=None), "null")
    _refused(lambda: raw(0, 1, 0, 0, 1, ROW, o=None), "out", "null")
    _refused(lambda: raw(0, 0, 0, 0, 1, ROW), "num_cols")
    _refused(lambda: raw(0, 1, 0, 0, 0, ROW), "num_rows")
    _refused(lambda: raw(1, 3, 0, 0, 1, ROW), "col_begin", "ncols")          # past the polynomials
    _refused(lambda: raw(0, 7, 0, 0, 1, ROW), "ncols")                       # the leaf is 7 words wide: the salts are not served
    _refused(lambda: raw(0xFFFFFFFF, 2, 0, 0, 1, ROW), "ncols")              # no 32-bit wrap
    _refused(lambda: raw(0, 1, 4, 0, 1, ROW), "sub_bits")                    # rate_bits + 1
    _refused(lambda: raw(0, 1, 3, 200, 57, ROW), "row_begin", "M")           # 257 > M = 256
    _refused(lambda: raw(0, 1, 0, 32, 1, COL), "row_begin", "M")             # M = 32 at sub_bits = 0
    _refused(lambda: raw(0, 1, 0, 1, 0xFFFFFFFFFFFFFFFF, COL), "row_begin")  # no 64-bit wrap
    _refused(lambda: raw(0, 1, 0, 0, 1, 2), "layout")
    b.lde_values(0, 3, 3, 200, 56)                                          # the window that ends at M is served
    b.free()

    v = oracle.rand_field(np.random.default_rng(8), (2, 64))
    h = C.c_void_p()

    def commit(values=v, K=1, num_polys=2, log_n=3, sub_bits=3, rb=3, cap_height=4, outp=C.byref(h)):
        binding._chk(L.glp_batch_from_coset_values(ctx._h, binding._p(values) if values is not None else None, 0, K, num_polys, log_n, sub_bits,
                                                   rb, cap_height, 0, None, outp))
    _refused(lambda: commit(values=None), "values", "null")
    _refused(lambda: commit(outp=None), "out", "null")
    _refused(lambda: commit(K=0), "num_proofs")
    _refused(lambda: commit(K=4097), "num_proofs")
    _refused(lambda: commit(num_polys=0), "num_polys")
    _refused(lambda: commit(sub_bits=4, log_n=2), "sub_bits")
    _refused(lambda: commit(cap_height=7), "cap_height")
    assert not h.value

    for shift in (0, cq.P, cq.P + 6):
        _refused(lambda: ctx.coset_ifft(v, shift), "shift")
