"""glp_fri_*: openings and FRI of caller-held batches on the GPU (include/glp.h).
A. The session pin: under the plonk instance built from glp_session_oracle's four batches, and the session's own challenges, the
   stepped and the one-call form reproduce glp_session_*'s openings, layer caps, final polynomial and proof words.
B. Instances the plonk prover never builds, word for word against tests/fri_restate.py (pinned on the CPU by test_fri_openings.py),
   whose verifier must accept.
C. Refusals."""
import ctypes as C

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
import plonky2_lib_amd.synth as synth
import fri_restate as fr
import zk_restate as zr
from test_fri_openings import shape_b

pytestmark = pytest.mark.gpu

SEED = [11, 22, 33, 44]
ACC_MAX_TERMS = 1024          # csrc/quotient_kernels.inc: the carry-free accumulators are flushed every so many terms


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    c.set_salt_seed(SEED)
    yield c
    c.close()


def _pow(ctx, ch, bits):
    st, pend = fr.challenger_state(ch)
    w = C.c_uint64()
    binding._chk(glp.load_library().glp_pow_search_h(ctx._h, ch.hasher, binding._p(st), binding._p(pend) if pend.size else None, pend.size,
                                                     int(bits), C.byref(w)))
    return int(w.value)


# ------------------------------------------------------------------ A. the session pin
def _session_pin(ctx, oracle, desc):
    hasher, nch, n_red = int(getattr(desc, "hasher", 0)), desc.num_challenges, len(desc.reduction_arity_bits)
    gc = glp.Circuit(ctx, desc)
    s = glp.Session(gc)
    ch = oracle.Challenger(hasher)
    ch.observe_hashes(gc.digest())
    ch.observe(s.public_inputs_hash)
    ch.observe_hashes(s.wires_cap)
    betas, gammas = ch.get_n(nch), ch.get_n(nch)
    ch.observe_hashes(s.partial_products(betas, gammas))
    ch.observe_hashes(s.quotient(ch.get_n(nch)))
    obs = [s.oracle(i) for i in range(4)]
    zk = bool(getattr(desc, "zero_knowledge", False))
    zeta = ch.get_ext()
    inst = fr.plonk_instance(desc, zeta, zk)
    assert [b.ncols for b in obs] == inst.ncols and [b.leaf_len for b in obs] == inst.leaf_len
    f = glp.FriOpenings(ctx, obs, inst.points, desc.reduction_arity_bits, desc.proof_of_work_bits, desc.num_query_rounds)
    op = s.open(zeta)
    want_op = fr.plonk_openings_to_points(desc, op)
    got_op = f.open()
    assert f.num_openings == inst.num_openings and (got_op == want_op).all()
    ch.observe(want_op)
    st, pend = fr.challenger_state(ch)                     # where glp_fri_prove resumes
    alpha = ch.get_ext()
    s.fri_combine(alpha); f.combine(alpha)
    for _ in range(n_red):
        cap = s.fri_commit()
        assert (f.commit() == cap).all()
        ch.observe_hashes(cap)
        beta = ch.get_ext()
        s.fri_fold(beta); f.fold(beta)
    fin = s.fri_final_poly()
    assert (f.final_poly() == fin).all()
    ch.observe(fin)
    w = _pow(ctx, ch, desc.proof_of_work_bits)
    ch.observe([w])
    assert ch.get() >> (64 - desc.proof_of_work_bits) == 0
    idx = [ch.get() % (1 << inst.lgN) for _ in range(desc.num_query_rounds)]
    s.queries(w, idx); f.queries(w, idx)
    proof, fproof = s.proof(), f.proof()
    start = 3 * (4 << desc.cap_height) + 2 * inst.num_openings
    want = proof[start:len(proof) - len(desc.public_inputs)]
    assert fproof.size == want.size == inst.layout()[5] == glp.fri_proof_words(obs, desc.reduction_arity_bits, desc.num_query_rounds)
    assert (fproof == want).all(), "first mismatch at FriProof word %d" % int(np.argmax(fproof != want))
    op1, proof1 = glp.fri_prove(ctx, obs, inst.points, desc.reduction_arity_bits, desc.proof_of_work_bits, desc.num_query_rounds, st, pend)
    assert (op1 == want_op).all() and (proof1 == want).all()
    if zk:                                                  # the salts ride at the end of the blinded oracles' leaves
        o_q = inst.layout()[0]
        at = o_q + inst.leaf_len[0] + 4 * (inst.lgN - inst.cap_height) + inst.ncols[1]
        assert (fproof[at:at + 4] == zr.salt(oracle, SEED, zr.TAG_WIRES, idx[0])).all()
    f.end(); s.end(); gc.free()


def _keccak(desc):
    desc.hasher, desc.circuit_digest = 1, None
    return desc


SESSION_CASES = {
    "arith 2^6 recursion config": lambda: synth.arith_circuit(6, synth.Config.standard_recursion_config(), seed=106),
    "arith 2^12 ecc config": lambda: synth.arith_circuit(12, synth.Config.standard_ecc_config(), seed=112),
    "keccak hasher": lambda: _keccak(synth.arith_circuit(7, synth.Config.standard_recursion_config(), seed=12)),
    "zero knowledge": lambda: synth.zkdsa_circuit(config=synth.Config.standard_recursion_zk_config(num_query_rounds=4)),
    "one challenge": lambda: synth.arith_circuit(8, synth.Config(135, 80, num_challenges=1), seed=31),
    "three challenges": lambda: synth.arith_circuit(8, synth.Config(135, 80, num_challenges=3), seed=31),
}


@pytest.mark.parametrize("case", list(SESSION_CASES))
def test_fri_reproduces_the_sessions_fri(ctx, oracle, case):
    _session_pin(ctx, oracle, SESSION_CASES[case]())


# ------------------------------------------------------------------ B. other shapes, against the restatement
def _commit_both(ctx, oracle, inst, coeffs):
    """every oracle on the GPU and in the restatement; a salted one goes through from_values_salted and the restated salt PRF"""
    gpu, ref = [], []
    for co, salted in zip(coeffs, inst.salted):
        if salted:
            vals = np.stack([oracle.fft(c) for c in co])
            gpu.append(ctx.batch_from_values_salted(vals, SEED, inst.rate_bits, inst.cap_height, inst.hasher))
            salts = zr.salt_columns(oracle, SEED, zr.TAG_BATCH, 1 << inst.lgN)
            ref.append(fr.commit(oracle, co, inst.rate_bits, inst.cap_height, inst.hasher, salts))
        else:
            gpu.append(ctx.batch_from_coeffs(co, inst.rate_bits, inst.cap_height, inst.hasher))
            ref.append(fr.commit(oracle, co, inst.rate_bits, inst.cap_height, inst.hasher))
        assert (gpu[-1].cap() == ref[-1].cap).all()
    return gpu, ref


def _against_restatement(ctx, oracle, inst, coeffs, rng):
    gpu, ref = _commit_both(ctx, oracle, inst, coeffs)
    ch = oracle.Challenger(inst.hasher)
    for o in ref:
        ch.observe_hashes(o.cap)
    ch.observe(oracle.rand_field(rng, 3))                  # leaves inputs pending in the sponge
    want_op, want = fr.prove_openings(oracle, inst, ref, fr.challenger_clone(oracle, ch))
    want_op = np.array(want_op, np.uint64)
    assert fr.verify_fri_proof(oracle, inst, [o.cap for o in ref], want_op, want, fr.challenger_clone(oracle, ch)) == 0
    args = (ctx, gpu, inst.points, inst.arity_bits, inst.pow_bits, inst.nq)
    # one call, the library's transcript
    st, pend = fr.challenger_state(ch)
    assert 0 < pend.size < 8
    op1, proof1 = glp.fri_prove(*args, st, pend)
    assert (op1 == want_op).all(), "first opening that differs: %d" % int(np.argmax((op1 != want_op).any(axis=1)))
    assert proof1.size == want.size and (proof1 == want).all(), "first mismatch at FriProof word %d" % int(np.argmax(proof1 != want))
    # stepped, the caller's transcript
    f = glp.FriOpenings(*args)
    assert (f.open() == want_op).all()
    ch2 = fr.challenger_clone(oracle, ch)
    f.combine(ch2.get_ext())
    capw = 4 << inst.cap_height
    for r in range(len(inst.arity_bits)):
        cap = f.commit()
        assert (cap.reshape(-1) == want[r * capw:(r + 1) * capw]).all()
        ch2.observe_hashes(cap)
        f.fold(ch2.get_ext())
    fin = f.final_poly()
    ch2.observe(fin)
    w = _pow(ctx, ch2, inst.pow_bits)
    ch2.observe([w])
    ch2.get()
    f.queries(w, [ch2.get() % (1 << inst.lgN) for _ in range(inst.nq)])
    assert (f.proof() == want).all()
    f.end()
    for b in gpu:
        b.free()


@pytest.mark.parametrize("cap_height", [0, 2])
@pytest.mark.parametrize("arity_bits", [[1, 2], [4]])
@pytest.mark.parametrize("log_n", [5, 8, 9])
def test_three_oracles_three_points(ctx, oracle, log_n, arity_bits, cap_height):
    """5, 3 (salted) and 41 columns; point 0 names oracle 0, oracle 2 [7, 41) and oracle 1; point 1 two ranges of oracle 2 that overlap
    point 0's; point 2 one column of the salted oracle.  2^5 (one partly idle workgroup), 2^8 (exactly one) and 2^9 points (two)."""
    rng = np.random.default_rng(1000 * log_n + 10 * len(arity_bits) + cap_height)
    inst, coeffs, _ = shape_b(rng, oracle, log_n, arity_bits, cap_height)
    _against_restatement(ctx, oracle, inst, coeffs, rng)


def test_four_points(ctx, oracle):
    """GLP_FRI_MAX_POINTS points, one of them twice the same point as another (one zeta table serves both)"""
    rng = np.random.default_rng(4)
    inst, coeffs, _ = shape_b(rng, oracle, 5, [2], 1)
    pts = inst.points + [(inst.points[0][0], [(0, 2, 3), (2, 40, 1)])]
    inst = fr.Instance(5, inst.rate_bits, 1, 0, inst.ncols, inst.salted, pts, [2], inst.pow_bits, inst.nq)
    _against_restatement(ctx, oracle, inst, coeffs, rng)


@pytest.mark.parametrize("log_n", [5, 8])
def test_more_columns_than_one_accumulator_flush(ctx, oracle, log_n):
    """one oracle of ACC_MAX_TERMS + 8 columns through the one-proof API (glp_fri_prove and the stepped handle); the second point
    names 12 columns around column ACC_MAX_TERMS.  2^5 points reach k_fri_combine_many_small: 8 lanes share a point and take 129
    program entries each, so this case pins the wide program there and no lane flushes.  2^8 points reach k_fri_combine_many: every
    lane walks all ACC_MAX_TERMS + 8 entries and crosses the accumulator flush."""
    rng = np.random.default_rng(5)
    ncols = ACC_MAX_TERMS + 8
    coeffs = [oracle.rand_field(rng, (ncols, 1 << log_n))]
    z = [tuple(int(v) for v in oracle.rand_field(rng, 2)) for _ in range(2)]
    inst = fr.Instance(log_n, 3, 1, 0, [ncols], [False], [(z[0], [(0, 0, ncols)]), (z[1], [(0, ACC_MAX_TERMS - 4, 12)])], [2, 1], 6, 2)
    _against_restatement(ctx, oracle, inst, coeffs, rng)


# ------------------------------------------------------------------ C. refusals
def _refused(ctx, oracles, points, arity_bits=(2,), pow_bits=4, nq=2):
    with pytest.raises(glp.GlpError) as e:
        glp.FriOpenings(ctx, oracles, points, list(arity_bits), pow_bits, nq)
    return e.value.code, str(e.value)


def test_begin_refusals(ctx, oracle):
    rng = np.random.default_rng(6)
    co = oracle.rand_field(rng, (3, 32))
    b = ctx.batch_from_coeffs(co, 3, 2)
    salted = ctx.batch_from_values_salted(co, SEED, 3, 2)
    z = (5, 9)
    ok = [(z, [(0, 0, 3)])]
    glp.FriOpenings(ctx, [b], ok, [2], 4, 2).end()
    cases = [
        (([], ok), "num_oracles"), (([b] * 9, ok), "num_oracles"),
        (([b], []), "num_points"), (([b], ok * 5), "num_points"),
        (([b], [(z, [(0, 0, 1)] * 17)]), "num_ranges"),
        (([b, ctx.batch_from_coeffs(oracle.rand_field(rng, (2, 64)), 3, 2)], ok), "log_n"),
        (([b, ctx.batch_from_coeffs(co, 2, 2)], ok), "rate_bits"),
        (([b, ctx.batch_from_coeffs(co, 3, 1)], ok), "cap_height"),
        (([b, ctx.batch_from_coeffs(co, 3, 2, hasher=1)], ok), "hasher"),
        (([b], [(z, [(1, 0, 1)])]), "oracle"),
        (([b], [(z, [(0, 2, 2)])]), "ncols"), (([b], [(z, [(0, 4, 0)])]), "ncols"),
        (([b, salted], [(z, [(1, 0, 4)])]), "salts are not polynomials"),
        (([b], [(z, [])]), "no polynomial"), (([b], [(z, [(0, 1, 0)])]), "no polynomial"),
        (([b], [(z, [(0, 0, 3)]), ((1, 2), [(0, 3, 0)])]), "points[1] names no polynomial"),
        (([b], [((glp.P, 0), [(0, 0, 3)])]), "canonical"),
    ]
    for (oracles, points), fragment in cases:
        code, msg = _refused(ctx, oracles, points)
        assert code == -1 and fragment in msg, (fragment, msg)
    for arity, fragment in (([3, 3], "above log_n"), ([0], "outside 1..4"), ([5], "outside 1..4"), ([2] * 17, "reductions")):
        code, msg = _refused(ctx, [b], ok, arity_bits=arity)
        assert code == -1 and fragment in msg, (fragment, msg)
    code, msg = _refused(ctx, [b], ok, nq=0)
    assert code == -1 and "num_query_rounds" in msg
    code, msg = _refused(ctx, [b], ok, pow_bits=33)
    assert code == -1 and "proof_of_work_bits" in msg
    other = glp.Context(0)
    foreign = other.batch_from_coeffs(co, 3, 2)
    code, msg = _refused(ctx, [b, foreign], ok)
    assert code == -1 and "ctx" in msg
    foreign.free(); other.close()
    h = C.c_void_p()
    assert glp.load_library().glp_fri_begin(ctx._h, None, C.byref(h)) == -1 and b"null" in glp.load_library().glp_last_error()
    # a point of the coset g H the commitments live on: x - z is not invertible there (GLP_ERR_PROVE, as zeta in the subgroup)
    on_coset = (7 * pow(oracle.root_of_unity(5), 3, glp.P) % glp.P, 0)
    code, msg = _refused(ctx, [b], [(z, [(0, 0, 3)]), (on_coset, [(0, 0, 1)])])
    assert code == -5 and "coset" in msg
    glp.FriOpenings(ctx, [b], [((on_coset[0], 1), [(0, 0, 1)])], [2], 4, 2).end()      # the same a with b != 0 is a fine point


def test_steps_out_of_order(ctx, oracle):
    rng = np.random.default_rng(7)
    b = ctx.batch_from_coeffs(oracle.rand_field(rng, (3, 32)), 3, 2)
    f = glp.FriOpenings(ctx, [b], [((5, 9), [(0, 0, 3)])], [2, 1], 0, 2)
    for early in (lambda: f.combine([1, 2]), f.commit, lambda: f.fold([1, 2]), f.final_poly, lambda: f.queries(0, [1, 2]), f.proof):
        with pytest.raises(glp.GlpError) as e:
            early()
        assert e.value.code == -1
    f.open()
    with pytest.raises(glp.GlpError):
        f.open()
    with pytest.raises(glp.GlpError):
        f.commit()
    with pytest.raises(glp.GlpError):
        f.combine([glp.P, 0])                              # not canonical
    f.combine([3, 4])
    with pytest.raises(glp.GlpError):
        f.fold([1, 2])                                     # no layer committed
    f.commit()
    with pytest.raises(glp.GlpError):
        f.commit()                                         # beta pending
    for bad in ([glp.P, 0], [1, 2 ** 64 - 1]):
        with pytest.raises(glp.GlpError) as e:
            f.fold(bad)                                    # not canonical
        assert e.value.code == -1 and "beta" in str(e.value) and "canonical" in str(e.value)
    with pytest.raises(glp.GlpError):
        f.final_poly()
    f.fold([1, 2]); f.commit(); f.fold([5, 6])
    with pytest.raises(glp.GlpError):
        f.commit()                                         # no layer left
    with pytest.raises(glp.GlpError):
        f.queries(0, [1, 2])
    assert f.final_poly().shape == (4, 2)
    with pytest.raises(glp.GlpError):
        f.queries(0, [1])                                  # two query rounds
    with pytest.raises(glp.GlpError):
        f.queries(0, [1, 1 << 8])                          # outside the LDE domain
    with pytest.raises(glp.GlpError):
        f.proof()
    f.queries(0, [1, 255])
    assert f.proof().size == glp.fri_proof_words([b], [2, 1], 2)
    f.end()
    b.free()


def test_session_oracle_before_its_stage(ctx):
    desc = synth.arith_circuit(5, synth.Config.standard_recursion_config(), seed=3)
    gc = glp.Circuit(ctx, desc)
    s = glp.Session(gc)
    nch = desc.num_challenges
    assert s.oracle(0).ncols == desc.num_constants + desc.num_routed_wires and s.oracle(1).ncols == desc.num_wires
    for i in (2, 3, 4):
        with pytest.raises(glp.GlpError) as e:
            s.oracle(i)
        assert e.value.code == -1
    s.partial_products([5] * nch, [7] * nch)
    zs = s.oracle(2)
    assert zs.ncols == nch * (1 + desc.num_partial_products) and zs.coeffs(0, 1).shape == (1, 32)
    with pytest.raises(glp.GlpError):
        s.oracle(3)
    s.quotient([9] * nch)
    q = s.oracle(3)
    assert q.ncols == nch * desc.quotient_degree_factor and (q.cap() == s.oracle(3).cap()).all()
    q.free()                                               # a borrowed handle: freeing the Batch leaves the session's oracle alone
    assert s.oracle(3).cap().shape == (1 << desc.cap_height, 4)
    s.end(); gc.free()
