"""The vanishing identity at zeta for caller-held circuits on the GPU (include/glp.h: glp_gate_program_eval_ext, glp_perm_check_zeta).
Fixed seeds; every comparison is word for word against the restatements of tests/gate_program_ext_restate.py (pinned to
zeta_identity.check by tests/test_zeta_check.py), never against the library's own verifier.
1. programs traced from the gate bodies, on the openings of glp_prove proofs, one, two and four challenges, one proof and three proofs
   of different witnesses.
2. a random program: every operand kind on both sides, 24 registers all live, an instruction count that is no multiple of 4, gates of
   1, 0 and 1 500 EMITs, COL_NEXT on one oracle only (the others hand in no at_next), a proof_stride larger than the columns;
   K = 1, 63, 64, 65 and 129: one wave with dead lanes, a full wave, and one lane past one and past two blocks of 64.
3. boundary values: openings and points with the components 0, 1, p - 1, points with second component 0.
4. the whole check on glp_prove proofs, the gate sums handed over in HBM: accepted, and one word changed in every opening section
   gives zeta_identity.check's verdict; three proofs with one damaged; zeta = 1; the seam end to end with no glp_circuit on the
   verifying side; every refusal by name, before any launch."""
import ctypes as C
import functools

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
from plonky2_lib_amd import gate_program as gp
import plonky2_lib_amd.gl_numpy as gl
import plonky2_lib_amd.synth as synth
import coset_quotient as cq
import fri_restate as fr
import gate_program_ext_restate as gx
import gate_program_restate as gr
import zeta_identity as zi
import zeta_identity_recursion as zr

pytestmark = pytest.mark.gpu

P = zi.P
SECTIONS = ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q")
ORACLE_COLS = (5, 17, 3)
NEXT_ORACLE = 1                                                    # the only oracle whose COL_NEXT the random program reads
NUM_PARAMS = 3
BLOCK = 64                                                         # proofs per block of k_gate_program_ext


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _rand(seed, shape):
    return gl.rand(np.random.default_rng(seed), shape)


def _as_words(pairs):
    return np.array(pairs, np.uint64).reshape(-1, 2)


# ------------------------------------------------------------------ proofs of the three circuits, three witnesses each
def _descs(name):
    from oracle import oracle
    oracle.build()
    pi = [5, 1 << 44]
    if name == "arith":                                            # another seed is another circuit of the same gates: the program is the same
        return [synth.arith_circuit(4, synth.Config.standard_ecc_config(), seed=23 + k, public_inputs=pi, pi_hash=oracle.hash_no_pad(pi)) for k in range(3)]
    if name == "ext":
        return [synth.ext_gates_circuit(4, witness_seed=None if k == 0 else 100 + k) for k in range(3)]
    return [synth.recursion_gates_circuit(5, synth.Config.standard_recursion_config(), witness_seed=None if k == 0 else 200 + k) for k in range(3)]


@pytest.fixture(scope="module")
def proved(ctx):
    """name -> (descs, traced program, checker, proofs, digests, GateProgram): glp_prove's proofs of three witnesses"""
    made = {}

    def get(name):
        if name not in made:
            descs = _descs(name)
            prog = gx.trace_circuit(descs[0], zr.gate_constraints) if name == "recursion" else gr.trace_circuit(descs[0])[0]
            proofs, digests = [], []
            for d in descs:
                gc = glp.Circuit(ctx, d)
                proofs.append(np.array(gc.prove(), np.uint64))
                digests.append(np.array(gc.digest(), np.uint64))
                gc.free()
            made[name] = (descs, prog, zr.check if name == "recursion" else zi.check, proofs, digests, ctx.gate_program(prog))
        return made[name]
    yield get
    for m in made.values():
        m[5].free()


def _fri_order(desc, proof):
    """the proof's opening section in the order of glp_fri_open, [count][2]"""
    lay = zi.proof_layout(desc)
    start = lay["constants"][0]
    count = sum(lay[s][1] for s in SECTIONS)
    return fr.plonk_openings_to_points(desc, np.asarray(proof, np.uint64)[start:start + 2 * count])


def _restated_sums(desc, prog, proof, zeta, alphas, pih):
    op = gx.proof_openings(desc, proof)
    return gx.run_ext(prog, [op["constants"] + op["sigmas"], op["wires"]], None, zeta, alphas, pih)


# ------------------------------------------------------------------ 1. traced programs at zeta
@pytest.mark.parametrize("nch", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["arith", "ext", "recursion"])
def test_traced_programs_at_zeta(ctx, proved, name, nch):
    descs, prog, _check, proofs, digests, g = proved(name)
    K = len(descs)
    ch = [zi.challenges(d, p, dig) for d, p, dig in zip(descs, proofs, digests)]
    zetas = np.array([c[3] for c in ch], np.uint64)
    pihs = np.array([c[4] for c in ch], np.uint64)
    alphas = _rand(10 * nch + len(name), (K, nch))
    want = np.array([_restated_sums(descs[k], prog, proofs[k], ch[k][3], alphas[k], ch[k][4]) for k in range(K)], np.uint64)
    assert want.shape == (K, nch, 2) and want.any() and (want[0] != want[1]).any() and (want[1] != want[2]).any()
    ops = np.stack([_fri_order(descs[k], proofs[k]) for k in range(K)])
    parts = glp.plonk_ext_openings(descs[0], ops)
    got = g.eval_ext(zetas, parts["program"], alphas, pihs)
    assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:1]
    one = g.eval_ext(zetas[0], glp.plonk_ext_openings(descs[0], ops[0])["program"], alphas[0], pihs[0])      # K = 1
    assert one.shape == (nch, 2) and (one == want[0]).all()


# ------------------------------------------------------------------ 2. a random program
@functools.lru_cache(maxsize=None)
def _random_program(seed=7, long_gate=1500):
    """tests/test_gpu_gate_program.py's generator with COL_NEXT on one oracle only: 24 virtual registers that all stay alive to the last
    gate, so every result overwrites a register that is still in use"""
    rng = np.random.default_rng(seed)
    asm = gp.Assembler(ORACLE_COLS, NUM_PARAMS)
    regs = [asm.reg() for _ in range(gp.MAX_REGS)]
    ops = (asm.add, asm.sub, asm.mul)

    def col():
        o = int(rng.integers(len(ORACLE_COLS)))
        return asm.col(o, int(rng.integers(ORACLE_COLS[o])))

    def col_next():
        return asm.col_next(NEXT_ORACLE, int(rng.integers(ORACLE_COLS[NEXT_ORACLE])))

    def imm():
        return asm.imm(int(rng.integers(0, 1 << 63)) * 2 % P if rng.integers(4) else [0, 1, P - 1][int(rng.integers(3))])

    def reg():
        return regs[int(rng.integers(len(regs)))]
    makers = (reg, col, col_next, imm, lambda: asm.param(int(rng.integers(NUM_PARAMS))), lambda: asm.x)

    def operand(live_regs=True):
        return makers[int(rng.integers(0 if live_regs else 1, len(makers)))]()
    for i, r in enumerate(regs):                               # first writes: no register operand yet
        ops[i % 3](r, operand(False), operand(False))
    for ka, ma in enumerate(makers):                           # every operand kind on both sides, under every operation
        for kb, mb in enumerate(makers):
            ops[(ka + kb) % 3](reg(), ma(), mb())
    asm.mul(regs[3], regs[3], regs[3])                         # both operands and the destination one register
    asm.sub(regs[4], regs[5], regs[4])
    asm.mov(regs[6], regs[7])
    asm.emit(regs[0])                                          # a gate of 1 EMIT
    asm.end(regs[1])
    asm.end(asm.x)                                             # a gate of 0 EMITs
    for j in range(long_gate):                                 # a gate of 1 500 EMITs, operands of every kind
        ops[int(rng.integers(3))](reg(), operand(), operand())
        asm.emit(operand())
    asm.end(col())
    for j in range(400):
        ops[int(rng.integers(3))](reg(), operand(), operand())
        if j % 7 == 0:
            asm.mov(reg(), operand())
        if j % 5 == 0:
            asm.emit(operand())
        if j % 97 == 96:
            asm.end(operand())
    for r in regs:                                             # all 24 read at the very end: all alive throughout
        asm.emit(r)
    asm.end(asm.imm(1))
    n = len(asm._ins)
    if n % 4 == 0:                                             # the last load of four instruction words is partly padding
        asm._ins.insert(n - 1, gp.Instruction(gp.OP_EMIT, None, asm.x, None))
    prog = asm.assemble()
    assert prog.num_regs == prog.max_live == gp.MAX_REGS and prog.max_constraints == long_gate and len(prog) > 2 * long_gate and len(prog) % 4
    kinds = {(side, o.kind) for i in prog.instructions for side, o in (("a", i.a), ("b", i.b)) if o is not None}
    assert kinds == {(s, k) for s in "ab" for k in range(6)}
    assert {o.oracle for i in prog.instructions for o in (i.a, i.b) if o is not None and o.kind == gp.COL_NEXT} == {NEXT_ORACLE}
    assert {o.oracle for i in prog.instructions for o in (i.a, i.b) if o is not None and o.kind == gp.COL} == {0, 1, 2}
    return prog


K_MAX = 2 * BLOCK + 1
PAD = 3                                                            # words between one proof's openings and the next one's


@functools.lru_cache(maxsize=None)
def _random_case():
    """openings [K_MAX] of random canonical words, each oracle in an array of its own with PAD spare words per proof, the openings at
    w_n * point in a second plane of it; and the restated interpreter's result for every proof, computed once"""
    prog = _random_program()
    arrays = [_rand(60 + o, (K_MAX, 2, 2 * c + PAD)) for o, c in enumerate(ORACLE_COLS)]
    points, alphas, params = _rand(71, (K_MAX, 2)), _rand(72, (K_MAX, 2)), _rand(73, (K_MAX, NUM_PARAMS))
    for a in arrays + [points]:                                    # some words below 2^64 - p: v + p is another 64-bit word for the same element
        a[..., 1] >>= np.uint64(33)
    want = np.array([gx.run_ext(prog, [gx.pairs(a[k, 0, :2 * c]) for a, c in zip(arrays, ORACLE_COLS)],
                                [gx.pairs(a[k, 1, :2 * c]) for a, c in zip(arrays, ORACLE_COLS)], points[k], alphas[k], params[k])
                     for k in range(K_MAX)], np.uint64)
    return prog, arrays, points, alphas, params, want


def _random_openings(arrays, next_oracles=(NEXT_ORACLE,)):
    return [glp.ExtOpenings(a, 0, 2 * c + PAD if o in next_oracles else None, 2 * (2 * c + PAD)) for o, (a, c) in enumerate(zip(arrays, ORACLE_COLS))]


@pytest.mark.parametrize("K", [1, BLOCK - 1, BLOCK, BLOCK + 1, K_MAX])
def test_random_program_is_the_restated_interpreter(ctx, K):
    prog, arrays, points, alphas, params, want = _random_case()
    assert glp.gate_program_check(prog) == 1500
    g = ctx.gate_program(prog)
    got = g.eval_ext(points[:K], _random_openings(arrays), alphas[:K], params[:K])
    assert got.shape == (K, 2, 2) and (got == want[:K]).all(), np.argwhere(got != want[:K])[:1]
    g.free()


def test_device_inputs_and_device_output(ctx):
    """the same call over HBM: openings, points and out; words >= p among device inputs are reduced as they are loaded"""
    prog, arrays, points, alphas, params, want = _random_case()
    K = BLOCK + 1
    g = ctx.gate_program(prog)
    lifted = [a[:K].copy() for a in arrays]
    pts = points[:K].copy()
    for a in lifted:                                               # v < 2^64 - p stays below 2^64 as v + p
        small = a < np.uint64((1 << 64) - P)
        a[small] += np.uint64(P)
        assert small.any()
    small = pts < np.uint64((1 << 64) - P)
    pts[small] += np.uint64(P)
    bufs = [ctx.dev_alloc(a.nbytes) for a in lifted] + [ctx.dev_alloc(pts.nbytes), ctx.dev_alloc(K * 2 * 2 * 8)]
    try:
        for b, a in zip(bufs, lifted + [pts]):
            ctx.dev_upload(b, a)
        ops = [glp.ExtOpenings(None, 0, 2 * c + PAD if o == NEXT_ORACLE else None, 2 * (2 * c + PAD), dev_ptr=bufs[o]) for o, c in enumerate(ORACLE_COLS)]
        assert g.eval_ext(bufs[3], ops, alphas[:K], params[:K], out_dev_ptr=bufs[4]) is None
        back = np.empty((K, 2, 2), np.uint64)
        ctx.dev_download(bufs[4], back)
        assert (back == want[:K]).all(), np.argwhere(back != want[:K])[:1]
    finally:
        ctx.synchronize()
        for b in bufs:
            ctx.dev_free(b)
    g.free()


# ------------------------------------------------------------------ 3. boundary values
def test_boundary_values(ctx):
    vals = [0, 1, P - 1]
    consts = [(a, b) for a in vals for b in vals]                  # the nine polynomials' openings, and the nine points
    asm = gp.Assembler([len(consts)])
    srcs = [asm.col(0, j) for j in range(len(consts))] + [asm.imm(v) for v in vals] + [asm.x]
    r = asm.reg()
    for op in (asm.add, asm.sub, asm.mul):
        for oa in srcs:
            for ob in srcs:
                op(r, oa, ob)
                asm.emit(r)
    asm.emit(asm.col(0, 8))
    asm.end(asm.col(0, 8))                                         # (p - 1, p - 1) as a filter
    asm.emit(asm.imm(P - 1))
    asm.emit(asm.x)
    asm.end(asm.x)
    prog = asm.assemble()
    assert prog.max_constraints == 3 * 13 * 13 + 1
    K = len(consts)
    points = np.array(consts, np.uint64)
    assert sum(1 for p in consts if p[1] == 0) == 3                # points of the base field among them
    ops = np.array([consts] * K, np.uint64)                        # [K][9][2]
    alphas = np.array([[P - 1, 1, 0, _rand(1, (1,))[0]]] * K, np.uint64)
    want = np.array([gx.run_ext(prog, [consts], None, consts[k], alphas[k]) for k in range(K)], np.uint64)
    g = ctx.gate_program(prog)
    got = g.eval_ext(points, [glp.ExtOpenings(ops)], alphas)
    assert (got == want).all(), np.argwhere(got != want)[:1]
    g.free()


# ------------------------------------------------------------------ 4. the whole check
def _tampered(desc, proof, seed):
    """(section, word, copy with 1 added mod p to that word): the first, the last and a random word of every opening section"""
    lay = zi.proof_layout(desc)
    rng = np.random.default_rng(seed)
    for name in SECTIONS:
        o, cnt = lay[name]
        for word in sorted({o, o + 2 * cnt - 1, o + int(rng.integers(0, 2 * cnt))}):
            bad = np.array(proof, np.uint64)
            bad[word] = (int(bad[word]) + 1) % P
            yield name, word, bad


def _whole_check(ctx, g, desc, proofs, challenges, reasons=True):
    """eval_ext into HBM, then perm_check_zeta on the same openings array with the gate sums from HBM"""
    K, nch = len(proofs), int(desc.num_challenges)
    ops = np.stack([_fri_order(desc, p) for p in proofs])
    parts = glp.plonk_ext_openings(desc, ops)
    betas, gammas, alphas = (np.array([c[i] for c in challenges], np.uint64) for i in range(3))
    zetas = np.array([c[3] for c in challenges], np.uint64)
    pihs = np.array([c[4] for c in challenges], np.uint64)
    dgs = ctx.dev_alloc(K * nch * 2 * 8)
    try:
        assert g.eval_ext(zetas, parts["program"], alphas, pihs, out_dev_ptr=dgs) is None
        return ctx.perm_check_zeta(desc, int(desc.quotient_degree_factor), zetas, parts["sigmas"], parts["wires"], parts["zs"], parts["zs_next"],
                                   parts["quotient"], betas, gammas, alphas, gate_sums_dev_ptr=dgs, reasons=reasons)
    finally:
        ctx.synchronize()
        ctx.dev_free(dgs)


@pytest.mark.parametrize("name", ["arith", "ext"])
def test_whole_check_on_a_proof_and_its_tampered_copies(ctx, proved, name):
    descs, prog, check, proofs, digests, g = proved(name)
    desc, proof, digest = descs[0], proofs[0], digests[0]
    qdf = int(desc.quotient_degree_factor)
    cases = [("", -1, proof)] + list(_tampered(desc, proof, 3))
    chal = zi.challenges(desc, proof, digest)                      # no opening enters the transcript before zeta
    status, reasons = _whole_check(ctx, g, desc, [c[2] for c in cases], [chal] * len(cases))
    assert status[0] == 0 and reasons[0] == "", reasons[0]
    caught = set()
    q0 = zi.proof_layout(desc)["q"][0]
    for k, (section, word, bad) in enumerate(cases[1:], 1):
        want = check(desc, bad, digest)
        restated = gx.check_proof(desc, prog, bad, digest)
        assert (restated == "") == want, (section, word)
        assert (status[k] == 0) == want and status[k] in (0, -5), (section, word, reasons[k])
        assert reasons[k] == restated, (section, word, reasons[k], restated)
        if not want:
            caught.add(section)
            assert reasons[k].startswith("Mismatch between evaluation and opening of quotient polynomial (challenge ")
            if section == "q":                                     # one challenge's chunk: that challenge is named
                assert reasons[k] == gx.MISMATCH % ((word - q0) // 2 // qdf)
    assert caught == set(SECTIONS), "no changed word was rejected in %s" % (set(SECTIONS) - caught,)


def test_three_proofs_one_damaged(ctx, proved):
    descs, prog, check, proofs, digests, g = proved("ext")
    assert all((d.constants == descs[0].constants).all() and (d.sigmas == descs[0].sigmas).all() for d in descs), "one circuit, three witnesses"
    chal = [zi.challenges(d, p, dig) for d, p, dig in zip(descs, proofs, digests)]
    assert len({c[3] for c in chal}) == 3
    status = _whole_check(ctx, g, descs[0], proofs, chal, reasons=False)
    assert list(status) == [0, 0, 0]
    o = zi.proof_layout(descs[0])["wires"][0]
    bad = proofs[1].copy()
    bad[o] = (int(bad[o]) + 1) % P
    assert not check(descs[1], bad, digests[1])
    status, reasons = _whole_check(ctx, g, descs[0], [proofs[0], bad, proofs[2]], chal)
    assert list(status) == [0, -5, 0] and reasons[0] == reasons[2] == "" and reasons[1] == gx.check_proof(descs[1], prog, bad, digests[1])


def test_zeta_one_is_a_verdict(ctx, proved):
    descs, prog, _check, proofs, digests, g = proved("arith")
    desc = descs[0]
    chal = [zi.challenges(desc, proofs[0], digests[0])] * 3
    chal[1] = chal[1][:3] + ((1, 0),) + chal[1][4:]
    status, reasons = _whole_check(ctx, g, desc, [proofs[0]] * 3, chal)
    assert list(status) == [0, -5, 0] and reasons == ["", "zeta = 1", ""]


def test_without_gate_sums_the_gate_term_is_absent(ctx, proved):
    """host gate sums are the HBM ones; with none, the restatement without the term decides"""
    descs, prog, _check, proofs, digests, g = proved("arith")
    desc, proof = descs[0], proofs[0]
    betas, gammas, alphas, zeta, pih = zi.challenges(desc, proof, digests[0])
    ops = _fri_order(desc, proof)
    parts = glp.plonk_ext_openings(desc, ops)
    sums = g.eval_ext(np.array(zeta, np.uint64), parts["program"], alphas, pih)
    args = (desc, int(desc.quotient_degree_factor), np.array(zeta, np.uint64), parts["sigmas"], parts["wires"], parts["zs"], parts["zs_next"], parts["quotient"],
            betas, gammas, alphas)
    assert list(ctx.perm_check_zeta(*args, gate_sums=sums)) == [0]
    op = gx.proof_openings(desc, proof)
    want = gx.perm_check(desc, args[1], zeta, op["sigmas"], op["wires"], op["zs"] + op["pp"], op["zs_next"], op["q"], betas, gammas, alphas)
    status, reasons = ctx.perm_check_zeta(*args, reasons=True)
    assert want != "" and list(status) == [-5] and reasons == [want]


def test_the_seam_end_to_end_without_a_circuit_on_the_verifying_side(ctx, oracle):
    """tests/test_gpu_gate_program.py::test_the_seam_end_to_end_with_a_gate_program up to the proof; then the verifier: fri_verify_many and
    the two calls of this file on one openings array.  glp.Circuit only supplies the digest the transcript starts from."""
    desc = cq.seam_circuit(oracle)
    rb, chh, nch, nc = int(desc.rate_bits), int(desc.cap_height), int(desc.num_challenges), int(desc.num_constants)
    sub_bits = int(desc.quotient_degree_factor).bit_length() - 1
    cap = 4 << chh
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    digest = gc.digest()
    gc.free()
    pih = oracle.hash_no_pad(np.asarray(desc.public_inputs, np.uint64))
    g = ctx.gate_program(gr.trace_circuit(desc)[0])
    cs = ctx.batch_from_values(np.concatenate([np.asarray(desc.constants, np.uint64), np.asarray(desc.sigmas, np.uint64)]), rb, chh)
    wb = ctx.batch_from_values(desc.wires, rb, chh)
    ch = oracle.Challenger(0)
    ch.observe_hashes(digest)
    ch.observe(pih)
    ch.observe_hashes(wb.cap())
    betas, gammas = ch.get_n(nch), ch.get_n(nch)
    zb = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, betas, gammas, rb, chh)
    ch.observe_hashes(zb.cap())
    alphas = ch.get_n(nch)
    words = nch << (int(desc.degree_bits) + sub_bits)
    dgs, dq = ctx.dev_alloc(words * 8), ctx.dev_alloc(words * 8)
    try:
        assert g.sums([cs, wb], sub_bits, alphas, pih, out_dev_ptr=dgs) is None
        assert ctx.perm_quotient_values(desc, cs, nc, wb, zb, sub_bits, betas, gammas, alphas, gate_sums_dev_ptr=dgs, out_dev_ptr=dq) is None
        qb = ctx.batch_from_coset_values(None, sub_bits, rb, chh, dev_ptr=dq, shape=(nch, words // nch))
    finally:
        ctx.synchronize()
        ctx.dev_free(dgs); ctx.dev_free(dq)
    ch.observe_hashes(qb.cap())
    zeta = ch.get_ext()
    inst = fr.plonk_instance(desc, zeta, False)
    batches = [cs, wb, zb, qb]
    fri_args = (desc.reduction_arity_bits, desc.proof_of_work_bits, desc.num_query_rounds)
    want_op = fr.plonk_openings_to_points(desc, proof[3 * cap:3 * cap + 2 * inst.num_openings])
    ch.observe(want_op)
    st, pend = fr.challenger_state(ch)
    op, tail = glp.fri_prove(ctx, batches, inst.points, *fri_args, st, pend)
    assert (np.asarray(op) == want_op).all() and (tail == proof[3 * cap + 2 * inst.num_openings:len(proof) - len(desc.public_inputs)]).all()

    # ---- the verifying side: caps, openings, the FriProof and the program; no glp_circuit
    openings = np.array(op, np.uint64).reshape(1, -1, 2)
    zs = np.array([[p for p, _ranges in inst.points]], np.uint64)
    status, reasons = glp.fri_verify_many(ctx, batches, inst.points, zs, *fri_args, openings, np.asarray(tail, np.uint64)[None], np.asarray(st, np.uint64)[None],
                                          np.asarray(pend, np.uint64).reshape(1, -1), caps=[b.cap() for b in batches])
    assert list(status) == [0], reasons

    def identity(openings):
        parts = glp.plonk_ext_openings(desc, openings)
        assert parts["count"] == openings.shape[1]
        zw = np.array([zeta], np.uint64)
        dsum = ctx.dev_alloc(nch * 2 * 8)
        try:
            assert g.eval_ext(zw, parts["program"], [alphas], [pih], out_dev_ptr=dsum) is None
            return ctx.perm_check_zeta(desc, int(desc.quotient_degree_factor), zw, parts["sigmas"], parts["wires"], parts["zs"], parts["zs_next"],
                                       parts["quotient"], [betas], [gammas], [alphas], gate_sums_dev_ptr=dsum, reasons=True)
        finally:
            ctx.synchronize()
            ctx.dev_free(dsum)
    status, reasons = identity(openings)
    assert list(status) == [0] and reasons == [""]
    flipped = openings.copy()
    w0 = int(desc.num_constants) + int(desc.num_routed_wires)      # the first wire
    flipped[0, w0, 0] = (int(flipped[0, w0, 0]) + 1) % P
    status, reasons = identity(flipped)
    assert list(status) == [-5] and reasons[0].startswith("Mismatch between evaluation and opening of quotient polynomial")
    g.free()
    for b in batches:
        b.free()


# ------------------------------------------------------------------ refusals
def _refused(fn, *needles):
    with pytest.raises(glp.GlpError) as e:
        fn()
    assert e.value.code == -1, str(e.value)                # GLP_ERR_ARG
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def _bad(v, i):
    v = np.array(v, np.uint64)
    v.reshape(-1)[i] = P + 3
    return v


def test_eval_ext_refusals(ctx):
    L = glp.load_library()
    prog, arrays, points, alphas, params, _want = _random_case()
    K = 2
    g = ctx.gate_program(prog)
    ctx2 = glp.Context(0)
    g2 = ctx2.gate_program(prog)
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.stage_reset()
    name = "glp_gate_program_eval_ext"
    ops = _random_openings(arrays)

    def ev(o=ops, pts=points[:K], a=alphas[:K], p=params[:K], prog_=g):
        view = glp.GateProgram(ctx, prog_._h, prog_.num_params, prog_.num_oracles)      # always under this test's ctx: another ctx's program is the library's to refuse
        try:
            return view.eval_ext(pts, o, a, p)
        finally:
            view._h = None                                         # the handle stays prog_'s

    def swap(i, **kw):
        o = list(ops)
        f = dict(array=o[i].array, at=o[i].at, at_next=o[i].at_next, proof_stride=o[i].proof_stride)
        f.update(kw)
        o[i] = glp.ExtOpenings(**f)
        return o
    _refused(lambda: ev(prog_=g2), name, "program", "ctx")
    _refused(lambda: ev(o=swap(1, proof_stride=2 * ORACLE_COLS[1] - 1)), name, "openings[1].proof_stride", "33", "17 polynomials")
    _refused(lambda: ev(o=swap(NEXT_ORACLE, at_next=None)), name, "openings[%d].at_next" % NEXT_ORACLE, "null")
    ev(o=swap(0, at_next=None))                                    # nothing reads the others' at_next: NULL is fine (served below as well)
    _refused(lambda: ev(a=_rand(1, (K, 5))), name, "num_challenges", "1..4")
    _refused(lambda: ev(a=_bad(alphas[:K], 3)), name, "alphas[1][1]", "canonical")
    _refused(lambda: ev(p=_bad(params[:K], 2)), name, "params[0][2]", "canonical")
    _refused(lambda: ev(p=None), name, "params", "null", "num_params = 3")
    _refused(lambda: ev(pts=_bad(points[:K], 3)), name, "points", "proof 1, word 1", "canonical")
    stride = 2 * (2 * ORACLE_COLS[2] + PAD)
    _refused(lambda: ev(o=swap(2, array=_bad(arrays[2], stride + 4))), name, "openings[2].at", "proof 1, word 4", "canonical")
    nx = 2 * ORACLE_COLS[1] + PAD
    _refused(lambda: ev(o=swap(1, array=_bad(arrays[1], nx + 5))), name, "openings[1].at_next", "proof 0, word 5", "canonical")
    ev(o=swap(1, array=_bad(arrays[1], 2 * ORACLE_COLS[1])))       # a spare word between the proofs is nobody's
    # raw calls: null pointers and the counts the binding derives
    cs = (binding._ExtOpenings * 3)(*[o._c() for o in ops])
    out = np.zeros((K, 2, 2), np.uint64)
    p_ = binding._p
    pts, al, prm = points[:K].copy(), alphas[:K].copy(), params[:K].copy()

    def raw(c=ctx._h, prog_=g._h, K_=K, nch=2, pts_=pts, o=cs, a=al, pr_=prm, out_=out):
        binding._chk(L.glp_gate_program_eval_ext(c, prog_, K_, nch, None if pts_ is None else p_(pts_), o, 0, None if a is None else p_(a),
                                                 None if pr_ is None else p_(pr_), None if out_ is None else p_(out_), 0))
    _refused(lambda: raw(c=None), name, "ctx", "null")
    _refused(lambda: raw(prog_=None), name, "program", "null")
    _refused(lambda: raw(prog_=g2._h), name, "program", "another ctx")
    _refused(lambda: raw(pts_=None), name, "points", "null")
    _refused(lambda: raw(o=None), name, "openings", "null")
    no_at = (binding._ExtOpenings * 3)(*[o._c() for o in ops])
    no_at[2].at = None
    _refused(lambda: raw(o=no_at), name, "openings[2].at", "null")
    _refused(lambda: raw(a=None), name, "alphas", "null")
    _refused(lambda: raw(out_=None), name, "out", "null")
    _refused(lambda: raw(K_=0), name, "num_proofs")
    _refused(lambda: raw(K_=4097), name, "num_proofs")
    _refused(lambda: raw(nch=0), name, "num_challenges")
    _refused(lambda: raw(nch=5), name, "num_challenges")
    served = [s[0] for s in ctx.stages()]
    assert served == ["gate_program.eval_ext"] * 2, "a refused call reached a launch: %s" % (served,)
    ctx.set_profiling(False)
    g2.free(); ctx2.close()
    g.free()


def test_perm_check_zeta_refusals(ctx, proved):
    L = glp.load_library()
    descs, prog, _check, proofs, digests, g = proved("arith")
    desc, proof = descs[0], proofs[0]
    nch, qdf, nr = int(desc.num_challenges), int(desc.quotient_degree_factor), int(desc.num_routed_wires)
    betas, gammas, alphas, zeta, pih = zi.challenges(desc, proof, digests[0])
    ops = np.stack([_fri_order(desc, proof)] * 2)
    parts = glp.plonk_ext_openings(desc, ops)
    count = parts["count"]
    K = 2
    two = lambda v: np.array([v, v], np.uint64)
    sums = g.eval_ext(two(zeta), parts["program"], two(alphas), two(pih))
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.stage_reset()
    name = "glp_perm_check_zeta"
    base = dict(desc=desc, chunks=qdf, zetas=two(zeta), sigmas=parts["sigmas"], wires=parts["wires"], zs=parts["zs"], zs_next=parts["zs_next"],
                quotient=parts["quotient"], betas=two(betas), gammas=two(gammas), alphas=two(alphas), gate_sums=sums)

    def check(**kw):
        a = dict(base, **kw)
        return ctx.perm_check_zeta(a["desc"], a["chunks"], a["zetas"], a["sigmas"], a["wires"], a["zs"], a["zs_next"], a["quotient"], a["betas"],
                                   a["gammas"], a["alphas"], gate_sums=a["gate_sums"])

    def moved(part, **kw):
        f = dict(array=part.array, at=part.at, at_next=part.at_next, proof_stride=part.proof_stride)
        f.update(kw)
        return glp.ExtOpenings(**f)
    _refused(lambda: check(chunks=0), name, "num_quotient_chunks", "1..256")
    _refused(lambda: check(chunks=257), name, "num_quotient_chunks", "1..256")
    _refused(lambda: check(sigmas=moved(parts["sigmas"], proof_stride=2 * nr - 2)), name, "sigmas.proof_stride")
    _refused(lambda: check(wires=moved(parts["wires"], proof_stride=2 * nr - 2)), name, "wires.proof_stride")
    nzp = glp.perm_num_polys(desc)
    _refused(lambda: check(zs=moved(parts["zs"], proof_stride=2 * nzp - 2), zs_next=moved(parts["zs_next"], proof_stride=2 * nzp - 2)), name, "zs.proof_stride")
    _refused(lambda: check(quotient=moved(parts["quotient"], proof_stride=2 * nch * qdf - 2)), name, "quotient.proof_stride")
    _refused(lambda: check(zs_next=None), name, "zs.at_next", "null")
    _refused(lambda: check(betas=_bad(two(betas), 1)), name, "betas[0][1]", "canonical")
    _refused(lambda: check(gammas=_bad(two(gammas), 2)), name, "gammas[1][0]", "canonical")
    _refused(lambda: check(alphas=_bad(two(alphas), 3)), name, "alphas[1][1]", "canonical")
    _refused(lambda: check(zetas=_bad(two(zeta), 2)), name, "zetas", "proof 1, word 0", "canonical")
    _refused(lambda: check(gate_sums=_bad(sums, 2 * nch + 1)), name, "gate_sums", "proof 1, word 1", "canonical")
    stride = 2 * count
    for part, polys in (("sigmas", nr), ("wires", nr), ("zs", nzp), ("quotient", nch * qdf)):
        at = parts[part].at + stride + 2 * polys - 1               # proof 1, the last word read
        _refused(lambda: check(**{part: moved(parts[part], array=_bad(ops, at)), "zs_next": moved(parts["zs_next"], array=_bad(ops, at))}
                               if part == "zs" else {part: moved(parts[part], array=_bad(ops, at))}),
                 name, part + ".at", "proof 1, word %d" % (2 * polys - 1), "canonical")
    at = parts["zs_next"].at + 2 * nch - 1
    _refused(lambda: check(zs=moved(parts["zs"], array=_bad(ops, at)), zs_next=moved(parts["zs_next"], array=_bad(ops, at))), name, "zs.at_next",
             "proof 0, word %d" % (2 * nch - 1), "canonical")

    class Shape:                                                   # a description glp_perm_num_polys refuses
        degree_bits, num_wires, num_routed_wires, num_challenges, quotient_degree_factor, k_is = 60, desc.num_wires, nr, nch, qdf, desc.k_is
    _refused(lambda: check(desc=Shape), name, "desc.log_n")
    # raw calls: null pointers and the proof count
    d, keep = glp.perm_desc(desc)
    cs = {k: parts[k]._c() for k in ("sigmas", "wires", "zs", "quotient")}
    cs["zs"].at_next = parts["zs_next"]._c().at
    status = np.zeros(K, np.int32)
    p_ = binding._p
    arr = dict(zetas=two(zeta), betas=two(betas), gammas=two(gammas), alphas=two(alphas))

    def raw(c=ctx._h, d_=d, K_=K, st=status, **kw):
        a = dict(arr, **kw)
        o = {k: a.get(k, cs[k]) for k in cs}
        ptr = lambda v: None if v is None else p_(v)
        ref = lambda v: None if v is None else C.byref(v)
        binding._chk(L.glp_perm_check_zeta(c, None if d_ is None else C.byref(d_), K_, qdf, ptr(a["zetas"]), ref(o["sigmas"]), ref(o["wires"]), ref(o["zs"]),
                                           ref(o["quotient"]), 0, ptr(a["betas"]), ptr(a["gammas"]), ptr(a["alphas"]), None, 0,
                                           None if st is None else st.ctypes.data_as(C.c_void_p), None))
    _refused(lambda: raw(c=None), name, "ctx", "null")
    _refused(lambda: raw(d_=None), name, "desc", "null")
    for k in ("zetas", "sigmas", "wires", "zs", "quotient", "betas", "gammas", "alphas"):
        _refused(lambda: raw(**{k: None}), name, k, "null")
    no_at = binding._ExtOpenings(None, None, stride)
    _refused(lambda: raw(wires=no_at), name, "wires.at", "null")
    _refused(lambda: raw(st=None), name, "status_out", "null")
    _refused(lambda: raw(K_=0), name, "num_proofs")
    _refused(lambda: raw(K_=4097), name, "num_proofs")
    assert ctx.stages() == [], "a refused call reached a launch: %s" % (ctx.stages(),)
    assert list(check()) == [0, 0]                                 # and the unrefused call is served, under its stage name
    assert [s[0] for s in ctx.stages()] == ["perm.check_zeta"]
    ctx.set_profiling(False)
    del keep
