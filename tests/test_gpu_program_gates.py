"""GLP_GATE_PROGRAM on the GPU (include/glp.h, "GATE PROGRAMS IN A CIRCUIT"): k_quotient_gate_program, k_witness_check_program, the
verifier's host interpreter and glp_circuit_create_prog, judged by the twin circuit of tests/program_gates.py.  D' gives chosen gates
of a description D type 23 with programs traced from the restated bodies; constants, sigmas and every constraint value are the same
field elements, so digest, caps and every proof word must equal the CPU oracle's proof of D (where the oracle has the gates; the
extension and recursion gates are pinned by tests/zeta_identity_recursion.py instead) and the library's own.  Fixed seeds."""
import functools
import os

import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
from plonky2_lib_amd import gate_program as gp
import program_gates as pg
import zeta_identity_recursion as zr

pytestmark = pytest.mark.gpu

P = pg.P
REC = synth.Config.standard_recursion_config
SEED = [0x1111, 0x2222, 0x3333, 0x4444]


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _last_error():
    return glp.load_library().glp_last_error().decode()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert (got == want).all(), "%s: first mismatch at word %d" % (what, int(np.argmax(got.reshape(-1) != want.reshape(-1))))


CASES = {
    "zkdsa3": lambda: synth.zkdsa_circuit(3),                                  # 8 live lanes, PoseidonGate's 123 constraints
    "arith5": lambda: synth.arith_circuit(5, seed=31),
    "arith10": lambda: synth.arith_circuit(10, seed=32),                      # more than one 256-lane block
    "ext": lambda: synth.ext_gates_circuit(4, REC(), seed=33),
    "rec": lambda: synth.recursion_gates_circuit(4, REC(), seed=34),
    "mixed": lambda: synth.recursion_gates_circuit(4, REC(), seed=35, mix_ext=True),      # only ONE gate of a shared group becomes a program
    "zkdsa3_nch1": lambda: synth.zkdsa_circuit(3, config=REC(num_challenges=1)),
    "zkdsa3_nch3": lambda: synth.zkdsa_circuit(3, config=REC(num_challenges=3)),
    "zkdsa3_nch4": lambda: synth.zkdsa_circuit(3, config=REC(num_challenges=4)),
    "arith5_nch1": lambda: synth.arith_circuit(5, synth.Config.standard_ecc_config(num_challenges=1), seed=36),
    "arith5_nch3": lambda: synth.arith_circuit(5, synth.Config.standard_ecc_config(num_challenges=3), seed=37),
    "arith5_nch4": lambda: synth.arith_circuit(5, synth.Config.standard_ecc_config(num_challenges=4), seed=38),
    "arith5_step2": lambda: synth.arith_circuit(5, synth.Config.standard_ecc_config(max_quotient_degree_factor=4), seed=39),   # qdf 4 < 2^rate_bits
    "arith5_step2_nch3": lambda: synth.arith_circuit(5, synth.Config.standard_ecc_config(max_quotient_degree_factor=4, num_challenges=3), seed=40),
}
NO_ORACLE = ("ext", "rec", "mixed")              # gates the CPU oracle does not evaluate


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (D, D', programs), made once per case and never written to"""
    desc = CASES[name]()
    which = [pg.mixed_group(desc)] if name == "mixed" else None
    d2, progs = pg.twin(desc, which)
    if name == "mixed":
        g = d2.gates[which[0]]
        assert sum(int(h["selector_index"]) == int(g["selector_index"]) and int(h["type"]) != pg.GATE_PROGRAM and int(h["num_constraints"]) > 0
                   for h in d2.gates) >= 1
    return desc, d2, progs


@functools.lru_cache(maxsize=None)
def _oracle_proof(oracle, name):
    oc = oracle.OracleCircuit(_case(name)[0])
    rc, ref = oc.prove()
    assert rc == 0 and oc.verify(ref) == 0
    return oc, ref


def _pair(ctx, name):
    desc, d2, progs = _case(name)
    return glp.Circuit(ctx, desc), glp.Circuit(ctx, d2, programs=progs)


# ---------------------------------------------------------------------------------------------------- 1, 2. one proof
@pytest.mark.parametrize("name", list(CASES))
def test_twin_proof_is_the_oracles(ctx, oracle, name):
    desc, d2, progs = _case(name)
    gc, gt = _pair(ctx, name)
    _same(gt.digest(), gc.digest(), "digest")
    _same(gt.constants_sigmas_cap(), gc.constants_sigmas_cap(), "constants_sigmas cap")
    assert gt.proof_words == gc.proof_words
    got = gt.prove()
    _same(got, gc.prove(), "prove(D') against prove(D)")
    assert gt.verify(got), _last_error()
    assert gc.verify(got), _last_error()
    assert gt.verify_batch(got[None, :]).all()
    if name in NO_ORACLE:
        assert zr.check(desc, got, gc.digest())
    else:
        oc, ref = _oracle_proof(oracle, name)
        _same(got, ref, "prove(D') against the oracle's proof of D")
        assert oc.verify(got) == 0
    assert gt.check_witness(by_gate=True).as_tuple() == gc.check_witness(by_gate=True).as_tuple()
    assert gt.check_witness().ok
    gc.free(); gt.free()


# ---------------------------------------------------------------------------------------------------- 3. the other drivers
@pytest.mark.parametrize("name,K", [("zkdsa3", 3), ("zkdsa3", 256), ("arith5", 3)])
@pytest.mark.parametrize("host_transcript", [False, True])
def test_twin_prove_batch(ctx, name, K, host_transcript):
    desc, d2, progs = _case(name)
    gc, gt = _pair(ctx, name)
    rng = np.random.default_rng(K)
    wires = np.stack([np.asarray(desc.wires, np.uint64)] * K)
    bad = sorted(set(int(k) for k in rng.integers(0, K, 2)))      # members whose witness breaks a program gate: same invalid transcript
    gi = next(i for i, g in enumerate(d2.gates) if int(g["type"]) == pg.GATE_PROGRAM and len(zr.gate_rows(d2, i)))
    row, col = int(zr.gate_rows(d2, gi)[0]), glp.gate_program_circuit_check(progs[int(d2.gates[gi]["p0"])])[2] - 1
    for k in bad:
        wires[k, col, row] = (int(wires[k, col, row]) + 1 + k) % P
    pis = np.stack([np.asarray(desc.public_inputs, np.uint64)] * K)
    if host_transcript:
        os.environ["GLP_BATCH_HOST_TRANSCRIPT"] = "1"
    try:
        want, got = gc.prove_batch(wires, pis), gt.prove_batch(wires, pis)
    finally:
        os.environ.pop("GLP_BATCH_HOST_TRANSCRIPT", None)
    _same(got, want, "prove_batch(D') against prove_batch(D)")
    _same(got[0 if 0 not in bad else 1], gc.prove(wires=wires[0 if 0 not in bad else 1]), "a member against glp_prove")
    ok_t, why_t = gt.verify_batch(got, reasons=True)
    ok_c, why_c = gc.verify_batch(got, reasons=True)
    assert (ok_t == ok_c).all() and why_t == why_c
    assert [k for k in range(K) if not ok_t[k]] == bad
    gc.free(); gt.free()


def test_twin_stepped_session(ctx, oracle):
    from test_gpu_prove import _stepped_proof
    for name in ("zkdsa3", "arith5_nch3"):
        desc, d2, progs = _case(name)
        gt = glp.Circuit(ctx, d2, programs=progs)
        d2s = d2.__class__()
        d2s.__dict__.update(d2.__dict__)
        d2s.circuit_digest = gt.digest()
        _same(_stepped_proof(gt, oracle, d2s), _oracle_proof(oracle, name)[1], "stepped session of D' against the oracle's proof of D")
        gt.free()


def test_twin_keccak_hasher(ctx, oracle):
    for make in (lambda: synth.zkdsa_circuit(3), lambda: synth.arith_circuit(5, seed=41)):
        desc = make()
        desc.hasher = 1                              # GLP_HASH_KECCAK25
        d2, progs = pg.twin(desc)
        gc, gt = glp.Circuit(ctx, desc), glp.Circuit(ctx, d2, programs=progs)
        _same(gt.digest(), gc.digest(), "digest")
        got = gt.prove()
        _same(got, gc.prove(), "prove(D') against prove(D), KeccakHash<25>")
        oc = oracle.OracleCircuit(desc)
        rc, ref = oc.prove()
        assert rc == 0
        _same(got, ref, "prove(D') against the oracle's proof of D, KeccakHash<25>")
        assert gt.verify(got) and gt.verify_batch(got[None, :]).all()
        K = 3
        wires = np.stack([np.asarray(desc.wires, np.uint64)] * K)
        pis = np.stack([np.asarray(desc.public_inputs, np.uint64)] * K)
        _same(gt.prove_batch(wires, pis), gc.prove_batch(wires, pis), "prove_batch, KeccakHash<25>")
        gc.free(); gt.free()


def test_twin_zero_knowledge(ctx):
    desc = synth.zkdsa_circuit(config=synth.Config.standard_recursion_zk_config(num_query_rounds=4), blinding_seed=7)
    assert desc.zero_knowledge
    d2, progs = pg.twin(desc)
    gc, gt = glp.Circuit(ctx, desc), glp.Circuit(ctx, d2, programs=progs)
    assert gt.zero_knowledge and gt.proof_words == gc.proof_words
    try:
        ctx.set_salt_seed(SEED)
        want = gc.prove()
        ctx.set_salt_seed(SEED)
        got = gt.prove()
        _same(got, want, "zero-knowledge prove(D') against prove(D) under one salt seed")
        assert gt.verify(got) and gc.verify(got) and gt.verify_batch(got[None, :]).all()
        K = 3
        wires = np.stack([np.asarray(desc.wires, np.uint64)] * K)
        pis = np.stack([np.asarray(desc.public_inputs, np.uint64)] * K)
        ctx.set_salt_seed(SEED)
        wb = gc.prove_batch(wires, pis)
        ctx.set_salt_seed(SEED)
        _same(gt.prove_batch(wires, pis), wb, "zero-knowledge prove_batch")
    finally:
        ctx.set_salt_seed(None)
    gc.free(); gt.free()


# ---------------------------------------------------------------------------------------------------- 4. a broken witness
@pytest.mark.parametrize("name", ["zkdsa3", "arith5", "arith5_nch3", "mixed"])
def test_one_changed_cell_on_a_program_row(ctx, name):
    desc, d2, progs = _case(name)
    gc, gt = _pair(ctx, name)
    for gi, g in enumerate(d2.gates):
        if int(g["type"]) != pg.GATE_PROGRAM or not len(zr.gate_rows(d2, gi)):
            continue
        used = glp.gate_program_circuit_check(progs[int(g["p0"])])[2]
        row, col = int(zr.gate_rows(d2, gi)[-1]), used - 1
        w = np.asarray(desc.wires, np.uint64).copy()
        w[col, row] = (int(w[col, row]) + 1) % P
        assert any(zr.row_constraints(desc, gi, row, wires=w)), (gi, row, col)
        got = gt.prove(wires=w)
        _same(got, gc.prove(wires=w), "the same invalid transcript, gate %d" % gi)
        assert not gt.verify(got) and not gc.verify(got)
        assert not gt.verify_batch(got[None, :]).any()
        rt, rc = gt.check_witness(wires=w, by_gate=True), gc.check_witness(wires=w, by_gate=True)
        assert rt.as_tuple() == rc.as_tuple() and rt.rows_failed_by_gate == rc.rows_failed_by_gate
        assert rt.failed_constraints and rt.gate_type == pg.GATE_PROGRAM and "type 23" in str(rt)
    gc.free(); gt.free()


# ---------------------------------------------------------------------------------------------------- 6. operand extremes
def test_operand_extremes(ctx):
    """every wire and every gate constant of every row is one of 0, 1, p - 1, 2^32 - 1, neighbouring columns meeting in every pair: the
    witness satisfies nothing, which the twin must prove and report exactly as the built-in bodies do"""
    desc, _, _ = _case("arith5")
    d = desc.__class__()
    d.__dict__.update(desc.__dict__)
    n, nsel = 1 << int(desc.degree_bits), int(desc.num_selectors)
    d.constants = np.asarray(desc.constants, np.uint64).copy()
    d.constants[nsel:] = pg.extreme_columns(n, int(desc.num_constants) - nsel, phase=1)
    d.wires = pg.extreme_columns(n, int(desc.num_wires))
    d.circuit_digest = None
    d2, progs = pg.twin(d)
    gc, gt = glp.Circuit(ctx, d), glp.Circuit(ctx, d2, programs=progs)
    _same(gt.digest(), gc.digest(), "digest")
    _same(gt.prove(), gc.prove(), "prove(D') against prove(D) at the operand extremes")
    rt, rc = gt.check_witness(by_gate=True), gc.check_witness(by_gate=True)
    assert rt.as_tuple() == rc.as_tuple() and rt.rows_failed_by_gate == rc.rows_failed_by_gate and rt.failed_constraints
    gc.free(); gt.free()


# ---------------------------------------------------------------------------------------------------- 5. a gate the library has no body for
GATE_K = 0x123456789ABCDEF


def _square_gate_circuit(lg=5):
    """rows of a gate d - k (a b + c)^2 (wires 0..3, gate constant 0), d of each row copied into a of the next; the last rows NoopGate.
    Built as ArithmeticGate rows of one operation, whose selector and copy data the program gate takes over."""
    cfg = synth.Config(16, 8, proof_of_work_bits=4, num_query_rounds=4)
    b = synth.Builder(cfg, lg, seed=51)
    n = b.n
    rows = np.arange(0, n - 3)
    b.set_rows(rows, synth.GATE_ARITHMETIC, 1)
    b.gate_consts[0, rows] = GATE_K
    b.connect_pairs(rows[:-1], 3, rows[1:], 0)
    desc = b.build()
    gi = next(i for i, g in enumerate(desc.gates) if int(g["type"]) == synth.GATE_ARITHMETIC)
    desc.gates[gi].update(type=pg.GATE_PROGRAM, p0=0, p1=0, num_constraints=1)
    asm, F, cs, lw, _ = pg.assembler(desc)
    t = F.add(F.mul(lw[0], lw[1]), lw[2])
    prog = pg.close(asm, F, [F.sub(lw[3], F.mul(F.mul(t, t), cs[int(desc.num_selectors)]))])
    return desc, prog, rows, gi


def _square_witness(desc, rows, off_by_one=None):
    w = np.asarray(desc.wires, np.uint64).copy()
    a = int(w[0, rows[0]])
    for r in rows:
        bb, c = int(w[1, r]), int(w[2, r])
        if off_by_one == r:
            bb = (bb + 1) % P
        w[0, r] = a
        a = GATE_K * pow((a * bb + c) % P, 2, P) % P
        w[3, r] = a
    return w


def test_a_gate_without_a_builtin_body(ctx, oracle):
    import coset_quotient as cq  # noqa: F401  (the seam's helpers live beside it)
    import fri_restate as fr
    from plonky2_lib_amd import witness_program as wprog
    desc, prog, rows, gi = _square_gate_circuit()
    assert glp.gate_program_circuit_check(prog) == (1, 5, 4, int(desc.num_selectors) + 1)
    n, nw = 1 << int(desc.degree_bits), int(desc.num_wires)
    honest = _square_witness(desc, rows)
    gt = glp.Circuit(ctx, desc, programs=[prog])
    assert gt.witness_units(gi).shape[0] == 0                         # no built-in generator: its rows are the caller's
    # the witness from a unit program per row: a, b, c -> d = k (a b + c)^2; a of the next row arrives through the copy
    asm = wprog.Assembler(3)
    t = asm.add(asm.reg(), asm.mul(asm.reg(), asm.input(0), asm.input(1)), asm.input(2))
    asm.emit(asm.mul(asm.reg(), asm.mul(asm.reg(), t, t), asm.imm(GATE_K)))
    cell = lambda col, row: col * n + int(row)
    units = np.array([[glp.WGEN_PROGRAM, 0, 4 * i, 3, 1, 0, 0, 0, 0] for i in range(len(rows))], np.int64)
    cells = np.array([c for r in rows for c in (cell(0, r), cell(1, r), cell(2, r), cell(3, r))], np.uint64)
    inputs = [cell(0, rows[0])] + [cell(1, r) for r in rows] + [cell(2, r) for r in rows]
    plan = gt.witness_plan(inputs, free_units=(units, cells), programs=[asm.assemble()])
    start = honest.copy()
    start[0, rows[1:]] = 0
    start[3, rows] = 0
    ptr = ctx.dev_alloc(start.nbytes)
    try:
        ctx.dev_upload(ptr, start)
        plan.generate(ptr, np.array([[int(honest.reshape(-1)[c]) for c in inputs]], np.uint64), 1)
        got_w = np.empty_like(start)
        ctx.dev_download(ptr, got_w)
        _same(got_w, honest, "the generated witness")
        assert gt.check_witness(dev_wires_ptr=ptr).ok
        proof = gt.prove_device(ptr)
    finally:
        ctx.dev_free(ptr)
        plan.free()
    assert gt.verify(proof), _last_error()
    assert gt.verify_batch(proof[None, :]).all()
    # the seam path for the same circuit: the gate with its filter as a seam program, the library's permutation quotient around it
    rb, chh, nch, nc = int(desc.rate_bits), int(desc.cap_height), int(desc.num_challenges), int(desc.num_constants)
    sub_bits = int(desc.quotient_degree_factor).bit_length() - 1
    cap = 4 << chh
    sasm = gp.Assembler([nc, nw], num_params=4)
    SF = gp.TraceField(sasm)
    scs, slw = [sasm.col(0, j) for j in range(nc)], [sasm.col(1, j) for j in range(nw)]
    g = desc.gates[gi]
    filt = SF.one
    for v in range(int(g["group_start"]), int(g["group_end"])):
        if v != int(g["row"]):
            filt = SF.mul(filt, SF.sub(SF.lift(v), scs[int(g["selector_index"])]))
    if int(desc.num_selectors) > 1:
        filt = SF.mul(filt, SF.sub(SF.lift(0xFFFFFFFF), scs[int(g["selector_index"])]))
    st = SF.add(SF.mul(slw[0], slw[1]), slw[2])
    sasm.emit(SF.sub(slw[3], SF.mul(SF.mul(st, st), scs[int(desc.num_selectors)])))
    sasm.end(filt)
    seam = ctx.gate_program(sasm.assemble(hoist_emits=True))
    cs = ctx.batch_from_values(np.concatenate([np.asarray(desc.constants, np.uint64), np.asarray(desc.sigmas, np.uint64)]), rb, chh)
    wb = ctx.batch_from_values(honest, rb, chh)
    _same(wb.cap().reshape(-1), proof[:cap], "wires cap")
    pih = oracle.hash_no_pad(np.asarray(desc.public_inputs, np.uint64))
    ch = oracle.Challenger(0)
    ch.observe_hashes(gt.digest()); ch.observe(pih); ch.observe_hashes(wb.cap())
    betas, gammas = ch.get_n(nch), ch.get_n(nch)
    zb = ctx.perm_zs_commit(desc, honest, desc.sigmas, betas, gammas, rb, chh)
    _same(zb.cap().reshape(-1), proof[cap:2 * cap], "zs / partial products cap")
    ch.observe_hashes(zb.cap())
    alphas = ch.get_n(nch)
    words = nch << (int(desc.degree_bits) + sub_bits)
    dgs, dq = ctx.dev_alloc(words * 8), ctx.dev_alloc(words * 8)
    try:
        seam.sums([cs, wb], sub_bits, alphas, pih, out_dev_ptr=dgs)
        ctx.perm_quotient_values(desc, cs, nc, wb, zb, sub_bits, betas, gammas, alphas, gate_sums_dev_ptr=dgs, out_dev_ptr=dq)
        qb = ctx.batch_from_coset_values(None, sub_bits, rb, chh, dev_ptr=dq, shape=(nch, words // nch))
    finally:
        ctx.synchronize()
        ctx.dev_free(dgs); ctx.dev_free(dq)
    _same(qb.cap().reshape(-1), proof[2 * cap:3 * cap], "the quotient cap against the seam's")
    ch.observe_hashes(qb.cap())
    inst = fr.plonk_instance(desc, ch.get_ext(), False)
    want_op = fr.plonk_openings_to_points(desc, proof[3 * cap:3 * cap + 2 * inst.num_openings])
    ch.observe(want_op)
    state, pend = fr.challenger_state(ch)
    op, _tail = glp.fri_prove(ctx, [cs, wb, zb, qb], inst.points, desc.reduction_arity_bits, desc.proof_of_work_bits, desc.num_query_rounds, state, pend)
    _same(op, want_op, "the openings against the seam's")
    seam.free()
    for bt in (cs, wb, zb, qb):
        bt.free()
    # one multiplicand off by one: the verdict flips
    bad = _square_witness(desc, rows, off_by_one=int(rows[len(rows) // 2]))
    bad[1] = honest[1]                                                # b itself is as the honest witness has it; d and what follows are not
    rep = gt.check_witness(wires=bad)
    assert rep.failed_constraints and rep.gate == gi and rep.row == int(rows[len(rows) // 2]) and rep.constraint == 0
    bp = gt.prove(wires=bad)
    assert not gt.verify(bp) and not gt.verify_batch(bp[None, :]).any()
    gt.free()


# ---------------------------------------------------------------------------------------------------- 7. refusals
def _refused(ctx, desc, programs, *needles, code=-1):
    ctx.stage_reset()
    ctx.set_profiling(True)
    try:
        with pytest.raises(glp.GlpError) as e:
            glp.Circuit(ctx, desc, programs=programs)
    finally:
        ctx.set_profiling(False)
    assert e.value.code == code, str(e.value)
    for needle in needles:
        assert needle in str(e.value), str(e.value)
    assert ctx.stages() == []


def test_refusals(ctx):
    L = glp.load_library()
    desc, prog, rows, gi = _square_gate_circuit()
    nc, nw, nsel = int(desc.num_constants), int(desc.num_wires), int(desc.num_selectors)

    def fresh(**gate_fields):
        d = desc.__class__()
        d.__dict__.update(desc.__dict__)
        d.gates = [dict(g) for g in desc.gates]
        d.gates[gi].update(gate_fields)
        return d

    def program(build, oracle_cols=None, num_params=4):
        asm = gp.Assembler(oracle_cols or [nc, nw], num_params=num_params)
        build(asm, gp.TraceField(asm))
        return asm.assemble()
    gate = "gate %d" % gi
    # type 23 without a program list: a type this call does not know (and *out stays null)
    _refused(ctx, desc, None, gate, "is not supported", code=-3)
    _refused(ctx, desc, [], gate, "is not supported", code=-3)
    d, keep = glp.binding._desc_to_c(desc)
    import ctypes as C
    h = C.c_void_p(0x5A5A)
    assert L.glp_circuit_create_ex(ctx._h, C.byref(d), 0, C.byref(h)) == -3 and h.value is None
    pd, keep2 = glp.gate_program_desc(prog)
    h = C.c_void_p(0x5A5A)
    bad = fresh(p0=1)
    d1, keep1 = glp.binding._desc_to_c(bad)
    assert L.glp_circuit_create_prog(ctx._h, C.byref(d1), 0, C.byref(pd), 1, C.byref(h)) == -1 and h.value is None
    _refused(ctx, fresh(p0=1), [prog], gate, "p0")
    _refused(ctx, fresh(p1=1), [prog], gate, "p1")
    _refused(ctx, fresh(num_constraints=2), [prog], gate, "num_constraints")
    two = program(lambda a, F: (a.emit(a.col(1, 0)), a.emit(a.col(1, 1)), a.end(a.imm(1))))
    _refused(ctx, desc, [two], gate, "num_constraints")
    _refused(ctx, desc, [program(lambda a, F: (a.emit(F.sub(a.col_next(1, 0), a.col(1, 1))), a.end(a.imm(1))))], "programs[0]", "instruction 0", "COL_NEXT")
    _refused(ctx, desc, [program(lambda a, F: (a.emit(F.sub(a.col(1, 0), a.x)), a.end(a.imm(1))))], "programs[0]", "instruction 0", "X")
    _refused(ctx, desc, [program(lambda a, F: (a.emit(a.col(1, 0)), a.end(a.imm(1)), a.end(a.imm(1))))], "programs[0]", "instruction 1", "END")
    _refused(ctx, desc, [program(lambda a, F: (a.emit(a.col(1, 0)), a.end(a.imm(7))))], "programs[0]", "instruction 1", "END")
    _refused(ctx, desc, [program(lambda a, F: (a.emit(a.col(1, 0)), a.end(a.col(1, 0))))], "programs[0]", "instruction 1", "END")
    # a column beyond the circuit's (the program's own oracle_cols allow it)
    _refused(ctx, desc, [program(lambda a, F: (a.emit(a.col(1, nw)), a.end(a.imm(1))), [nc, nw + 1])], gate, "num_wires")
    _refused(ctx, desc, [program(lambda a, F: (a.emit(a.col(0, nc)), a.end(a.imm(1))), [nc + 1, nw])], gate, "num_constants")
    # the degree rule: degree + filter degree <= quotient_degree_factor + 1, one below it accepted
    g = desc.gates[gi]
    filt = int(g["group_end"]) - int(g["group_start"]) - 1 + (1 if nsel > 1 else 0)
    top = int(desc.quotient_degree_factor) + 1 - filt

    def power(e):
        def build(a, F):
            x = a.col(1, 0)
            for _ in range(e - 1):
                x = F.mul(x, a.col(1, 1))
            a.emit(x)
            a.end(a.imm(1))
        return build
    _refused(ctx, desc, [program(power(top + 1))], gate, "degree %d" % (top + 1), "exceeds")
    glp.Circuit(ctx, desc, programs=[program(power(top))]).free()
    # the constraint bound, both sides (the circuit declares as many gate constraints as the program emits)
    bound = glp.GATE_PROGRAM_MAX_CONSTRAINTS

    def many(a, F):
        for _ in range(bound):
            a.emit(a.col(1, 0))
        a.end(a.imm(1))
    full = program(many)
    wide = fresh(num_constraints=bound)
    wide.num_gate_constraints = bound
    glp.Circuit(ctx, wide, programs=[full]).free()
    full.code = np.concatenate([full.code[:1], full.code])
    wide = fresh(num_constraints=bound + 1)
    wide.num_gate_constraints = bound + 1
    _refused(ctx, wide, [full], "programs[0]", "instruction %d" % bound, "EMIT")
    glp.Circuit(ctx, desc, programs=[prog]).free()               # the unmodified description is accepted
