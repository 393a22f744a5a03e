"""Gate programs on the GPU (include/glp.h: glp_gate_program_create, glp_gate_program_sums).  Fixed seeds, every word compared.
1. programs traced from zeta_identity.gate_constraints against perm_restate.gate_sums over rows from Batch.lde_values: the seam circuit
   and the extension-gate circuit at sub_bits 3, 1, 0, then one, three and four challenges.  M is 16..128: every launch has dead lanes.
2. random programs against the restated interpreter (tests/gate_program_restate.py): 24 registers all live, every operand kind on
   both sides, COL_NEXT (it wraps at the last slot), X, gates of 1, 0 and 1 500 EMITs, several thousand instructions, results that
   overwrite one of their own operands; one block with dead lanes, and several blocks.
3. boundary values: the constant polynomials 0, 1, p - 1 against the pool words 0, 1, p - 1 in every ADD / SUB / MUL pairing.
4. three proofs in one call (shared and per-proof oracles, salted), device output, the seam end to end, every refusal by name.
The CPU side (the restatement pinned against perm_restate.gate_sums) is tests/test_gate_program.py."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
from plonky2_lib_amd import gate_program as gp
import plonky2_lib_amd.gl_numpy as gl
import plonky2_lib_amd.synth as synth
import coset_quotient as cq
import fri_restate as fr
import gate_program_restate as gr
import perm_restate as pr

pytestmark = pytest.mark.gpu

ROW = glp.LDE_ROW_MAJOR
P = cq.P
SEED = [11, 12, 13, 14]
ORACLE_COLS = (5, 17, 3)
NUM_PARAMS = 3


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _rand(seed, shape):
    return gl.rand(np.random.default_rng(seed), shape)


def _rows(b, sub_bits, ncols=None):
    return b.lde_values(0, b.ncols if ncols is None else ncols, sub_bits, layout=ROW)


def _first_diff(got, want):
    return "first mismatch at %s" % (tuple(np.argwhere(got != want)[0]) if (got != want).any() else None,)


# ------------------------------------------------------------------ 1. traced gate programs against perm_restate.gate_sums
@functools.lru_cache(maxsize=None)
def _circuit(name):
    from oracle import oracle
    oracle.build()
    if name == "seam":
        desc = cq.seam_circuit(oracle)
        pih = oracle.hash_no_pad(np.asarray(desc.public_inputs, np.uint64))
    else:
        desc, pih = synth.ext_gates_circuit(4), np.zeros(4, np.uint64)
    prog, _counts = gr.trace_circuit(desc)
    return desc, pih, prog


def _with_challenges(desc, nch):
    """what perm_restate.gate_sums reads of a description, with another number of challenges"""
    return SimpleNamespace(num_challenges=nch, num_selectors=desc.num_selectors, num_gate_constraints=desc.num_gate_constraints,
                           num_constants=desc.num_constants, gates=desc.gates)


@pytest.fixture(scope="module")
def traced(ctx):
    made = {}

    def get(name):
        if name not in made:
            desc, pih, prog = _circuit(name)
            rb, chh = int(desc.rate_bits), int(desc.cap_height)
            cs = ctx.batch_from_values(np.concatenate([np.asarray(desc.constants, np.uint64), np.asarray(desc.sigmas, np.uint64)]), rb, chh)
            wb = ctx.batch_from_values(desc.wires, rb, chh)
            made[name] = (desc, pih, ctx.gate_program(prog), cs, wb)
        return made[name]
    yield get
    for _d, _p, g, cs, wb in made.values():
        g.free(); cs.free(); wb.free()


def _check_traced(traced, name, sub_bits, nch):
    desc, pih, g, cs, wb = traced(name)
    alphas = _rand(100 * sub_bits + nch, (nch,))
    want = pr.gate_sums(_with_challenges(desc, nch), _rows(cs, sub_bits, int(desc.num_constants)), _rows(wb, sub_bits), alphas, pih)
    got = g.sums([cs, wb], sub_bits, alphas, pih)
    assert want.any() and got.shape == want.shape == (nch, 16 << sub_bits)
    assert (got == want).all(), _first_diff(got, want)


@pytest.mark.parametrize("sub_bits", [3, 1, 0])
@pytest.mark.parametrize("name", ["seam", "ext"])
def test_traced_programs_are_gate_sums(traced, name, sub_bits):
    _check_traced(traced, name, sub_bits, 2)


@pytest.mark.parametrize("nch", [1, 3, 4])
def test_traced_seam_program_at_one_three_and_four_challenges(traced, nch):
    _check_traced(traced, "seam", 3, nch)


# ------------------------------------------------------------------ 2. random programs against the restated interpreter
@functools.lru_cache(maxsize=None)
def _random_program(seed=7, long_gate=1500):
    """Straight-line code over 24 virtual registers that all stay alive to the last gate, so virtual register i is physical register i
    and every result overwrites a register that is still in use."""
    rng = np.random.default_rng(seed)
    asm = gp.Assembler(ORACLE_COLS, NUM_PARAMS)
    regs = [asm.reg() for _ in range(gp.MAX_REGS)]
    ops = (asm.add, asm.sub, asm.mul)

    def col(kind=None):
        o = int(rng.integers(len(ORACLE_COLS)))
        c = int(rng.integers(ORACLE_COLS[o]))
        return asm.col_next(o, c) if (rng.integers(2) if kind is None else kind) else asm.col(o, c)

    def imm():
        return asm.imm(int(rng.integers(0, 1 << 63)) * 2 % P if rng.integers(4) else [0, 1, P - 1][int(rng.integers(3))])

    def reg():
        return regs[int(rng.integers(len(regs)))]
    makers = (reg, lambda: col(0), lambda: col(1), imm, lambda: asm.param(int(rng.integers(NUM_PARAMS))), lambda: asm.x)

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
    prog = asm.assemble()
    assert prog.num_regs == prog.max_live == gp.MAX_REGS and prog.max_constraints == long_gate and len(prog) > 2 * long_gate
    assert [i.dst.index for i in prog.instructions[:gp.MAX_REGS]] == list(range(gp.MAX_REGS))
    kinds = {(side, o.kind) for i in prog.instructions for side, o in (("a", i.a), ("b", i.b)) if o is not None}
    assert kinds == {(s, k) for s in "ab" for k in range(6)}
    return prog


def _oracle_values(lg, K=1, seed=50):
    return [_rand(seed + o, (K, c, 1 << lg)) for o, c in enumerate(ORACLE_COLS)]


# (log_n, sub_bits, rate_bits): M = 64 and 128, one block with dead lanes (8 of 32 and 32 of 64 slots of each plane live); M = 4096, 16 blocks of
# 8 planes; M = 512, two blocks of one plane (QL = 256) under rate_bits 1
SHAPES = [(3, 3, 3), (5, 2, 3), (9, 3, 3), (9, 0, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "2^%d sub_bits %d rate_bits %d" % s)
def test_random_program_is_the_restated_interpreter(ctx, shape):
    lg, sub_bits, rb = shape
    prog = _random_program()
    assert glp.gate_program_check(prog) == 1500
    vals = _oracle_values(lg)
    bs = [ctx.batch_from_values(v[0], rb, min(4, lg + rb)) for v in vals]
    g = ctx.gate_program(prog)
    alphas, params = _rand(3 * lg + sub_bits, (2,)), _rand(77, (NUM_PARAMS,))
    want = gr.run(prog, [_rows(b, sub_bits) for b in bs], sub_bits, alphas, params)
    got = g.sums(bs, sub_bits, alphas, params)
    assert got.shape == want.shape == (2, 1 << (lg + sub_bits)) and (got == want).all(), _first_diff(got, want)
    g.free()
    for b in bs:
        b.free()


# ------------------------------------------------------------------ 3. boundary values
def test_boundary_values(ctx):
    lg, sub_bits = 3, 2
    consts = [0, 1, P - 1]
    b = ctx.batch_from_values(np.array([[v] * (1 << lg) for v in consts], np.uint64), 3, 4)      # constant polynomials: constant LDEs
    asm = gp.Assembler([3])
    srcs = [(asm.col(0, j), v) for j, v in enumerate(consts)] + [(asm.imm(v), v) for v in consts]
    r = asm.reg()
    expect = []
    for op, f in ((asm.add, lambda x, y: x + y), (asm.sub, lambda x, y: x - y), (asm.mul, lambda x, y: x * y)):
        for oa, va in srcs:
            for ob, vb in srcs:
                op(r, oa, ob)
                asm.emit(r)
                expect.append(f(va, vb) % P)
    asm.emit(asm.col(0, 2))                                    # p - 1 against alpha^108 ...
    expect.append(P - 1)
    asm.end(asm.imm(P - 1))
    asm.emit(asm.imm(P - 1))                                   # ... and p - 1 against alpha^0 = 1, with alpha = p - 1 below
    asm.emit(asm.col(0, 2))                                    # (p - 1) * (p - 1)
    asm.end(asm.col(0, 2))
    prog = asm.assemble()
    assert len(expect) == 109 and list(prog.pool) == consts
    g = ctx.gate_program(prog)
    alphas = np.array([P - 1, 1, 0, _rand(1, (1,))[0]], np.uint64)
    got = g.sums([b], sub_bits, alphas)
    want = gr.run(prog, [_rows(b, sub_bits)], sub_bits, alphas)
    assert (got == want).all(), _first_diff(got, want)
    for c, alpha in enumerate(int(a) for a in alphas):         # and in plain integers, the same on every point
        first = sum(v * pow(alpha, t, P) for t, v in enumerate(expect)) % P
        second = ((P - 1) + (P - 1) * alpha) % P
        assert (got[c] == np.uint64((first * (P - 1) + second * (P - 1)) % P)).all(), c
    g.free(); b.free()


# ------------------------------------------------------------------ 4. three proofs, device output, end to end, refusals
@pytest.mark.parametrize("salted", [False, True], ids=["per-proof wires, one shared oracle", "all per proof, salted"])
def test_three_proofs_in_one_call(ctx, salted):
    lg, sub_bits, rb, K = 4, 3, 3, 3
    prog = _random_program(seed=9, long_gate=60)
    g = ctx.gate_program(prog)
    vals = _oracle_values(lg, K, seed=70)
    seed = SEED if salted else None
    bs = [ctx.batch_many_from_values(v, rb, 4, 0, seed) if salted or o != 1 else ctx.batch_from_values(v[0], rb, 4) for o, v in enumerate(vals)]
    assert [b.num_proofs for b in bs] == ([3, 3, 3] if salted else [3, 1, 3])
    assert all(b.leaf_len == b.ncols + 4 for b in bs) if salted else True
    alphas, params = _rand(5, (K, 2)), _rand(6, (K, NUM_PARAMS))
    got = g.sums(bs, sub_bits, alphas, params)
    assert got.shape == (K, 2, 1 << (lg + sub_bits))
    for k in range(K):
        members = [b.member(k) if b.num_proofs > 1 else b for b in bs]
        one = g.sums(members, sub_bits, alphas[k], params[k])
        want = gr.run(prog, [_rows(m, sub_bits) for m in members], sub_bits, alphas[k], params[k])
        assert (one == want).all(), (k, _first_diff(one, want))
        assert (got[k] == one).all(), (k, _first_diff(got[k], one))
    assert (got[0] != got[1]).any() and (got[1] != got[2]).any()
    do = ctx.dev_alloc(got.nbytes)                              # device output: read back, it is the host-output call's
    try:
        assert g.sums(bs, sub_bits, alphas, params, out_dev_ptr=do) is None
        back = np.empty_like(got)
        ctx.dev_download(do, back)
        assert (back == got).all(), _first_diff(back, got)
    finally:
        ctx.dev_free(do)
    g.free()
    for b in bs:
        b.free()


def test_the_seam_end_to_end_with_a_gate_program(ctx, oracle):
    """tests/test_gpu_perm_seam.py::test_the_seam_end_to_end_without_a_session with the gate constraints on the GPU as well: the gate
    sums go from GateProgram.sums to perm_quotient_values through HBM"""
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
    words = nch << (int(desc.degree_bits) + sub_bits)
    dgs, dq = ctx.dev_alloc(words * 8), ctx.dev_alloc(words * 8)
    try:
        assert g.sums([cs, wb], sub_bits, alphas, pih, out_dev_ptr=dgs) is None
        assert ctx.perm_quotient_values(desc, cs, nc, wb, zb, sub_bits, betas, gammas, alphas, gate_sums_dev_ptr=dgs, out_dev_ptr=dq) is None
        qb = ctx.batch_from_coset_values(None, sub_bits, rb, chh, dev_ptr=dq, shape=(nch, words // nch))
    finally:
        ctx.synchronize()
        ctx.dev_free(dgs); ctx.dev_free(dq)
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
    g.free()
    for b in (cs, wb, zb, qb):
        b.free()


def _refused(fn, *needles):
    with pytest.raises(glp.GlpError) as e:
        fn()
    assert e.value.code == -1, str(e.value)                # GLP_ERR_ARG
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def test_refusals(ctx):
    L = glp.load_library()
    lg, rb, n = 4, 3, 16
    prog = _random_program(seed=9, long_gate=60)
    g = ctx.gate_program(prog)
    vals = _oracle_values(lg, 3, seed=70)
    bs = [ctx.batch_from_values(v[0], rb, 4) for v in vals]
    alphas, params = _rand(5, (2,)), _rand(6, (NUM_PARAMS,))
    other_lg = ctx.batch_from_values(_rand(1, (ORACLE_COLS[1], 2 * n)), rb, 4)
    other_rb = ctx.batch_from_values(vals[1][0], 2, 4)
    narrow = ctx.batch_from_values(vals[1][0][:16], rb, 4)
    salted_narrow = ctx.batch_from_values_salted(vals[1][0][:14], SEED, rb, 4)       # 14 polynomials and 4 salts: the salts are not polynomials
    two = ctx.batch_many_from_values(vals[1][:2], rb, 4)
    ctx2 = glp.Context(0)
    foreign = ctx2.batch_from_values(vals[1][0], rb, 4)
    g2 = ctx2.gate_program(prog)
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.stage_reset()

    def sums(o=None, sub_bits=rb, a=alphas, p=params, prog_=g):
        return prog_.sums(bs if o is None else [bs[0], o, bs[2]], sub_bits, a, p)

    def bad(v, i):
        v = np.array(v, np.uint64)
        v.reshape(-1)[i] = P + 3
        return v
    name = "glp_gate_program_sums"
    _refused(lambda: sums(sub_bits=rb + 1), name, "sub_bits", "rate_bits")
    _refused(lambda: sums(o=other_lg), name, "log_n", "oracles[1]")
    _refused(lambda: sums(o=other_rb), name, "rate_bits", "oracles[1]")
    _refused(lambda: sums(o=foreign), name, "oracles[1]", "ctx")
    _refused(lambda: sums(prog_=g2), name, "program", "ctx")
    _refused(lambda: sums(o=narrow), name, "oracles[1]", "16 polynomials", "oracle_cols[1] is 17")
    _refused(lambda: sums(o=salted_narrow), name, "oracles[1]", "14 polynomials", "salts")
    _refused(lambda: sums(o=two), name, "oracles[1]", "2 members", "num_proofs = 1")
    a3 = np.stack([alphas] * 3)
    _refused(lambda: sums(o=two, a=a3, p=np.stack([params] * 3)), name, "oracles[1]", "2 members", "num_proofs = 3")
    _refused(lambda: sums(a=_rand(1, (5,))), name, "num_challenges", "1..4")
    _refused(lambda: sums(a=bad(alphas, 1)), name, "alphas[0][1]", "canonical")
    _refused(lambda: sums(p=bad(params, 2)), name, "params[0][2]", "canonical")
    _refused(lambda: sums(p=None), name, "params", "null", "num_params = 3")
    # raw calls: null pointers and the counts the binding derives
    hs = (C.c_void_p * 3)(*[b._h for b in bs])
    out = np.zeros(2 << (lg + rb), np.uint64)
    p_ = binding._p

    def raw(c=ctx._h, prog_=g._h, K=1, oracles=hs, nch=2, a=alphas, pr_=params, o=out):
        binding._chk(L.glp_gate_program_sums(c, prog_, K, oracles, rb, nch, None if a is None else p_(a),
                                             None if pr_ is None else p_(pr_), None if o is None else p_(o), 0))
    _refused(lambda: raw(c=None), name, "ctx", "null")
    _refused(lambda: raw(prog_=None), name, "program", "null")
    _refused(lambda: raw(oracles=None), name, "oracles", "null")
    _refused(lambda: raw(oracles=(C.c_void_p * 3)(bs[0]._h, None, bs[2]._h)), name, "oracles[1]", "null")
    _refused(lambda: raw(o=None), name, "out", "null")
    _refused(lambda: raw(a=None), name, "alphas", "null")
    _refused(lambda: raw(K=0), name, "num_proofs")
    _refused(lambda: raw(K=4097), name, "num_proofs")
    _refused(lambda: raw(nch=0), name, "num_challenges")
    # glp_gate_program_create refuses what glp_gate_program_check refuses, under its own name
    d, _keep = glp.gate_program_desc(prog, num_regs=gp.MAX_REGS - 1)
    h = C.c_void_p()
    assert L.glp_gate_program_create(ctx._h, C.byref(d), C.byref(h)) == -1 and not h.value
    msg = L.glp_last_error().decode()
    assert "glp_gate_program_create" in msg and "instruction 23" in msg and "field dst" in msg, msg
    assert ctx.stages() == [], "a refused call reached a launch: %s" % (ctx.stages(),)
    sums()                                                       # and the unrefused call is served, under its stage name
    st = ctx.stages()
    assert [s[0] for s in st] == ["gate_program.sums"]
    named = len({(o.kind in (gp.COL, gp.COL_NEXT), o.oracle, o.index) for i in prog.instructions for o in (i.a, i.b)
                 if o is not None and o.kind in (gp.COL, gp.COL_NEXT)})
    assert st[0][2] == 8.0 * (n << rb) * (named + 2), (st[0], named)
    ctx.set_profiling(False)
    g2.free(); foreign.free(); ctx2.close()
    g.free()
    for b in bs + [other_lg, other_rb, narrow, salted_narrow, two]:
        b.free()
