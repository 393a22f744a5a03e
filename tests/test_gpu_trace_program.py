"""Gate programs on the rows of H (include/glp.h: glp_gate_program_rows) against tests/trace_program_restate.py.  Fixed seeds, every
word compared.
1. random single-gate programs: 24 registers all live, every operand kind on both sides, results that overwrite one of their own
   operands, 1 EMIT and about 300 EMITs; n = 16 (one block, 240 dead lanes) and n = 512 (two blocks: COL_NEXT of row 255 is the
   other block's row 256 and row 511 wraps to row 0).
2. X is w_n^i, COL_NEXT is the next row, in plain integers.
3. three proofs with one shared and two per-proof inputs; host and device inputs and outputs; a device input word >= p is reduced.
4. every refusal by name, none of them reaching a launch; the served call runs under the stage name gate_program.rows.
The CPU side (the restatement against direct evaluation) is tests/test_running_columns.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
from plonky2_lib_amd import gate_program as gp
import plonky2_lib_amd.gl_numpy as gl
import coset_quotient as cq
import trace_program_restate as tr

pytestmark = pytest.mark.gpu

P = cq.P
ORACLE_COLS = (5, 17, 3)
NUM_PARAMS = 3


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _rand(seed, shape):
    return gl.rand(np.random.default_rng(seed), shape)


def _first_diff(got, want):
    return "first mismatch at %s" % (tuple(np.argwhere(got != want)[0]) if (got != want).any() else None,)


@functools.lru_cache(maxsize=None)
def _random_program(seed, emits):
    """One gate over 24 virtual registers that all stay alive to the end, so virtual register i is physical register i and every
    result overwrites a register that is still in use.  emits == 1: the only EMIT is the sum of all 24."""
    rng = np.random.default_rng(seed)
    asm = gp.Assembler(ORACLE_COLS, NUM_PARAMS)
    regs = [asm.reg() for _ in range(gp.MAX_REGS)]
    ops = (asm.add, asm.sub, asm.mul)

    def col(kind):
        o = int(rng.integers(len(ORACLE_COLS)))
        c = int(rng.integers(ORACLE_COLS[o]))
        return asm.col_next(o, c) if kind else asm.col(o, c)

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
    if emits == 1:
        for j in range(100):
            ops[int(rng.integers(3))](reg(), operand(), operand())
        for r in regs[1:]:
            asm.add(regs[0], regs[0], r)
        asm.emit(regs[0])
    else:
        for j in range(emits - len(regs)):
            ops[int(rng.integers(3))](reg(), operand(), operand())
            asm.emit(operand())
        for r in regs:                                         # all 24 read at the very end: all alive throughout
            asm.emit(r)
    asm.end(asm.imm(1))
    prog = asm.assemble()
    assert prog.num_regs == prog.max_live == gp.MAX_REGS and prog.max_constraints == emits and tr.shape_error(prog) is None
    assert [i.dst.index for i in prog.instructions[:gp.MAX_REGS]] == list(range(gp.MAX_REGS))
    kinds = {(side, o.kind) for i in prog.instructions[:-1] for side, o in (("a", i.a), ("b", i.b)) if o is not None}
    assert kinds == {(s, k) for s in "ab" for k in range(6)}
    return prog


def _inputs(lg, K=None, seed=50):
    return [_rand(seed + o, (c, 1 << lg) if K is None else (K, c, 1 << lg)) for o, c in enumerate(ORACLE_COLS)]


# ------------------------------------------------------------------ 1. random programs
@pytest.mark.parametrize("emits", [1, 300])
@pytest.mark.parametrize("lg", [4, 9], ids=["n = 16, one block with dead lanes", "n = 512, two blocks"])
def test_random_program_is_the_restatement(ctx, lg, emits):
    prog = _random_program(7, emits)
    assert glp.gate_program_check(prog) == emits
    g = ctx.gate_program(prog)
    vals, params = _inputs(lg), _rand(77, (NUM_PARAMS,))
    want = tr.run_rows(prog, vals, params)
    got = g.rows(vals, params)
    assert got.shape == want.shape == (emits, 1 << lg) and (got == want).all(), _first_diff(got, want)
    g.free()


# ------------------------------------------------------------------ 2. X and COL_NEXT in plain integers
@pytest.mark.parametrize("lg", [4, 9])
def test_x_is_the_row_s_root_of_unity_and_col_next_the_next_row(ctx, lg):
    n = 1 << lg
    asm = gp.Assembler([2])
    asm.emit(asm.x)
    asm.emit(asm.col_next(0, 1))
    asm.emit(asm.col(0, 1))
    asm.end(asm.imm(1))
    g = ctx.gate_program(asm.assemble())
    vals = np.stack([np.zeros(n, np.uint64), np.arange(n, dtype=np.uint64) + np.uint64(1000)])
    got = g.rows([vals])
    w, x = cq.root_of_unity(lg), 1
    for i in range(n):
        assert int(got[0, i]) == x, i
        x = x * w % P
    assert x == 1
    assert [int(v) for v in got[1]] == [1000 + (i + 1) % n for i in range(n)]      # row 255 -> 256 across the blocks, row n - 1 -> 0
    assert (got[2] == vals[1]).all()
    g.free()


# ------------------------------------------------------------------ 3. three proofs; host and device memory
def _on_device(ctx, arr):
    a = np.ascontiguousarray(arr, np.uint64)
    d = ctx.dev_alloc(a.nbytes)
    ctx.dev_upload(d, a)
    return d


def test_three_proofs_shared_and_per_proof_inputs_host_and_device(ctx):
    lg, K = 9, 3
    prog = _random_program(9, 40)
    g = ctx.gate_program(prog)
    per = _inputs(lg, K, seed=70)
    vals = [per[0], per[1][1].copy(), per[2]]                   # input 1 is shared by the three proofs
    for v in vals:
        v.reshape(-1)[::7] &= np.uint64(0x7FFFFFFF)             # values v with p + v < 2^64, for the device copies below
    params = _rand(6, (K, NUM_PARAMS))
    want = np.stack([tr.run_rows(prog, [vals[0][k], vals[1], vals[2][k]], params[k]) for k in range(K)])
    assert (want[0] != want[1]).any() and (want[1] != want[2]).any()
    got = g.rows(vals, params)
    assert got.shape == want.shape == (K, 40, 1 << lg) and (got == want).all(), _first_diff(got, want)
    # the same from HBM to HBM, with words >= p among the inputs: p + v where v is small enough, read as v
    lifted = []
    for v in vals:
        u = v.copy()
        u.reshape(-1)[::7] += np.uint64(P)
        assert (u.reshape(-1)[::7] >= np.uint64(P)).all()
        lifted.append(u)
    ptrs = [_on_device(ctx, u) for u in lifted]
    do = ctx.dev_alloc(want.nbytes)
    try:
        assert g.rows([v.shape for v in vals], params, in_dev_ptrs=ptrs, out_dev_ptr=do) is None
        back = np.empty_like(want)
        ctx.dev_download(do, back)
        assert (back == want).all(), _first_diff(back, want)
        for p_, u in zip(ptrs, lifted):                         # the caller's inputs are read, never written
            b = np.empty_like(u)
            ctx.dev_download(p_, b)
            assert (b == u).all()
        got = g.rows([v.shape for v in vals], params, in_dev_ptrs=ptrs)      # device inputs, host output
        assert (got == want).all(), _first_diff(got, want)
    finally:
        ctx.dev_free(do)
        for p_ in ptrs:
            ctx.dev_free(p_)
    g.free()


# ------------------------------------------------------------------ 4. refusals
def _refused(fn, *needles):
    with pytest.raises(glp.GlpError) as e:
        fn()
    assert e.value.code == -1, str(e.value)                # GLP_ERR_ARG
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def _shaped(build):
    asm = gp.Assembler(ORACLE_COLS, NUM_PARAMS)
    build(asm)
    return asm.assemble()


def test_refusals(ctx):
    L = glp.load_library()
    lg, n, K = 4, 16, 3
    name = "glp_gate_program_rows"
    prog = _random_program(9, 40)
    g = ctx.gate_program(prog)
    per = _inputs(lg, K, seed=70)
    vals = [per[0], per[1][1], per[2]]
    params = _rand(6, (K, NUM_PARAMS))
    ctx2 = glp.Context(0)
    g2 = ctx2.gate_program(prog)
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.stage_reset()
    # the program's shape

    def shaped(build, *needles):
        gs = ctx.gate_program(_shaped(build))
        _refused(lambda: gs.rows([v[0] if v.ndim == 3 else v for v in vals], params[0]), name, *needles)
        gs.free()
    shaped(lambda s: (s.emit(s.x), s.end(s.imm(1)), s.emit(s.x), s.end(s.imm(1))), "instruction 1", "field op", "END")

    def end_on_a_register(s):
        r = s.reg()
        s.mov(r, s.x)
        s.emit(s.x)
        s.end(r)
    shaped(end_on_a_register, "instruction 2", "field a", "IMM(1)", "kind 0")
    shaped(lambda s: (s.emit(s.x), s.end(s.x)), "instruction 1", "field a", "IMM(1)", "kind 5")
    shaped(lambda s: (s.emit(s.imm(1)), s.end(s.imm(2))), "instruction 1", "field a", "IMM(1)", "pool word")
    shaped(lambda s: (s.end(s.imm(1)),), "instruction 0", "field op", "EMIT")

    def bad(v, i):
        v = np.array(v, np.uint64)
        v.reshape(-1)[i] = P + 3
        return v
    _refused(lambda: g.rows(vals, bad(params, 4)), name, "params[1][1]", "canonical")
    _refused(lambda: g.rows([vals[0], bad(vals[1], 2 * n + 5), vals[2]], params), name, "inputs[1]", "word %d" % (2 * n + 5), "canonical")
    _refused(lambda: g.rows([vals[0], vals[1], bad(vals[2], 3 * n * 3 - 1)], params), name, "inputs[2]", "word %d" % (3 * n * 3 - 1), "canonical")
    # raw calls: null pointers, counts and member counts the binding derives
    arrs = [np.ascontiguousarray(v) for v in vals]
    ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in arrs])
    members = (C.c_uint32 * 3)(3, 1, 3)
    out = np.zeros(K * 40 * n, np.uint64)
    p_ = binding._p

    def raw(c=ctx._h, prog_=g._h, K_=K, lg_=lg, ins=ptrs, mem=members, pr_=params, o=out):
        binding._chk(L.glp_gate_program_rows(c, prog_, K_, lg_, ins, mem, 0, None if pr_ is None else p_(pr_), None if o is None else p_(o), 0))
    _refused(lambda: raw(c=None), name, "ctx", "null")
    _refused(lambda: raw(prog_=None), name, "program", "null")
    _refused(lambda: raw(prog_=g2._h), name, "program", "ctx")
    _refused(lambda: raw(ins=None), name, "inputs", "null")
    _refused(lambda: raw(mem=None), name, "input_members", "null")
    _refused(lambda: raw(o=None), name, "out", "null")
    _refused(lambda: raw(ins=(C.c_void_p * 3)(arrs[0].ctypes.data, None, arrs[2].ctypes.data)), name, "inputs[1]", "null")
    _refused(lambda: raw(pr_=None), name, "params", "null", "num_params = 3")
    _refused(lambda: raw(K_=0), name, "num_proofs")
    _refused(lambda: raw(K_=4097), name, "num_proofs")
    _refused(lambda: raw(lg_=25), name, "log_n")
    _refused(lambda: raw(mem=(C.c_uint32 * 3)(3, 2, 3)), name, "input_members[1] = 2", "num_proofs = 3")
    _refused(lambda: raw(mem=(C.c_uint32 * 3)(3, 1, 0)), name, "input_members[2] = 0")
    assert ctx.stages() == [], "a refused call reached a launch: %s" % (ctx.stages(),)
    raw()                                                        # and the unrefused call is served, under its stage name
    assert [s[0] for s in ctx.stages()] == ["gate_program.rows"]
    want = np.stack([tr.run_rows(prog, [vals[0][k], vals[1], vals[2][k]], params[k]) for k in range(K)])
    assert (out.reshape(want.shape) == want).all()
    ctx.set_profiling(False)
    g2.free(); ctx2.close()
    g.free()
