"""Gate programs (glp_gate_program_*), the part that needs no GPU.
1. programs traced from zeta_identity.gate_constraints, run by the restated interpreter (tests/gate_program_restate.py) on row-major
   rows of the oracle's LDE, are perm_restate.gate_sums word for word: the semantics in include/glp.h say what the seam needs.
2. the assembler: register allocation within its bound on those circuits, an error past it, immediates deduplicated, EMIT hoisting
   keeps the meaning.
3. glp_gate_program_check (host only) accepts the traced programs, returns their max_constraints, and names instruction and field
   in every refusal.
The device side is tests/test_gpu_gate_program.py."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
from plonky2_lib_amd import gate_program as gp
import plonky2_lib_amd.synth as synth
import coset_quotient as cq
import gate_program_restate as gr
import perm_restate as pr

NEW = ["glp_gate_program_check", "glp_gate_program_create", "glp_gate_program_free", "glp_gate_program_sums"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = cq.P


def lde_rows(oracle, values, rate_bits, sub_bits):
    """row-major [M][ncols] values on g <W_M> of the polynomials with these values on H"""
    step = 1 << (rate_bits - sub_bits)
    return np.stack([oracle.lde(oracle.ifft(v), rate_bits)[::step] for v in np.asarray(values, np.uint64)], axis=1)


@functools.lru_cache(maxsize=None)
def _circuit(name):
    from oracle import oracle
    oracle.build()
    if name == "seam":
        desc = cq.seam_circuit(oracle)
        pih = oracle.hash_no_pad(np.asarray(desc.public_inputs, np.uint64))
    else:
        desc, pih = synth.ext_gates_circuit(4), np.zeros(4, np.uint64)
    prog, counts = gr.trace_circuit(desc)
    return desc, pih, prog, counts


@pytest.mark.parametrize("name", ["seam", "ext"])
@pytest.mark.parametrize("sub_bits", [3, 0])
def test_traced_program_restated_is_gate_sums(oracle, name, sub_bits):
    desc, pih, prog, _counts = _circuit(name)
    rb = int(desc.rate_bits)
    cs = np.concatenate([np.asarray(desc.constants, np.uint64), np.asarray(desc.sigmas, np.uint64)])
    rows = [lde_rows(oracle, v, rb, sub_bits) for v in (cs, desc.wires)]
    alphas = oracle.rand_field(np.random.default_rng(31), (int(desc.num_challenges),))
    want = pr.gate_sums(desc, rows[0], rows[1], alphas, pih)
    assert want.any(), "the circuit's gates contribute nothing"
    got = gr.run(prog, rows, sub_bits, alphas, pih)
    assert got.shape == want.shape and (got == want).all(), "first mismatch at %s" % (np.argwhere(got != want)[:1],)


@pytest.mark.parametrize("name", ["seam", "ext"])
def test_register_allocation_stays_within_its_bound(name):
    desc, _pih, prog, counts = _circuit(name)
    assert 1 <= prog.num_regs <= gp.MAX_REGS and prog.max_live <= gp.MAX_REGS
    assert max(counts) > gp.MAX_REGS or name == "seam"           # the ext circuit has gates with more constraints than registers: hoisting is exercised
    assert len(counts) == len(desc.gates) and prog.max_constraints == max(counts)
    for ins in prog.instructions:
        for o in (ins.dst, ins.a, ins.b):
            assert o is None or o.kind != gp.REG or o.index < prog.num_regs


def test_assembler_refuses_a_twenty_fifth_live_register():
    asm = gp.Assembler([2])
    regs = [asm.reg() for _ in range(gp.MAX_REGS + 1)]
    for r in regs:
        asm.mov(r, asm.col(0, 0))
    for r in regs:
        asm.emit(r)
    asm.end(asm.imm(1))
    with pytest.raises(gp.AssemblerError) as e:
        asm.assemble()
    assert "live" in str(e.value)
    asm = gp.Assembler([2])
    regs = [asm.reg() for _ in range(gp.MAX_REGS)]                # exactly the bound: all alive at the first EMIT
    for r in regs:
        asm.mov(r, asm.col(0, 1))
    for r in regs:
        asm.emit(r)
    asm.end(asm.imm(1))
    prog = asm.assemble()
    assert prog.max_live == gp.MAX_REGS and prog.num_regs == gp.MAX_REGS
    assert sorted(i.dst.index for i in prog.instructions[:gp.MAX_REGS]) == list(range(gp.MAX_REGS))


def test_assembler_pool_operands_and_reuse():
    asm = gp.Assembler([3, 2], num_params=1)
    a, b = asm.imm(5), asm.imm(5 + P)
    assert a == b and asm.imm(0) != a and asm.imm(-1) == asm.imm(P - 1)
    for bad in (lambda: asm.col(2, 0), lambda: asm.col(1, 2), lambda: asm.col_next(0, 3), lambda: asm.param(1)):
        with pytest.raises(gp.AssemblerError):
            bad()
    F = gp.TraceField(asm)
    assert F.lift(7) == asm.imm(7) and F.lift(asm.x) is asm.x
    assert F.mul(F.lift(3), F.lift(4)) == asm.imm(12) and F.sub(F.zero, F.one) == asm.imm(P - 1)      # immediates fold
    t = F.add(asm.col(0, 0), asm.param(0))
    u = F.mul(t, t)                                               # t dies here: u takes its register
    asm.emit(u)
    asm.end(F.one)
    prog = asm.assemble()
    assert [i.op for i in prog.instructions] == [gp.OP_ADD, gp.OP_MUL, gp.OP_EMIT, gp.OP_END]
    assert prog.num_regs == 1 and prog.instructions[1].dst == prog.instructions[1].a == gp.Operand(gp.REG, 0, 0)
    assert list(prog.pool) == [5, 0, P - 1, 1, 7, 3, 4, 12]
    with pytest.raises(gp.AssemblerError):                        # a register read before it is written
        asm2 = gp.Assembler([1])
        asm2.emit(asm2.reg())
        asm2.end(asm2.imm(1))
        asm2.assemble()
    with pytest.raises(gp.AssemblerError):                        # no END at the end
        asm3 = gp.Assembler([1])
        asm3.emit(asm3.col(0, 0))
        asm3.assemble()


def test_hoisting_emits_keeps_the_meaning():
    """the same instructions with and without hoisting compute the same sums; only the registers alive differ"""
    rng = np.random.default_rng(4)
    rows = [gl_rand(rng, (16, 6))]

    def build(hoist):
        asm = gp.Assembler([6])
        F = gp.TraceField(asm)
        for gate in range(2):
            vs = [F.mul(F.add(asm.col(0, j), asm.x), asm.col_next(0, (j + gate) % 6)) for j in range(6)]
            r = asm.reg()
            asm.mov(r, vs[0])
            asm.add(r, r, vs[1])                                  # r written twice: its EMIT stays behind the second write
            for v in vs + [r, asm.col(0, 2)]:
                asm.emit(v)
            asm.end(F.sub(asm.col(0, gate), F.one))
        return asm.assemble(hoist_emits=hoist)
    plain, hoisted = build(False), build(True)
    assert len(plain) == len(hoisted) and [i.a for i in plain.instructions if i.op == gp.OP_EMIT][-1] == gp.Operand(gp.COL, 2, 0)
    assert hoisted.max_live < plain.max_live
    alphas = gl_rand(rng, (2,))
    assert (gr.run(plain, rows, 1, alphas) == gr.run(hoisted, rows, 1, alphas)).all()


def gl_rand(rng, shape):
    import plonky2_lib_amd.gl_numpy as gl
    return gl.rand(rng, shape)


# ------------------------------------------------------------------ glp_gate_program_check
def test_new_functions_are_declared_exported_and_bound():
    glp.build_library()
    declared = glp.exported_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", glp.library_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = glp.load_library()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in declared, name + " is not declared in include/glp.h"
        assert name in exported, name + " is not exported by libglprover.so"
        assert getattr(L, name).argtypes, name + " has no argtypes in binding.py"
        assert "fn " + name + "(" in integration, name + " is missing from INTEGRATION.md's extern block"
    assert hasattr(glp.Context, "gate_program") and callable(glp.gate_program_check) and hasattr(glp.GateProgram, "sums")
    # the C struct: pointer, u32, padding, pointer, four u32, pointer
    assert binding._GateProgramDesc.pool.offset == 16 and binding._GateProgramDesc.oracle_cols.offset == 40 and C.sizeof(binding._GateProgramDesc) == 48
    hdr = open(os.path.join(ROOT, "include", "glp.h")).read()
    for macro, value in (("GLP_GP_MAX_REGS", gp.MAX_REGS), ("GLP_GP_MAX_INSTRUCTIONS", gp.MAX_INSTRUCTIONS), ("GLP_GP_MAX_CONSTRAINTS", gp.MAX_CONSTRAINTS),
                         ("GLP_GP_MAX_ORACLES", gp.MAX_ORACLES), ("GLP_GP_OP_ADD", gp.OP_ADD), ("GLP_GP_OP_SUB", gp.OP_SUB), ("GLP_GP_OP_MUL", gp.OP_MUL),
                         ("GLP_GP_OP_MOV", gp.OP_MOV), ("GLP_GP_OP_EMIT", gp.OP_EMIT), ("GLP_GP_OP_END", gp.OP_END), ("GLP_GP_REG", gp.REG),
                         ("GLP_GP_COL", gp.COL), ("GLP_GP_COL_NEXT", gp.COL_NEXT), ("GLP_GP_IMM", gp.IMM), ("GLP_GP_PARAM", gp.PARAM), ("GLP_GP_X", gp.X),
                         ("GLP_GP_DST_SHIFT", gp._DST_SHIFT), ("GLP_GP_A_SHIFT", gp._A_SHIFT), ("GLP_GP_B_SHIFT", gp._B_SHIFT),
                         ("GLP_GP_COL_ORACLE_SHIFT", gp._COL_ORACLE_SHIFT)):
        assert re.search(r"#define %s %du?\s" % (macro, value), hdr), macro


@pytest.mark.parametrize("name", ["seam", "ext"])
def test_check_accepts_the_traced_programs(name):
    _desc, _pih, prog, counts = _circuit(name)
    assert glp.gate_program_check(prog) == max(counts)


def _refused(fn, *needles):
    with pytest.raises(glp.GlpError) as e:
        fn()
    assert e.value.code == -1, str(e.value)                # GLP_ERR_ARG
    for needle in needles:
        assert needle in str(e.value), str(e.value)


class _Raw:
    """a program given as raw fields, for descriptions no assembler would produce"""

    def __init__(self, code, pool=(), num_regs=2, num_params=1, oracle_cols=(3, 2)):
        self.code, self.pool = np.array(code, np.uint64), np.array(pool, np.uint64)
        self.num_regs, self.num_params, self.oracle_cols = num_regs, num_params, list(oracle_cols)


def _w(op, dst=0, a=0, b=0):
    return op | dst << 4 | a << 9 | b << 36


def _o(kind, index=0, oracle=0):
    return gp.encode_operand(gp.Operand(kind, index, oracle))


def test_check_names_instruction_and_field_in_every_refusal():
    check = glp.gate_program_check
    col, end = _o(gp.COL, 1, 0), _w(gp.OP_END, a=_o(gp.X))
    good = _Raw([_w(gp.OP_MOV, 0, col), _w(gp.OP_ADD, 1, _o(gp.REG, 0), _o(gp.IMM, 0)), _w(gp.OP_EMIT, a=_o(gp.REG, 1)), end], pool=[5])
    assert check(good) == 1
    assert (gp.Assembler([3, 2], 1).col(0, 1), gp.encode(gp.Instruction(gp.OP_MOV, gp.Operand(gp.REG, 0, 0), gp.Operand(gp.COL, 1, 0), None))) == \
        (gp.Operand(gp.COL, 1, 0), _w(gp.OP_MOV, 0, col))

    def prog(*words, **kw):
        return _Raw(list(words) + [end], pool=[5], **kw)
    # opcodes and operand kinds
    _refused(lambda: check(prog(_w(0, 0, col))), "instruction 0", "field op", "opcode 0")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, col), _w(7, 0, col))), "instruction 1", "field op", "opcode 7")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, col) | 1 << 63)), "instruction 0", "field op", "bit 63")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, 6))), "instruction 0", "field a", "operand kind 6")
    _refused(lambda: check(prog(_w(gp.OP_ADD, 0, col, 7))), "instruction 0", "field b", "operand kind 7")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, col, col))), "instruction 0", "field b", "one operand")
    _refused(lambda: check(prog(_w(gp.OP_EMIT, 1, col))), "instruction 0", "field dst")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, _o(gp.X, 1)))), "instruction 0", "field a", "X")
    # registers
    _refused(lambda: check(prog(_w(gp.OP_MOV, 2, col))), "instruction 0", "field dst", "register 2", "num_regs = 2")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, col), _w(gp.OP_MOV, 1, _o(gp.REG, 2)))), "instruction 1", "field a", "register 2", "num_regs")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, col), _w(gp.OP_SUB, 1, _o(gp.REG, 0), _o(gp.REG, 1)))), "instruction 1", "field b", "register 1",
             "before it is written")
    _refused(lambda: check(prog(_w(gp.OP_EMIT, a=_o(gp.REG, 0)))), "instruction 0", "field a", "before it is written")
    _refused(lambda: check(prog(_w(gp.OP_ADD, 0, _o(gp.REG, 0), col))), "instruction 0", "field a", "before it is written")      # its own destination
    # pool, params, oracles, columns
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, _o(gp.IMM, 1)))), "instruction 0", "field a", "pool index 1", "num_pool = 1")
    _refused(lambda: check(prog(_w(gp.OP_MUL, 0, col, _o(gp.PARAM, 1)))), "instruction 0", "field b", "param index 1", "num_params = 1")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, _o(gp.COL, 0, 2)))), "instruction 0", "field a", "oracle index 2", "num_oracles = 2")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, _o(gp.COL, 3, 0)))), "instruction 0", "field a", "column index 3", "oracle_cols[0] = 3")
    _refused(lambda: check(prog(_w(gp.OP_MOV, 0, col), _w(gp.OP_MOV, 0, _o(gp.COL_NEXT, 2, 1)))), "instruction 1", "field a", "column index 2",
             "oracle_cols[1] = 2")
    _refused(lambda: check(_Raw([end], pool=[5, P])), "pool[1]", "canonical")
    # the description
    _refused(lambda: check(good, num_regs=0), "num_regs")
    _refused(lambda: check(good, num_regs=gp.MAX_REGS + 1), "num_regs", "24")
    assert check(prog(_w(gp.OP_MOV, gp.MAX_REGS - 1, col), num_regs=gp.MAX_REGS)) == 0
    _refused(lambda: check(good, num_oracles=0), "num_oracles")
    _refused(lambda: check(good, num_oracles=5), "num_oracles")
    _refused(lambda: check(good, oracle_cols=None), "oracle_cols", "null")
    _refused(lambda: check(good, num_instructions=0), "num_instructions", "empty")
    _refused(lambda: check(good, code=None), "code", "null")
    _refused(lambda: check(good, pool=None), "pool", "null")
    too_long = _Raw([_w(gp.OP_EMIT, a=_o(gp.X))] * gp.MAX_INSTRUCTIONS + [end])
    _refused(lambda: check(too_long), "num_instructions", "65536")
    # the last instruction, and the EMITs of one gate
    _refused(lambda: check(_Raw([end, _w(gp.OP_EMIT, a=_o(gp.X))])), "instruction 1", "field op", "not END")
    _refused(lambda: check(_Raw([_w(gp.OP_MOV, 0, col)])), "instruction 0", "field op", "not END")
    emit = _w(gp.OP_EMIT, a=_o(gp.X))
    assert check(_Raw([emit] * gp.MAX_CONSTRAINTS + [end, emit, end])) == gp.MAX_CONSTRAINTS
    _refused(lambda: check(_Raw([emit, end] + [emit] * (gp.MAX_CONSTRAINTS + 1) + [end])), "instruction %d" % (gp.MAX_CONSTRAINTS + 2), "field op", "4096")
    L = glp.load_library()
    out = C.c_uint32(7)
    assert L.glp_gate_program_check(None, C.byref(out)) == -1 and b"desc" in L.glp_last_error() and out.value == 0
    d, _keep = glp.gate_program_desc(good)
    assert L.glp_gate_program_check(C.byref(d), None) == -1 and b"max_constraints_out" in L.glp_last_error()
    h = C.c_void_p()
    assert L.glp_gate_program_create(None, C.byref(d), C.byref(h)) == -1 and b"ctx" in L.glp_last_error() and not h.value
    assert L.glp_gate_program_sums(None, None, 1, None, 0, 1, None, None, None, 0) == -1 and b"null" in L.glp_last_error()
    L.glp_gate_program_free(None)
