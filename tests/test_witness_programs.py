"""Unit programs on the host (include/glp.h, UNIT PROGRAMS): every refusal of glp_witness_program_check by its message, and the
assembler's ready-made programs, BITS and LT run through tests/witness_program_restate.py against plain Python on the edge values.
glp_witness_program_check is host code and needs no context, so this file runs without a GPU, as tests/test_abi.py does."""
import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import witness_program as wprog
import witness_program_restate as wpr

P = wpr.P
EDGE = wpr.EDGE_VALUES
REG, COL, COL_NEXT, IMM, PARAM, X = 0, 1, 2, 3, 4, 5
ADD, SUB, MUL, MOV, EMIT, END, INV0, BITS, LT = range(1, 10)


@pytest.fixture(scope="module", autouse=True)
def library():
    glp.build_library()


def opd(kind, payload=0):
    return kind | payload << 3


def ins(op, dst=0, a=0, b=0):
    return op | dst << 4 | a << 9 | b << 36


class Bag:
    def __init__(self, code, pool=(1, 5), num_regs=2, num_inputs=1, num_outputs=1):
        self.code, self.pool = np.array(code, np.uint64), np.array(pool, np.uint64)
        self.num_regs, self.num_inputs, self.num_outputs = num_regs, num_inputs, num_outputs


END1 = ins(END, a=opd(IMM, 0))                     # pool word 0 is 1
GOOD = [ins(MOV, 0, opd(COL, 0)), ins(EMIT, a=opd(REG, 0)), END1]


def test_a_well_formed_program_passes():
    glp.witness_program_check(Bag(GOOD))
    for prog in (wprog.wire_split([63, 63]), wprog.wire_split([16] * 5), wprog.low_high(7, 20), wprog.equality()):
        glp.witness_program_check(prog)


REFUSALS = [
    ("opcode 10", Bag([ins(10, 0, opd(COL, 0))] + GOOD[1:]), r"instruction 0, field op: 0x[0-9a-f]{16} has the unknown opcode 10"),
    ("opcode 0", Bag([0] + GOOD), r"instruction 0, field op: .* unknown opcode 0"),
    ("bit 63", Bag([GOOD[0] | 1 << 63] + GOOD[1:]), r"instruction 0, field op: .*\(bit 63 is set\)"),
    ("dst in EMIT", Bag([GOOD[0], ins(EMIT, 1, opd(REG, 0)), END1]), r"instruction 1, field dst: 1 in an instruction without a destination"),
    ("b in MOV", Bag([ins(MOV, 0, opd(COL, 0), opd(IMM, 0))] + GOOD[1:]), r"instruction 0, field b: 0x3 in an instruction with one operand"),
    ("b in INV0", Bag([ins(INV0, 0, opd(COL, 0), opd(IMM, 1))] + GOOD[1:]), r"instruction 0, field b: 0xb in an instruction with one operand"),
    ("dst >= num_regs", Bag([ins(MOV, 2, opd(COL, 0))] + GOOD[1:]), r"instruction 0, field dst: register 2 is not below num_regs = 2"),
    ("register >= num_regs", Bag([GOOD[0], ins(EMIT, a=opd(REG, 7)), END1]), r"instruction 1, field a: register 7 is not below num_regs = 2"),
    ("read before written", Bag([GOOD[0], ins(ADD, 0, opd(REG, 0), opd(REG, 1)), GOOD[1], END1]),
     r"instruction 1, field b: register 1 is read before it is written"),
    ("pool index", Bag([ins(ADD, 0, opd(COL, 0), opd(IMM, 2))] + GOOD[1:]), r"instruction 0, field b: pool index 2 is not below num_pool = 2"),
    ("COL oracle", Bag([ins(MOV, 0, opd(COL, 1 << 22))] + GOOD[1:]), r"instruction 0, field a: oracle index 1, a unit program's COL has oracle 0"),
    ("COL j", Bag([ins(MOV, 0, opd(COL, 1))] + GOOD[1:]), r"instruction 0, field a: input cell 1 is not below num_inputs = 1"),
    ("COL_NEXT", Bag([ins(MOV, 0, opd(COL_NEXT, 0))] + GOOD[1:]), r"instruction 0, field a: operand kind 2 \(COL_NEXT\) has no meaning in a unit program"),
    ("PARAM", Bag([ins(ADD, 0, opd(COL, 0), opd(PARAM, 0))] + GOOD[1:]), r"instruction 0, field b: operand kind 4 \(PARAM\) has no meaning in a unit program"),
    ("X", Bag([ins(MOV, 0, opd(X))] + GOOD[1:]), r"instruction 0, field a: operand kind 5 \(X\) has no meaning in a unit program"),
    ("operand kind 6", Bag([ins(MOV, 0, opd(6))] + GOOD[1:]), r"instruction 0, field a: unknown operand kind 6"),
    ("BITS b not IMM", Bag([GOOD[0], ins(BITS, 1, opd(REG, 0), opd(REG, 0)), GOOD[1], END1]),
     r"instruction 1, field b: the bit range of BITS is an IMM, not operand kind 0"),
    ("BITS width 0", Bag([ins(BITS, 0, opd(COL, 0), opd(IMM, 1))] + GOOD[1:], pool=(1, 5)), r"instruction 0, field b: the bit range of BITS has width 0 \(lo = 5\)"),
    ("BITS lo + width", Bag([ins(BITS, 0, opd(COL, 0), opd(IMM, 1))] + GOOD[1:], pool=(1, 33 + 256 * 32)),
     r"instruction 0, field b: the bit range of BITS has lo \+ width = 33 \+ 32, more than 64"),
    ("BITS high bits", Bag([ins(BITS, 0, opd(COL, 0), opd(IMM, 1))] + GOOD[1:], pool=(1, 1 << 16 | 256)),
     r"instruction 0, field b: the bit range 0x10100 of BITS has bits set above bit 15"),
    ("too few EMITs", Bag(GOOD, num_outputs=2), r"desc\.num_outputs = 2, the program has 1 EMITs"),
    ("too many EMITs", Bag([GOOD[0], GOOD[1], GOOD[1], END1]), r"desc\.num_outputs = 1, the program has 2 EMITs"),
    ("last not END", Bag(GOOD[:2]), r"instruction 1, field op: the last instruction is not END"),
    ("END of a register", Bag([GOOD[0], GOOD[1], ins(END, a=opd(REG, 0))]), r"instruction 2, field a: the operand of END is not an IMM with the pool word 1"),
    ("END IMM(5)", Bag([GOOD[0], GOOD[1], ins(END, a=opd(IMM, 1))]), r"instruction 2, field a: the operand of END is not an IMM with the pool word 1"),
    ("second END", Bag([GOOD[0], END1, GOOD[1], END1]), r"instruction 1, field op: END before the last instruction, a unit program has exactly one"),
    ("pool word >= p", Bag(GOOD, pool=(1, P)), r"desc\.pool\[1\] = 0xffffffff00000001 is not a canonical field element"),
    ("no instruction", Bag([]), r"desc\.num_instructions is 0: an empty program"),
    ("too many instructions", Bag([GOOD[0]] * 65536 + GOOD[1:]), r"desc\.num_instructions = 65538 is more than 65536"),
    ("num_regs 0", Bag(GOOD, num_regs=0), r"desc\.num_regs = 0 outside 1\.\.24"),
    ("num_regs 25", Bag(GOOD, num_regs=25), r"desc\.num_regs = 25 outside 1\.\.24"),
    ("num_inputs 0", Bag(GOOD, num_inputs=0), r"desc\.num_inputs = 0 outside 1\.\.4096"),
    ("num_inputs 4097", Bag(GOOD, num_inputs=4097), r"desc\.num_inputs = 4097 outside 1\.\.4096"),
    ("num_outputs 0", Bag(GOOD, num_outputs=0), r"desc\.num_outputs = 0 outside 1\.\.4096"),
    ("num_outputs 4097", Bag(GOOD, num_outputs=4097), r"desc\.num_outputs = 4097 outside 1\.\.4096"),
]


@pytest.mark.parametrize("name,bag,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(name, bag, message):
    with pytest.raises(glp.GlpError, match=r"^.*glp_witness_program_check: " + message) as e:
        glp.witness_program_check(bag)
    assert e.value.code == -1                      # GLP_ERR_ARG


def test_null_pointers_are_named():
    with pytest.raises(glp.GlpError, match=r"desc\.code is null"):
        glp.witness_program_check(Bag(GOOD), code=None)
    with pytest.raises(glp.GlpError, match=r"desc\.pool is null with num_pool = 2"):
        glp.witness_program_check(Bag(GOOD), pool=None)


def test_the_gate_program_check_still_refuses_the_new_opcodes():
    from plonky2_lib_amd import gate_program as gp

    class G:
        code, pool, num_regs, num_params, oracle_cols = np.array([ins(INV0, 0, opd(COL, 0)), END1], np.uint64), np.array([1], np.uint64), 1, 0, [1]
    with pytest.raises(glp.GlpError, match=r"instruction 0, field op: .* unknown opcode 7"):
        glp.gate_program_check(G)
    assert gp.OP_END == 6


def _run(prog, values):
    return wpr.run_program(prog.code, prog.pool, values)


@pytest.mark.parametrize("v", EDGE)
def test_wire_split(v):
    assert _run(wprog.wire_split([63, 63]), [v]) == [v & (2 ** 63 - 1), v >> 63]                  # split_le(x, 64) at 80 routed wires
    assert _run(wprog.wire_split([16] * 5), [v]) == [(v >> 16 * i) & 0xFFFF for i in range(4)] + [0]
    assert _run(wprog.wire_split([1, 31, 32]), [v]) == [v & 1, (v >> 1) & (2 ** 31 - 1), v >> 32]
    assert _run(wprog.wire_split([60, 10]), [v]) == [v & (2 ** 60 - 1), v >> 60]


@pytest.mark.parametrize("v", EDGE)
def test_low_high(v):
    assert _run(wprog.low_high(32, 64), [v]) == [v & 0xFFFFFFFF, v >> 32]
    assert _run(wprog.low_high(7, 20), [v]) == [v & 127, (v >> 7) & (2 ** 13 - 1)]
    assert _run(wprog.low_high(63, 64), [v]) == [v & (2 ** 63 - 1), v >> 63]


@pytest.mark.parametrize("x", EDGE)
@pytest.mark.parametrize("y", EDGE)
def test_equality(x, y):
    d = (x - y) % P
    equal, inv = _run(wprog.equality(), [x, y])
    assert equal == (1 if x == y else 0) and inv == (pow(d, P - 2, P) if d else 0) and d * inv % P == 1 - equal


@pytest.mark.parametrize("lo,width", [(0, 64), (63, 1), (0, 1), (31, 2)])
def test_bits(lo, width):
    asm = wprog.Assembler(1)
    asm.emit(asm.bits(asm.reg(), asm.input(0), lo, width))
    prog = asm.assemble()
    glp.witness_program_check(prog)
    assert int(prog.pool[prog.instructions[0].b.index]) == lo + 256 * width
    for v in EDGE + [0x8000000180000001, 0xFFFFFFFE7FFFFFFF]:
        assert _run(prog, [v]) == [(v >> lo) & (2 ** width - 1)]
    for bad in ((0, 0), (64, 1), (1, 64), (-1, 2)):
        with pytest.raises(wprog.AssemblerError):
            asm.bits(asm.reg(), asm.input(0), *bad)


def test_lt():
    asm = wprog.Assembler(2)
    asm.emit(asm.lt(asm.reg(), asm.input(0), asm.input(1)))
    asm.emit(asm.lt(asm.reg(), asm.input(0), asm.imm(2 ** 32)))
    prog = asm.assemble()
    glp.witness_program_check(prog)
    for a in EDGE:
        assert _run(prog, [a, a]) == [0, 1 if a < 2 ** 32 else 0]                # equal operands
        for b in EDGE:
            assert _run(prog, [a, b])[0] == (1 if a < b else 0)
    assert _run(prog, [P - 1, 0])[0] == 0 and _run(prog, [0, P - 1])[0] == 1     # integers, not residues: p - 1 is not -1


def test_the_assembler_refuses_what_a_unit_program_has_not():
    asm = wprog.Assembler(2)
    with pytest.raises(wprog.AssemblerError):
        asm.input(2)
    with pytest.raises(wprog.AssemblerError):
        asm.col_next(0, 0)
    with pytest.raises(wprog.AssemblerError):
        asm.param(0)
    with pytest.raises(wprog.AssemblerError):
        asm.end(asm.imm(2))
    with pytest.raises(wprog.AssemblerError):
        wprog.Assembler(1).assemble()              # no EMIT
    with pytest.raises(wprog.AssemblerError):
        wprog.Assembler(0)


def test_split_le_records_its_wire_split_generator():
    from plonky2_lib_amd import gadgets
    gb = gadgets.GadgetBuilder()
    x = gb.target(2 ** 63 + 12345)
    gb.witness_input_targets.append(x)
    gb._place(x, gb._slot(("arith", 1, 1), gadgets.GATE_ARITHMETIC, gb.n_arith, 0, gb.n_arith, consts=(1, 1))[0], 0)
    bits = gb.split_le(x, 64)
    assert [gb.val[b] for b in bits] == [(gb.val[x] >> i) & 1 for i in range(64)]
    gb.split_le(x, 64)
    c = gb.build()
    assert len(c.witness_programs) == 1 and c.free_units.shape == (2, 9)         # one program, named twice
    assert [list(r[:2]) + list(r[3:]) for r in c.free_units] == [[9, 0, 1, 2, 0, 0, 0, 0]] * 2
    free = wpr.from_arrays(c.free_units, c.free_cells, c.moduli, c.witness_programs)
    flat = c.wires.reshape(-1)
    for f in free:
        assert f.ins == [int(c.witness_inputs[0])]
        assert wpr.run_program(f.code, f.pool, flat[f.ins]) == [int(v) for v in flat[f.outs]] == [12345, 1]


LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "glp.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(glp_witness_program_desc), offsetof(glp_witness_program_desc, code),
           offsetof(glp_witness_program_desc, num_instructions), offsetof(glp_witness_program_desc, pool), offsetof(glp_witness_program_desc, num_pool),
           offsetof(glp_witness_program_desc, num_regs), offsetof(glp_witness_program_desc, num_inputs), offsetof(glp_witness_program_desc, num_outputs));
    printf("%u %u %u %u %u %llu\n", GLP_WP_OP_INV0, GLP_WP_OP_BITS, GLP_WP_OP_LT, GLP_WP_MAX_CELLS, GLP_WGEN_PROGRAM, (unsigned long long)GLP_WP_BITS_RANGE(31, 2));
    return 0;
}
"""


def test_struct_layout_and_constants(tmp_path):
    """include/glp.h against the binding's mirror and the assembler's constants, from a C99 program that prints the header's own"""
    import ctypes as C
    import os
    import subprocess
    from plonky2_lib_amd import binding, gadgets
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(here, "include"), str(src), "-o", str(exe)])
    desc, consts = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    D = binding._WitnessProgramDesc
    assert desc == [C.sizeof(D)] + [getattr(D, f).offset for f, _ in D._fields_]
    assert consts == [wprog.OP_INV0, wprog.OP_BITS, wprog.OP_LT, wprog.MAX_CELLS, wprog.WGEN_PROGRAM, wprog.bits_range(31, 2)] == [7, 8, 9, 4096, 9, 31 + 512]
    assert binding.WGEN_PROGRAM == gadgets.WGEN_PROGRAM == wpr.PROGRAM == 9
    declared = glp.exported_symbols()
    assert "glp_witness_program_check" in declared and "glp_witness_plan_create_prog" in declared
    assert len(glp.load_library().glp_witness_plan_create_prog.argtypes) == 13
