"""Unit programs (include/glp.h, "witness generation, the dataflow half", UNIT PROGRAMS): the host side, no GPU and no library needed.

A unit program states a generator the library does not know as a straight-line program in the gate-program instruction word; the
planner runs it as a free unit of kind WGEN_PROGRAM.  The assembler is gate_program.Assembler (virtual registers, linear scan, the
pool) with the operand `input(j)` in place of the oracle columns, the three opcodes a generator needs beyond field arithmetic, and the
END a unit program must close with:

    asm = Assembler(num_inputs=2)
    d = asm.sub(asm.reg(), asm.input(0), asm.input(1))
    asm.emit(asm.inv0(asm.reg(), d))
    prog = asm.assemble()                  # .code, .pool, .num_regs, .num_inputs, .num_outputs

Ready-made: wire_split (plonky2's WireSplitGenerator), low_high (LowHighGenerator), equality (EqualityGenerator).
"""
import numpy as np

from . import gate_program as gp
from .gate_program import AssemblerError, Instruction, Operand, P       # noqa: F401  (re-exported)

OP_INV0, OP_BITS, OP_LT = 7, 8, 9          # GLP_WP_OP_*
OP_NAMES = {**gp.OP_NAMES, OP_INV0: "INV0", OP_BITS: "BITS", OP_LT: "LT"}
MAX_CELLS = 4096                           # GLP_WP_MAX_CELLS
WGEN_PROGRAM = 9                           # GLP_WGEN_PROGRAM


def bits_range(lo, width):
    """the pool word of a BITS instruction (GLP_WP_BITS_RANGE)"""
    return int(lo) + 256 * int(width)


class WitnessProgram:
    """An assembled unit program: what glp_witness_program_desc points at."""

    def __init__(self, prog, num_inputs):
        self.instructions, self.code, self.pool, self.num_regs, self.max_live = prog.instructions, prog.code, prog.pool, prog.num_regs, prog.max_live
        self.num_inputs = int(num_inputs)
        self.num_outputs = sum(1 for i in prog.instructions if i.op == gp.OP_EMIT)

    def __len__(self):
        return len(self.instructions)


class Assembler(gp.Assembler):
    def __init__(self, num_inputs):
        if not 1 <= int(num_inputs) <= MAX_CELLS:
            raise AssemblerError("1..%d input cells, not %d" % (MAX_CELLS, num_inputs))
        super().__init__([int(num_inputs)])
        self.num_inputs = int(num_inputs)

    def input(self, j):
        """the canonical value of the unit's j-th input cell"""
        return self.col(0, j)

    def col_next(self, oracle, col):
        raise AssemblerError("a unit program has no COL_NEXT")

    def param(self, j):
        raise AssemblerError("a unit program has no PARAM")

    def inv0(self, dst, a):
        return self._push(OP_INV0, dst, a, None)

    def bits(self, dst, a, lo, width):
        if width < 1 or lo < 0 or lo + width > 64:
            raise AssemblerError("BITS: lo = %d, width = %d is no range of a 64-bit word" % (lo, width))
        return self._push(OP_BITS, dst, a, self.imm(bits_range(lo, width)))

    def lt(self, dst, a, b):
        return self._push(OP_LT, dst, a, b)

    def end(self, a=None):
        if a is not None and (a.kind != gp.IMM or self.imm_value(a) != 1):
            raise AssemblerError("a unit program ends with END IMM(1)")
        super().end(self.imm(1))

    def assemble(self, hoist_emits=False):
        if not self._ins or self._ins[-1].op != gp.OP_END:
            self.end()
        if sum(1 for i in self._ins if i.op == gp.OP_END) != 1:
            raise AssemblerError("a unit program has exactly one END")
        prog = WitnessProgram(super().assemble(hoist_emits), self.num_inputs)
        if not 1 <= prog.num_outputs <= MAX_CELLS:
            raise AssemblerError("1..%d EMITs, not %d" % (MAX_CELLS, prog.num_outputs))
        return prog


def wire_split(widths):
    """plonky2's WireSplitGenerator as split_le places it: one input, one output per width; output k holds the bits of the input's
    canonical integer that start at widths[0] + ... + widths[k-1], widths[k] of them.  A range that leaves the 64-bit word is cut at
    bit 64, and one that starts there is the constant 0."""
    asm = Assembler(1)
    lo = 0
    for w in widths:
        if w < 1:
            raise AssemblerError("a width of %d" % w)
        if lo >= 64:
            asm.emit(asm.imm(0))
        else:
            asm.emit(asm.bits(asm.reg(), asm.input(0), lo, min(int(w), 64 - lo)))
        lo += int(w)
    return asm.assemble()


def low_high(n_log, bits):
    """plonky2's LowHighGenerator: one input of at most `bits` bits -> low = its n_log low bits, high = the rest"""
    if not 0 < n_log < bits <= 64:
        raise AssemblerError("low_high: 0 < n_log < bits <= 64, not %d, %d" % (n_log, bits))
    asm = Assembler(1)
    asm.emit(asm.bits(asm.reg(), asm.input(0), 0, n_log))
    asm.emit(asm.bits(asm.reg(), asm.input(0), n_log, bits - n_log))
    return asm.assemble()


def equality():
    """plonky2's EqualityGenerator, the outputs of WGEN_EQUALITY: in x, y -> equal = (x == y), inv = 1 / (x - y) or 0"""
    asm = Assembler(2)
    d = asm.sub(asm.reg(), asm.input(0), asm.input(1))
    inv = asm.inv0(asm.reg(), d)
    asm.emit(asm.sub(asm.reg(), asm.imm(1), asm.mul(asm.reg(), d, inv)))
    asm.emit(inv)
    return asm.assemble()


def units_array(units):
    """[(program index, [input cells], [output cells])] -> (int64 [num][9] rows of kind, modulus, cell_begin, len[6]; uint64 cells):
    the free_units pair of Circuit.witness_plan"""
    rows, cells = [], []
    for prog, ins, outs in units:
        rows.append([WGEN_PROGRAM, int(prog), len(cells), len(ins), len(outs), 0, 0, 0, 0])
        cells += [int(c) for c in ins] + [int(c) for c in outs]
    return np.array(rows, np.int64).reshape(-1, 9), np.array(cells, np.uint64)
