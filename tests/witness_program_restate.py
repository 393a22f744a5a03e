"""Unit programs of witness generation restated on the CPU (include/glp.h, "witness generation, the dataflow half", UNIT PROGRAMS):
an interpreter of the instruction word over Python integers, glued to the planner and the free units of tests/witness_plan_restate.py
and tests/witness_free_restate.py.  Nothing here shares code with csrc/ or with the package's assembler: the word is decoded from its
bit layout as the header states it.

    bits 3..0 opcode | bits 8..4 dst | bits 35..9 operand a | bits 62..36 operand b | bit 63 zero
    operand: kind in bits 2..0 (0 REG, 1 COL = input cell j, 3 IMM = pool word j), payload in bits 26..3
    1 ADD  2 SUB  3 MUL  4 MOV  5 EMIT (output cell number = EMITs so far)  6 END
    7 INV0 (1 / a, 0 for 0)  8 BITS (b: pool word lo + 256 width; (a >> lo) & (2^width - 1))  9 LT (1 if a < b as integers)

A program unit is a free unit of kind 9: it reads the classes of its input cells, writes its output cells (NO_CELL: not written) and
takes its wave, or is stuck, by the one rule of witness_free_restate.plan, which only looks at a unit's cells.
"""
import numpy as np

import witness_fill_restate as wfr
import witness_free_restate as fr

P = fr.P
NO_CELL = fr.NO_CELL
PROGRAM = 9
EDGE_VALUES = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, P - 1]


def run_program(code, pool, ins):
    """the values a unit EMITs, in order, from its input cells"""
    pool = [int(v) for v in pool]
    ins = [int(v) for v in ins]
    regs, out = {}, []

    def operand(f):
        kind, pl = f & 7, f >> 3
        if kind == 0:
            return regs[pl]
        if kind == 1:
            assert pl >> 22 == 0
            return ins[pl]
        assert kind == 3, "operand kind %d" % kind
        return pool[pl]
    for n, word in enumerate(int(w) for w in code):
        op, dst, fa, fb = word & 15, (word >> 4) & 31, (word >> 9) & (2 ** 27 - 1), (word >> 36) & (2 ** 27 - 1)
        assert word >> 63 == 0
        if op == 6:
            assert n == len(code) - 1 and operand(fa) == 1 and fa & 7 == 3
            break
        a = operand(fa)
        if op == 5:
            out.append(a)
        elif op == 1:
            regs[dst] = (a + operand(fb)) % P
        elif op == 2:
            regs[dst] = (a - operand(fb)) % P
        elif op == 3:
            regs[dst] = a * operand(fb) % P
        elif op == 4:
            regs[dst] = a
        elif op == 7:
            regs[dst] = pow(a, P - 2, P) if a else 0
        elif op == 8:
            assert fb & 7 == 3
            lo, width = pool[fb >> 3] & 255, pool[fb >> 3] >> 8
            assert width >= 1 and lo + width <= 64
            regs[dst] = (a >> lo) & (2 ** width - 1)
        elif op == 9:
            regs[dst] = 1 if a < operand(fb) else 0
        else:
            raise AssertionError("opcode %d" % op)
    assert all(0 <= v < P for v in out)
    return out


class Prog:
    """one program unit: its program's words and pool, input cells, output cells (NO_CELL = not written)"""
    kind = PROGRAM

    def __init__(self, code, pool, ins, outs):
        self.code, self.pool, self.ins, self.outs = [int(w) for w in code], [int(w) for w in pool], [int(c) for c in ins], [int(c) for c in outs]


def from_arrays(free_units, free_cells, moduli, programs):
    """the C layout of Circuit.witness_plan -> [Free or Prog], in the caller's order"""
    out = []
    for rec in np.asarray(free_units, np.int64).reshape(-1, 9):
        if int(rec[0]) != PROGRAM:
            out += fr.from_arrays(rec.reshape(1, 9), free_cells, moduli)
            continue
        pr, cb, ni, no = programs[int(rec[1])], int(rec[2]), int(rec[3]), int(rec[4])
        assert ni == pr.num_inputs and no == pr.num_outputs and not rec[5:].any()
        out.append(Prog(pr.code, pr.pool, free_cells[cb:cb + ni], free_cells[cb + ni:cb + ni + no]))
    return out


plan = fr.plan            # the rule reads a unit's .ins and .outs only


def generate(pl, input_values, start):
    """glp_witness_generate on a copy of `start` [num_wires][n]: witness_free_restate.generate with program units"""
    desc = pl.desc
    n, nsel = 1 << int(desc.degree_bits), int(desc.num_selectors)
    ng = len(pl.units)
    W = np.array(start, np.uint64).copy()
    flat = W.reshape(-1)
    for p, v in zip(pl.inputs, input_values):
        flat[p] = int(v)
    by_wave = {}
    for k, wv in enumerate(pl.unit_wave):
        if wv > 0:
            by_wave.setdefault(wv, []).append(k)
    for w in range(0, pl.num_waves + 1):
        puts = []
        for k in by_wave.get(w, ()):
            if k < ng:
                r, gi, u, _, outs = pl.units[k]
                keep = {p // n for p in outs}
                row = [int(v) for v in W[:, r]]
                gc = [int(v) for v in desc.constants[nsel:, r]]
                wfr.fill_row(desc.gates[gi], gc, row, lambda col, val, r=r, keep=keep: puts.append((col * n + r, val)) if col in keep else None)
                continue
            f = pl.free[k - ng]
            if f.kind == PROGRAM:
                vals = run_program(f.code, f.pool, [flat[c] for c in f.ins])
                assert len(vals) == len(f.outs)
            else:
                vals = fr.run_free(f.kind, f.len, f.modulus, [flat[c] for c in f.ins])
            puts += [(c, v) for c, v in zip(f.outs, vals) if c != NO_CELL]
        for p, val in puts:                       # every unit of a wave reads the witness as the wave found it
            flat[p] = val
        for src, dst in pl.copies.get(w, ()):
            flat[dst] = flat[src]
    return W


def program_waves(pl):
    """the waves that hold a program unit"""
    ng = len(pl.units)
    return sorted({pl.unit_wave[ng + i] for i, f in enumerate(pl.free) if f.kind == PROGRAM and pl.unit_wave[ng + i] > 0})
