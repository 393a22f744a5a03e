"""Free units of witness generation restated on the CPU (include/glp.h, "witness generation, the dataflow half", FREE UNITS): the
generators that belong to no gate, as Python integers, and the planner rule and generation of tests/witness_plan_restate.py extended by
them.  Nothing here shares code with csrc/.

A free unit is (kind, modulus index, operand lengths len[6], cell run): the run lists the input cells, then the output cells, limbs
little-endian, in the operand order of its kind:
  EQUALITY 1            in x, y                        out equal, inv              field arithmetic (plonky2's EqualityGenerator, recalled)
  NONNATIVE_ADD 2       in a, b                        out sum, overflow (1 cell)  [REF src/ecdsa/gadgets/nonnative.rs:475-490]
  NONNATIVE_MULTI_ADD 3 in len[0] summands of len[1]   out sum, overflow (1 cell)  [REF :553-576]
  NONNATIVE_SUB 4       in a, b                        out diff, overflow (1 cell) [REF :648-663]
  NONNATIVE_MUL 5       in a, b                        out prod, overflow (limbs)  [REF :727-740]
  NONNATIVE_INV 6       in x                           out inv, div                [REF :797-809]
  BIGUINT_DIV_REM 7     in a, b                        out div, rem                [REF src/ecdsa/gadgets/biguint.rs:342-349]
  GLV_SECP256K1 8       in k (8)                       out k1, k2 (4 each), k1_neg, k2_neg   [REF src/ecdsa/curve/glv.rs:38-77]
The nonnative kinds reduce every operand modulo m first.  Addition overflows when a + b > m, strictly.  Outside a generator's domain: a
cell >= 2^32 is read as its low 32 bits, a zero divisor gives div = rem = 0, x = 0 or gcd(x, m) != 1 gives inv = div = 0, a result wider
than its cells is truncated, an empty quotient gives overflow 0.  An output cell NO_CELL is not written.

The rule: a free unit reads the classes of its input cells and is the writer of its output cells; its wave is 1 + the maximum wave of
the classes it reads; it is stuck as a gate unit is; class wave, source, copies and cell_waves treat a free writer like a gate writer;
in a wave gate units and free units run before the copies.  The plan's info counts gate units only, except num_waves: the highest wave
that holds any unit; free_info counts the free units.
"""
from math import gcd

import numpy as np

import witness_fill_restate as wfr
import witness_plan_restate as wp

P = 2 ** 64 - 2 ** 32 + 1
M32 = 2 ** 32 - 1
NO_CELL = 2 ** 64 - 1
EQUALITY, ADD, MULTI_ADD, SUB, MUL, INV, DIV_REM, GLV = range(1, 9)
MAX_LIMBS = 18

FN = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
_w = lambda ws: sum(int(w) << (64 * i) for i, w in enumerate(ws))
A1 = B2 = _w([16747920425669159701, 3496713202691238861])          # [REF src/ecdsa/curve/glv.rs:25-32]
MINUS_B1 = _w([8022177200260244675, 16448129721693014056])
A2 = _w([6323353552219852760, 1498098850674701302, 1])


def num_in(kind, ln):
    return ln[0] * ln[1] if kind == MULTI_ADD else ln[0] if kind in (INV, GLV) else ln[0] + ln[1]


def num_out(kind, ln):
    return ln[1] + ln[2] if kind == INV else ln[1] + ln[2] + ln[3] + ln[4] if kind == GLV else ln[2] + ln[3]


def _big(cells):
    return sum((int(c) & M32) << (32 * i) for i, c in enumerate(cells))


def _limbs(v, n):
    return [(v >> (32 * i)) & M32 for i in range(n)]


def glv_decompose(k):
    """decompose_secp256k1_scalar: Ratio::round is half away from zero, and n is odd"""
    rnd = lambda a: a // FN + (1 if 2 * (a % FN) > FN else 0)
    c1, c2 = rnd(B2 * k) % FN, rnd(MINUS_B1 * k) % FN
    k1 = (k - c1 * A1 - c2 * A2) % FN
    k2 = (c1 * MINUS_B1 - c2 * B2) % FN
    n1, n2 = k1 > FN // 2, k2 > FN // 2
    return (FN - k1 if n1 else k1), (FN - k2 if n2 else k2), int(n1), int(n2)


def run_free(kind, ln, m, ins):
    """the output cells of one free unit, in run order, from its input cells (field elements)"""
    ins = [int(v) for v in ins]
    assert len(ins) == num_in(kind, ln)
    if kind == EQUALITY:
        d = (ins[0] - ins[1]) % P
        return [1 if d == 0 else 0, pow(d, P - 2, P) if d else 0]
    if kind in (ADD, SUB, MUL):
        a, b = _big(ins[:ln[0]]) % m, _big(ins[ln[0]:]) % m
        if kind == ADD:
            s = a + b
            over = s > m
            return _limbs(s - m if over else s, ln[2]) + [int(over)]
        if kind == SUB:
            return _limbs(a - b if a >= b else m + a - b, ln[2]) + [int(a < b)]
        return _limbs(a * b % m, ln[2]) + _limbs(a * b // m, ln[3])
    if kind == MULTI_ADD:
        s = sum(_big(ins[i * ln[1]:(i + 1) * ln[1]]) % m for i in range(ln[0]))
        return _limbs(s % m, ln[2]) + [(s // m) & M32]
    if kind == INV:
        x = _big(ins) % m
        inv = pow(x, -1, m) if x and gcd(x, m) == 1 else 0
        return _limbs(inv, ln[1]) + _limbs(x * inv // m, ln[2])
    if kind == DIV_REM:
        a, b = _big(ins[:ln[0]]), _big(ins[ln[0]:])
        q, r = (a // b, a % b) if b else (0, 0)
        return _limbs(q, ln[2]) + _limbs(r, ln[3])
    if kind == GLV:
        k1, k2, n1, n2 = glv_decompose(_big(ins) % FN)
        return _limbs(k1, ln[1]) + _limbs(k2, ln[2]) + [n1, n2]
    raise ValueError("kind %r" % (kind,))


class Free:
    """one free unit: kind, modulus (the integer, or 0), len[6], input cells, output cells (NO_CELL = not placed)"""

    def __init__(self, kind, modulus, ln, ins, outs):
        self.kind, self.modulus, self.len, self.ins, self.outs = int(kind), int(modulus), [int(x) for x in ln], [int(c) for c in ins], [int(c) for c in outs]
        assert len(self.ins) == num_in(self.kind, self.len) and len(self.outs) == num_out(self.kind, self.len)


def from_arrays(free_units, free_cells, moduli):
    """the C layout (uint32 [num][9]: kind, modulus, cell_begin, len[6]; uint64 cells; uint32 moduli [num][8]) -> [Free]"""
    out = []
    for rec in np.asarray(free_units, np.int64).reshape(-1, 9):
        kind, mi, cb, ln = int(rec[0]), int(rec[1]), int(rec[2]), [int(x) for x in rec[3:]]
        ni, no = num_in(kind, ln), num_out(kind, ln)
        m = sum(int(v) << (32 * i) for i, v in enumerate(np.asarray(moduli).reshape(-1, 8)[mi])) if kind in (ADD, MULTI_ADD, SUB, MUL, INV) else 0
        out.append(Free(kind, m, ln, free_cells[cb:cb + ni], free_cells[cb + ni:cb + ni + no]))
    return out


def plan(desc, input_cells, free, cls=None, withhold=()):
    """wp.plan with free units; `withhold`: indices into `free` of units that are left out (they and everything downstream are then
    reported stuck: the withheld unit itself is not a unit of the plan, so the stuck ones are its readers)."""
    n, nw = 1 << int(desc.degree_bits), int(desc.num_wires)
    cls = wp.classes(desc) if cls is None else cls
    gate_units = wp.all_units(desc)
    ng = len(gate_units)
    free = [f for i, f in enumerate(free) if i not in set(withhold)]
    us = [(u[3], u[4]) for u in gate_units] + [(f.ins, [c for c in f.outs if c != NO_CELL]) for f in free]
    inputs = [int(p) for p in input_cells]
    assert len(set(inputs)) == len(inputs) and len({int(cls[p]) for p in inputs}) == len(inputs)
    class_wave = {int(cls[p]): 0 for p in inputs}
    readers, pending = {}, []
    for k, (ins, _) in enumerate(us):
        need = {int(cls[p]) for p in ins if int(cls[p]) not in class_wave}
        pending.append(len(need))
        for c in need:
            readers.setdefault(c, []).append(k)
    unit_wave = [-1] * len(us)
    ready = [k for k in range(len(us)) if pending[k] == 0]
    w = 0
    while ready:
        w += 1
        nxt = []
        for k in ready:
            unit_wave[k] = w
        for k in ready:
            for p in us[k][1]:
                c = int(cls[p])
                if c not in class_wave:
                    class_wave[c] = w
                    for r in readers.get(c, ()):
                        pending[r] -= 1
                        if pending[r] == 0:
                            nxt.append(r)
        ready = nxt
    pl = wp.Plan()
    pl.desc, pl.cls, pl.units, pl.free, pl.unit_wave, pl.inputs, pl.class_wave = desc, cls, gate_units, free, unit_wave, inputs, class_wave
    pl.num_waves = w
    cw = np.full(nw * n, -1, np.int64)
    known = np.array(sorted(class_wave), np.int64)
    lut = np.full(nw * n, -1, np.int64)
    lut[known] = [class_wave[int(c)] for c in known]
    cw[:] = lut[np.asarray(cls, np.int64)]
    writer = {}
    for k, (_, outs) in enumerate(us):
        for p in outs:
            assert p not in writer, "two units write one cell"
            writer[p] = k
            if unit_wave[k] >= 0:
                cw[p] = unit_wave[k]
    pl.cell_waves = cw.reshape(nw, n)
    members = {}
    for p in np.nonzero(lut[np.asarray(cls, np.int64)] >= 0)[0]:
        members.setdefault(int(cls[p]), []).append(int(p))
    inset = set(inputs)
    pl.copies = {}
    for c, ms in members.items():
        cwv = class_wave[c]
        src = min(p for p in ms if (cwv == 0 and p in inset) or (p in writer and unit_wave[writer[p]] == cwv))
        for p in ms:
            if p != src:
                pl.copies.setdefault(cwv, []).append((src, p))
    stuck = [k for k in range(ng) if unit_wave[k] < 0]
    fstuck = [k - ng for k in range(ng, len(us)) if unit_wave[k] < 0]
    per_wave = np.bincount([x for x in unit_wave[:ng] if x > 0], minlength=w + 1)
    fper_wave = np.bincount([x for x in unit_wave[ng:] if x > 0], minlength=w + 1)
    g = gate_units
    pl.info = dict(num_waves=w, num_units=ng, num_stuck_units=len(stuck), num_copies=sum(len(v) for v in pl.copies.values()),
                   num_cells_known=int((cw >= 0).sum()), widest_wave_units=int(per_wave.max()),
                   stuck_row=g[stuck[0]][0] if stuck else None, stuck_gate=g[stuck[0]][1] if stuck else None,
                   stuck_unit=g[stuck[0]][2] if stuck else None)
    pl.free_info = dict(num_free_units=len(free), num_stuck_free_units=len(fstuck), first_stuck_free_unit=fstuck[0] if fstuck else None,
                        widest_wave_free_units=int(fper_wave.max()))
    pl.stuck = [(g[k][0], g[k][1], g[k][2]) for k in stuck]
    pl.stuck_free = fstuck
    return pl


def generate(pl, input_values, start):
    """glp_witness_generate on a copy of `start` [num_wires][n]"""
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
            else:
                f = pl.free[k - ng]
                vals = run_free(f.kind, f.len, f.modulus, [flat[c] for c in f.ins])
                puts += [(c, v) for c, v in zip(f.outs, vals) if c != NO_CELL]
        for p, val in puts:                       # every unit of a wave reads the witness as the wave found it
            flat[p] = val
        for src, dst in pl.copies.get(w, ()):
            flat[dst] = flat[src]
    return W
