"""The free units that tests/test_gpu_biguint_device.py runs on the GPU, and tests/test_biguint_device_vectors.py runs first through the
host program (csrc/examples/biguint_host.cpp --per-unit) to show that they reach the rare branches of csrc/biguint_dev.h in both of its
instances: the one with every count a compile-time 8 (`all8`) and the general-length one (`any`).

The vectors are grouped by SHAPE -- kind, modulus, len[6] -- and every shape has K value sets, so that the whole set is K proofs in
lock step over one plan in which each shape is one free unit.  A shape also says which of its output cells are not placed
(GLP_WGEN_NO_CELL).  Limbs are drawn from SPECIAL with probability 0.8 and at random otherwise; the named edges of every kind are the
first value sets of its shapes.  Expected outputs are witness_free_restate.run_free: Python integers.

What is here that the gadget builders never emit:
  all8     8-limb odd moduli whose top limb is 1, 2, 0x10000, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF (the normalisation shift of
           the division is 31, 30, 15, 1, 0, 0, 0), both secp256k1 moduli and two composite moduli 3 q; operands below the modulus and
           unreduced ones: all-ones limbs, m, m + 1, 2 m - 1, 2^256 - 1
  any      moduli of 1 .. 7 limbs, and 8-limb moduli in units that miss the all8 shape by one length; operands of 0, 1, nm - 1, nm,
           nm + 1, 17 and 18 limbs; results of 0 .. 18 cells, truncated and zero-padded; MULTI_ADD of 0, 1, 3 and 17 summands; DIV_REM with a
           divisor of 0, with zero top limbs, longer than the dividend, 18 by 8 limbs, and the classic correction cases; GLV either side
           of the sign flips and with k >= n
  both     cells that carry bits above bit 31 (below p: only the low 32 bits are the limb); x = 0 and gcd(x, m) != 1 for the inverse"""
import functools

import numpy as np

import witness_free_restate as fr

K = 32                                    # value sets per shape = proofs in lock step
SEED = 5
FP = 2 ** 256 - 2 ** 32 - 977
FN = fr.FN
ONES = 2 ** 256 - 1
SPECIAL = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF]
TOPS = [1, 2, 0x10000, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF]
MODULI_PER_TOP = 4
NO_CELL = fr.NO_CELL
HAS_MODULUS = (fr.ADD, fr.MULTI_ADD, fr.SUB, fr.MUL, fr.INV)


def limbs(v, n):
    """the integer v as n little-endian u32 limbs, truncated"""
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def num_limbs(m):
    return (m.bit_length() + 31) // 32


def shift_of(m):
    """the division's normalisation shift for the divisor m: the leading zeros of its top limb"""
    return 32 * num_limbs(m) - m.bit_length()


def is_all8(kind, ln, m):
    """big::all8, restated"""
    if num_limbs(m) != 8 or ln[:3] != [8, 8, 8]:
        return False
    return kind == fr.INV or (kind == fr.MUL and ln[3] == 8) or (kind in (fr.ADD, fr.SUB) and ln[3] == 1)


class Shape:
    """one free unit of the plan: kind, modulus (the integer; 0 for the kinds without), len[6], K lists of input cell values, and the
    indices of the output cells that are not placed"""

    def __init__(self, kind, modulus, ln, sets, name):
        self.kind, self.modulus, self.len, self.sets, self.name, self.unplaced = kind, modulus, list(ln), sets, name, frozenset()
        assert len(sets) == K and all(len(s) == fr.num_in(kind, self.len) for s in sets), name
        self.all8 = kind in HAS_MODULUS and is_all8(kind, self.len, modulus)

    def __repr__(self):
        return "%s: kind %d, len %s, modulus %#x (%d limbs, shift %d), %s instance" % (
            self.name, self.kind, self.len, self.modulus, num_limbs(self.modulus), shift_of(self.modulus) if self.modulus else 0, "all8" if self.all8 else "any")


class _Draw:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def int(self, lo, hi):
        return int(self.rng.integers(lo, hi))

    def limbs(self, n):
        return [SPECIAL[self.int(0, len(SPECIAL))] if self.rng.random() < 0.8 else self.int(0, 1 << 32) for _ in range(n)]

    def modulus(self, nm, top):
        m = self.limbs(nm - 1) + [top]
        m[0] |= 1
        return fr._big(m)

    def operand(self, n, m):
        """n limbs; every other one is cut down below m, when it is long enough to exceed it"""
        v = self.limbs(n)
        if self.int(0, 2) and n >= num_limbs(m):
            v = limbs(fr._big(v) & ((1 << (m.bit_length() - 1)) - 1), n)
        return v


def _fill(d, named, draw):
    sets = [list(s) for s in named[:K]]
    while len(sets) < K:
        sets.append(draw())
    return sets


def _all8_shapes(d):
    moduli = [FP, FN, 3 * (FN // 3 | 1), 3 * ((1 << 225) | fr._big(d.limbs(7)) | 1)]                # the last two: composite, shift 0 and shift 29
    moduli += [d.modulus(8, top) for top in TOPS for _ in range(MODULI_PER_TOP)]
    out = []
    for i, m in enumerate(moduli):
        assert num_limbs(m) == 8 and m & 1
        L = lambda v: limbs(v, 8)
        pairs = [(m - 1, m - 1), (ONES, ONES), (m, m + 1), (min(2 * m - 1, ONES), m - 1), (ONES, 1), (m + 1, m), (0, 0), (1, m - 1), (m // 2, m // 2 + 1), (5, 3), (3, 5),
                 (m - 1, 1), (m - 2, 1), (m // 2 + 1, m // 2 + 1)]
        for kind, name in ((fr.ADD, "add"), (fr.SUB, "sub"), (fr.MUL, "mul")):
            sets = _fill(d, [L(a) + L(b) for a, b in pairs], lambda: d.operand(8, m) + d.operand(8, m))
            out.append(Shape(kind, m, [8, 8, 8, 8 if kind == fr.MUL else 1, 0, 0], sets, "all8 %s, modulus %d" % (name, i)))
        xs = [0, 1, m - 1, (m + 1) // 2, m, m + 1, ONES, 2, 3, m - 2, m // 3, 6, min(2 * m - 1, ONES)]
        out.append(Shape(fr.INV, m, [8, 8, 8, 0, 0, 0], _fill(d, [L(x) for x in xs], lambda: d.operand(8, m)), "all8 inv, modulus %d" % i))
    return out, moduli


def _any_modular_shapes(d, moduli8):
    out = []
    small = [3, 0xFFFFFFFB, 0x10001, 15, 3 * 0x2AAAAAAB55555555]                                 # 1 limb; the last two composite: 1 and 2 limbs
    small += [d.modulus(nm, TOPS[(nm * 3) % len(TOPS)]) for nm in range(2, 8)]
    for i, m in enumerate(small):
        nm = num_limbs(m)
        lens = sorted({0, 1, nm - 1, nm, nm + 1, 17, 18})
        for kind, name in ((fr.ADD, "add"), (fr.SUB, "sub"), (fr.MUL, "mul")):
            for j, la in enumerate(lens):
                lb = lens[(j + kind + i) % len(lens)]
                ln = [la, lb, d.int(0, 19), d.int(0, 19) if kind == fr.MUL else 1, 0, 0]
                named = [[0xFFFFFFFF] * (la + lb), limbs(m - 1, la) + limbs(m - 1, lb), limbs(m, la) + limbs(m + 1, lb), limbs(2 * m - 1, la) + limbs(1, lb)]
                out.append(Shape(kind, m, ln, _fill(d, named, lambda: d.operand(la, m) + d.operand(lb, m)), "%s, %d-limb modulus %d" % (name, nm, i)))
        for lx in lens:
            xs = [0, 1, m - 1, (m + 1) // 2, m, m + 1, 3, m // 3, 2, (1 << (32 * lx)) - 1]
            out.append(Shape(fr.INV, m, [lx, d.int(0, 19), d.int(0, 19), 0, 0, 0], _fill(d, [limbs(x, lx) for x in xs], lambda: d.operand(lx, m)),
                             "inv, %d-limb modulus %d" % (nm, i)))
        # the inverse in full: x = 1, m - 1, (m + 1) / 2 fit their cells
        xs = [0, 1, m - 1, (m + 1) // 2, 3, m // 3]
        out.append(Shape(fr.INV, m, [nm, nm, nm, 0, 0, 0], _fill(d, [limbs(x, nm) for x in xs], lambda: d.operand(nm, m)), "inv in full, %d-limb modulus %d" % (nm, i)))
    # 8-limb moduli in units that miss the all8 shape by one length
    near = {fr.ADD: [(7, 8, 8, 1), (8, 9, 8, 1), (8, 8, 7, 1), (8, 8, 9, 1)], fr.SUB: [(9, 8, 8, 1), (8, 7, 8, 1), (8, 8, 7, 1), (8, 8, 9, 1)],
            fr.MUL: [(8, 8, 8, 7), (8, 8, 8, 9), (8, 8, 7, 8), (9, 8, 8, 8), (8, 7, 8, 8)], fr.INV: [(8, 8, 7, 0), (8, 7, 8, 0), (9, 8, 8, 0), (7, 8, 8, 0), (8, 8, 9, 0)]}
    for i, m in enumerate([FP, moduli8[4], moduli8[4 + 2 * MODULI_PER_TOP], moduli8[2]]):             # shifts 0, 31, 15 and the composite
        for kind, lns in near.items():
            for ln in lns:
                ln = list(ln) + [0, 0]
                if kind == fr.INV:
                    named = [limbs(x, ln[0]) for x in (0, 1, m - 1, (m + 1) // 2, m, 3, m // 3, ONES)]
                    draw = lambda: d.operand(ln[0], m)
                else:
                    named = [limbs(a, ln[0]) + limbs(b, ln[1]) for a, b in ((m - 1, m - 1), (ONES, ONES), (m, m + 1), (min(2 * m - 1, ONES), m - 1), (ONES, 1))]
                    draw = lambda: d.operand(ln[0], m) + d.operand(ln[1], m)
                out.append(Shape(kind, m, ln, _fill(d, named, draw), "kind %d one length off all8, 8-limb modulus %d" % (kind, i)))
    # NONNATIVE_MULTI_ADD: 0, 1, 3 and 17 summands
    for i, m in enumerate([FP, small[1], small[7], moduli8[4]]):
        nm = num_limbs(m)
        for cnt in (0, 1, 3, 17):
            for ll in sorted({0, 1, nm, 18}) + ([nm + 1] if cnt == 3 else []):
                named = [[0xFFFFFFFF] * (cnt * ll), limbs(m - 1, ll) * cnt, limbs(m, ll) * cnt]
                out.append(Shape(fr.MULTI_ADD, m, [cnt, ll, nm if cnt != 3 else d.int(0, 19), 1, 0, 0], _fill(d, named, lambda: [v for _ in range(cnt) for v in d.operand(ll, m)]),
                                 "multi_add of %d x %d limbs, %d-limb modulus %d" % (cnt, ll, nm, i)))
    return out


def _div_rem_shapes(d):
    out = []

    def shape(ln, named, name, divisor=None):
        la, lb = ln[0], ln[1]
        out.append(Shape(fr.DIV_REM, 0, list(ln) + [0, 0], _fill(d, named, lambda: d.limbs(la) + (divisor() if divisor else d.limbs(lb))), "div_rem " + name))
    shape((8, 4, 5, 4), [d.limbs(8) + [0, 0, 0, 0], d.limbs(8) + [7, 0, 0, 0], d.limbs(8) + [1, 0, 0, 0], d.limbs(8) + d.limbs(2) + [0, 0], d.limbs(8) + d.limbs(3) + [0]],
          "by 0 and by divisors whose top limbs are 0", divisor=lambda: (d.limbs(d.int(0, 5)) + [0] * 4)[:4])
    shape((18, 8, 11, 8), [[0xFFFFFFFF] * 26, [0xFFFFFFFF] * 18 + [1] + [0] * 7, [0xFFFFFFFF] * 18 + [0] * 7 + [1], [0] * 17 + [1] + [0xFFFFFFFF] * 8], "18 by 8 limbs")
    shape((18, 8, 18, 18), [[0xFFFFFFFF] * 26, [0xFFFFFFFF] * 18 + [0] * 8], "18 by 8 limbs, padded results", divisor=lambda: (d.limbs(d.int(0, 9)) + [0] * 8)[:8])
    shape((2, 6, 0, 6), [], "a dividend shorter than the divisor")
    shape((2, 6, 3, 8), [], "a dividend shorter than the divisor, padded")
    shape((0, 3, 1, 3), [], "an empty dividend")
    shape((5, 0, 5, 2), [], "an empty divisor")
    shape((3, 3, 1, 3), [[3, 0, 0x80000000] + [1, 0, 0x20000000]], "the add-back case")
    shape((4, 3, 2, 3), [[0, 0xFFFE0000, 0x7FFFFFFF, 0x7FFF8000] + [1, 0, 0x80000000]], "the digit-correction case")
    shape((8, 2, 7, 2), [[5, 6, 7, 0, 0, 0, 0, 0] + [9, 1]], "a quotient with zero top limbs")
    shape((4, 1, 2, 1), [[1 << 40, 7, 1 << 63, 9] + [3]], "a truncated quotient")
    for la, lb in ((1, 1), (2, 2), (8, 8), (9, 8), (12, 8), (16, 8), (17, 7), (18, 1), (18, 2), (7, 8), (18, 5), (10, 3)):
        shape((la, lb, d.int(0, 19), d.int(0, 19)), [[0xFFFFFFFF] * (la + lb)], "%d by %d limbs" % (la, lb))
    return out


def glv_scalars(d):
    """0, 1, n - 1, k >= n, values either side of the sign flips of k1 and k2 (found by bisection on the restated decomposition)"""
    ks = [0, 1, 2, FN - 1, FN - 2, FN // 2, FN // 2 + 1, FN, FN + 5, ONES]
    for which in (2, 3):
        found = 0
        while found < 6:
            lo, hi = sorted(fr._big(d.rng.integers(0, 1 << 32, 8)) % FN for _ in range(2))
            if fr.glv_decompose(lo)[which] == fr.glv_decompose(hi)[which]:
                continue
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if fr.glv_decompose(mid)[which] == fr.glv_decompose(lo)[which] else (lo, mid)
            ks += [lo, hi]
            found += 1
    return ks


def _glv_shapes(d):
    ks = glv_scalars(d)
    while len(ks) < 2 * K:
        ks.append(fr._big(d.limbs(8)))
    return [Shape(fr.GLV, 0, [8, 4, 4, 1, 1, 0], [limbs(k, 8) for k in ks[i * K:(i + 1) * K]], "glv %d" % i) for i in range(2)]


@functools.lru_cache(maxsize=None)
def shapes(seed=SEED):
    d = _Draw(seed)
    a8, moduli8 = _all8_shapes(d)
    out = a8 + _any_modular_shapes(d, moduli8) + _div_rem_shapes(d) + _glv_shapes(d)
    for i, sh in enumerate(out):
        # cells >= 2^32, below p = 2^64 - 2^32 + 1: value sets 5, 13, 21 and 29 of every shape; only the low 32 bits are the limb
        for k in range(5, K, 8):
            sh.sets[k] = [v | (d.int(1, 1 << 31) << 32) if d.int(0, 2) else v for v in sh.sets[k]]
        no = fr.num_out(sh.kind, sh.len)
        if no and (i % 3 == 1 or sh.kind == fr.GLV):       # every third unit, and both GLV units, leave one or two of their output cells out
            sh.unplaced = frozenset(d.int(0, no) for _ in range(1 + i % 2))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(seed=SEED):
    """[shape][k] -> the output cells, as Python integers say"""
    return tuple(tuple(fr.run_free(sh.kind, sh.len, sh.modulus, s) for s in sh.sets) for sh in shapes(seed))


def host_lines(shs):
    """the units in the input format of the host program, shape by shape, value set by value set"""
    out = []
    for sh in shs:
        ml = limbs(sh.modulus, num_limbs(sh.modulus)) if sh.kind in HAS_MODULUS else []
        head = [sh.kind, len(ml)] + ml + sh.len
        out += [" ".join("%x" % v for v in head + s) for s in sh.sets]
    return out


def place(shs, num_cells):
    """every shape as one free unit on a run of cells of its own, scattered over a trace of num_cells cells that nothing constrains
    -> (units int64 [num][9], cells uint64, moduli uint32 [num][8], [Free], per shape its input cells, per shape its placed output
    cells as (index in the unit's outputs, cell))"""
    step = 7919                                            # a prime that does not divide num_cells: i -> i * step walks every cell once
    assert np.gcd(step, num_cells) == 1
    pool = iter(range(num_cells))
    take = lambda k: [next(pool) * step % num_cells for _ in range(k)]
    moduli = sorted({sh.modulus for sh in shs if sh.kind in HAS_MODULUS})
    units, cells, free, ins, outs = [], [], [], [], []
    for sh in shs:
        cin, cout = take(fr.num_in(sh.kind, sh.len)), take(fr.num_out(sh.kind, sh.len))        # an unplaced output keeps its cell: nothing may write it
        run = [NO_CELL if i in sh.unplaced else c for i, c in enumerate(cout)]
        units.append([sh.kind, moduli.index(sh.modulus) if sh.kind in HAS_MODULUS else 0, len(cells)] + sh.len)
        cells += cin + run
        free.append(fr.Free(sh.kind, sh.modulus, sh.len, cin, run))
        ins.append(cin)
        outs.append([(i, c) for i, c in enumerate(run) if c != NO_CELL])
    return (np.array(units, np.int64), np.array(cells, np.uint64), np.array([limbs(m, 8) for m in moduli], np.uint32), free, ins, outs)
