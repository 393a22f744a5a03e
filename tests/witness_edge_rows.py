"""Hand-chosen rows at the corners where the row-local generators branch, and the circuits that carry them.

Per generator type one circuit of rows whose inputs lie in the gate's domain and, where the gate has inputs outside it, one of rows
that do not.  Every circuit is synth.Builder + set_rows with an identity sigma (no copy can fail): the table rows are the gate rows,
every other row is a NoopGate, at the smallest log_n >= 3 that fits.  Gate parameters are the ones synth.fill_ecdsa_gate_rows /
fill_gate_row, ext_gate_params and recursion_gate_params instantiate (standard_ecc_config for types 8-14, standard_recursion_config
for the rest), plus a ComparisonGate whose num_chunks does not divide num_bits (10 bits in 4 chunks of 3: degree 8, which
max_quotient_degree_factor = 8 carries) and U32AddManyGate at every num_addends up to 15 (16 in the out-of-domain circuit).

A row is a list of (column, value) inputs and the row's gate constants; everything a generator writes comes from
tests/witness_fill_restate.py.  Which set a row belongs to is decided by the restated constraints after the restated fill, never by the
code under test: a row declared out of domain that turns out satisfiable moves to the in-domain circuit (classified() reports the moves; tests/test_witness_edge_rows.py lists them with the reason).
"""
import itertools

import numpy as np

import plonky2_lib_amd.synth as synth
import limb_gates_restate as lg
import witness_fill_restate as wf
import zeta_identity_recursion as zr
from zeta_identity import _Fp

P = 0xFFFFFFFF00000001
M32 = (1 << 32) - 1
SPECIAL = [0, 1, 2, 3, P - 1, P - 2, P - 3, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001,
           0xFFFFFFFEFFFFFFFF, 1 << 63, (1 << 63) - 1, 0xFFFFFFFF]          # the set of tests/test_gpu_launch_paths.py
E6 = [0, 1, P - 1, M32, 1 << 32, 0xFFFFFFFF00000000]
REC, ECC = synth.Config.standard_recursion_config, synth.Config.standard_ecc_config
NAMES = {1: "Constant", 3: "Arithmetic", 4: "Poseidon", 5: "U32Interleave", 6: "UninterleaveToU32", 7: "UninterleaveToB32",
         8: "U32Arithmetic", 9: "U32AddMany", 10: "U32Subtraction", 11: "U32RangeCheck", 12: "Comparison", 13: "BaseSum",
         14: "RandomAccess", 15: "ArithmeticExtension", 16: "MulExtension", 17: "Reducing", 18: "ReducingExtension",
         20: "Exponentiation", 21: "CosetInterpolation", 22: "PoseidonMds"}


class Row:
    def __init__(self, kind, label, inputs, consts=(), declared_in=True):
        self.kind, self.label, self.inputs, self.consts, self.declared_in = kind, label, list(inputs), list(consts), declared_in


def _cyc(seq, k, count):
    return [seq[(k + i) % len(seq)] for i in range(count)]


def _ops_rows(kind, label, cases, ops, place, declared_in=True, consts=None):
    """cases (tuples of op inputs) packed `ops` to a row, the last row filled up by starting over; place(i, case) -> [(col, value)]"""
    rows = []
    for r0 in range(0, len(cases), ops):
        inputs = []
        for i in range(ops):
            inputs += place(i, cases[(r0 + i) % len(cases)])
        rows.append(Row(kind, "%s %d" % (label, r0 // ops), inputs, consts(len(rows)) if consts else (), declared_in))
    return rows


def _same_op_rows(kind, label, cases, ops, place, declared_in):
    """one row per case, every op of the row the same case"""
    return [Row(kind, "%s %s" % (label, tuple(hex(v) for v in c)), [cv for i in range(ops) for cv in place(i, c)], (), declared_in)
            for c in cases]


def _triples():
    return list(itertools.product(E6, repeat=3))


def _rows_of_type(t):
    """[Row] of generator type t, in-domain and declared out-of-domain ones."""
    rec, ecc = REC(), ECC()
    nr, nw = ecc.num_routed_wires, ecc.num_wires
    rows = []
    if t == 1:
        k = (1, rec.num_constants, 0)
        rows = [Row(k, "SPECIAL %d" % i, [], _cyc(SPECIAL, 2 * i, 2)) for i in range(8)]
    elif t == 3:
        k = (3, rec.num_routed_wires // 4, 0)
        pairs = list(itertools.product(E6, repeat=2))
        rows = _ops_rows(k, "E6^3", _triples() * 4, k[1], lambda i, c: [(4 * i + j, c[j]) for j in range(3)],
                         consts=lambda r: pairs[r % len(pairs)])[:len(pairs)]
    elif t in (15, 16):
        p0 = synth.ext_gate_params(rec)[t]
        k, st = (t, p0, 0), 8 if t == 15 else 6
        pairs = list(itertools.product(E6, repeat=2))

        def place(i, c):
            x, y, z = c
            vals = [x, y, y, z, z, x] if t == 15 else [x, y, z, x]
            return [(st * i + j, v) for j, v in enumerate(vals)]
        rows = _ops_rows(k, "E6^3", _triples(), p0, place, consts=lambda r: pairs[(7 * r) % len(pairs)][:2 if t == 15 else 1])
    elif t == 4:
        k = (4, 0, 0)
        states = {"all 0": [0] * 12, "all p-1": [P - 1] * 12, "SPECIAL 0..11": SPECIAL[:12], "SPECIAL 4..15": SPECIAL[4:]}
        for swap in (0, 1, 2):
            for name, s in states.items():
                rows.append(Row(k, "swap %d, %s" % (swap, name), list(enumerate(s)) + [(lg.POS_SWAP, swap)], (), swap < 2))
    elif t == 5:
        ops = min(rec.num_wires // 34, rec.num_routed_wires // 2)
        k, place = (5, ops, 0), lambda i, c: [(2 * i, c[0])]
        rows = _ops_rows(k, "x", [(x,) for x in (0, 1, 1 << 31, M32, 0x55555555, 0xAAAAAAAA)], ops, place)
        rows += _same_op_rows(k, "x", [(1 << 32,), (P - 1,)], ops, place, False)
    elif t in (6, 7):
        ops = min(rec.num_wires // 67, rec.num_routed_wires // 3)
        k = (t, ops, 0)
        xs = (0, 1, 2, 1 << 63, P - 1, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA)
        rows = _ops_rows(k, "x", [(x,) for x in xs], ops, lambda i, c: [(3 * i, c[0])])
    elif t == 8:
        ops = min(nr // 6, nw // 38)
        k, place = (8, ops, 0), lambda i, c: [(6 * i + j, c[j]) for j in range(3)]
        rows = _ops_rows(k, "u32", [(M32, M32, M32), (M32, M32, 0), (0, 0, 0), (65536, 65536, 0), (M32, 1, M32)], ops, place)
        rows += _same_op_rows(k, "operands", [(1 << 32, 1 << 32, 0), (P - 1, P - 1, P - 1), (1 << 32, 1, P - 1)], ops, place, False)
    elif t == 9:
        for na in range(1, 17):
            ops = min(nr // (na + 3), nw // (na + 3 + 18))
            k = (9, na, ops)
            place = lambda i, c, na=na: [((na + 3) * i + j, c[0]) for j in range(na + 1)]
            if na <= 15:
                rows += _same_op_rows(k, "%d addends and the carry all" % na, [(0,), (M32,)], ops, place, True)
            else:
                rows += _same_op_rows(k, "16 addends and the carry all", [(M32,)], ops, place, False)
        k3 = (9, 3, min(nr // 6, nw // 24))
        rows += _same_op_rows(k3, "3 addends and the carry all", [(1 << 32,), (P - 1,)], k3[2], lambda i, c: [(6 * i + j, c[0]) for j in range(4)], False)
    elif t == 10:
        ops = min(nr // 5, nw // 21)
        k, place, x = (10, ops, 0), (lambda i, c: [(5 * i + j, c[j]) for j in range(3)]), 0x89ABCDEF
        rows = _ops_rows(k, "u32", [(0, 0, 0), (0, M32, 1), (x, x, 0), (x, x, 1), (M32, 0, 0), (0, 1, 0)], ops, place)
        rows += _same_op_rows(k, "operands", [(1 << 32, 0, 0), (P - 1, 0, 0), (0, 1 << 32, 0), (0, P - 1, 0), (5, 2, P - 1)], ops, place, False)
    elif t == 11:
        ops = min(8, nw // 17)
        k, place = (11, ops, 0), lambda i, c: [(i, c[0])]
        rows = _ops_rows(k, "limb", [(0,), (M32,), (0x55555555,), (0xAAAAAAAA,)], ops, place)
        rows += _same_op_rows(k, "limb", [(1 << 32,), (P - 1,)], ops, place, False)
    elif t == 12:
        for nb, nc in ((32, 16), (10, 4)):
            k, top = (12, nb, nc), (1 << nb) - 1
            cb = -(-nb // nc)
            low, high = (1 << cb) - 1, top & ~((1 << (cb * (nc - 1))) - 1)
            body = 0x12345678 & top & ~low & ~high
            cases = {"equal at 0": (0, 0), "equal at the maximum": (top, top), "first = second + 1": (6, 5),
                     "first = second + 1 across a chunk": (1 << cb, (1 << cb) - 1),
                     "only the lowest chunk differs, first below": (body, body | low), "only the lowest chunk differs, first above": (body | low, body | 1 if low > 1 else body),
                     "only the highest chunk differs, first below": (body, body | high), "only the highest chunk differs, first above": (body | high, body),
                     "(0, max)": (0, top), "(max, 0)": (top, 0)}
            rows += [Row(k, "%d/%d %s" % (nb, nc, name), [(0, a), (1, b)]) for name, (a, b) in cases.items()]
            rows += [Row(k, "%d/%d %s" % (nb, nc, name), [(0, a), (1, b)], (), False)
                     for name, (a, b) in {"first = 2^bits": (top + 1, 5), "second = p - 1": (5, P - 1)}.items()]
    elif t == 13:
        for nl, base, cfg in ((16, 4, ecc), (min(rec.num_routed_wires - 1, 63), 2, rec)):
            k = (13, nl, base)
            vals = {"0": 0, "B^0": 1, "B^1": base, "B^(limbs-1)": base ** (nl - 1), "B^limbs - 1": base ** nl - 1}
            rows += [Row(k, "<%d> %s" % (base, name), [(0, v)]) for name, v in vals.items()]
            rows.append(Row(k, "<%d> B^limbs" % base, [(0, base ** nl)], (), False))
    elif t == 14:
        bits = 4
        copies = min(nr // (2 + (1 << bits)), nw // (2 + (1 << bits) + bits))
        nextra = min(nr - copies * (2 + (1 << bits)), ecc.num_constants)
        k, size = (14, bits, copies | nextra << 16), 1 << bits
        equal, special = [SPECIAL[12]] * size, _cyc(SPECIAL, 0, size)
        place = lambda i, c: [((2 + size) * i, c[0])] + [((2 + size) * i + 2 + j, v) for j, v in enumerate(c[1])]
        cases = [(0, special), (size - 1, special), (7, equal), (size - 1, _cyc(SPECIAL, 5, size)), (0, equal), (size - 1, equal), (1, special), (8, special)]
        rows = _ops_rows(k, "index", cases, copies, place, consts=lambda r: _cyc(SPECIAL, 4 + 3 * r, nextra))
        for idx in (size, P - 1):
            inputs = [cv for i in range(copies) for cv in place(i, (idx if i % 2 == 0 else size - 1, special))]
            rows.append(Row(k, "index %s in every other copy" % hex(idx), inputs, _cyc(SPECIAL, 9, nextra), False))
    elif t in (17, 18):
        p0 = synth.ext_gate_params(rec)[t]
        k, cw = (t, p0, 0), 1 if t == 17 else 2
        for an, alpha in (("0", (0, 0)), ("1", (1, 0)), ("X", (0, 1)), ("(p-1, p-1)", (P - 1, P - 1))):
            for on, old in (("0", (0, 0)), ("(p-1, 1)", (P - 1, 1))):
                for cn, co in (("all p-1", [P - 1] * (cw * p0)), ("SPECIAL", _cyc(SPECIAL, 3, cw * p0))):
                    rows.append(Row(k, "alpha %s, old accumulator %s, coefficients %s" % (an, on, cn),
                                    [(2, alpha[0]), (3, alpha[1]), (4, old[0]), (5, old[1])] + [(6 + j, v) for j, v in enumerate(co)]))
    elif t == 20:
        nb = synth.recursion_gate_params(rec)[20][0]
        k = (20, nb, 0)
        pattern = [(0x5A5A5A5A5A5A5A5A5 >> j) & 1 for j in range(nb)]
        one_hot = lambda j: [1 if i == j else 0 for i in range(nb)]
        cases = {"base 0, all bits 0": (0, [0] * nb), "base 0, bit 0 set": (0, one_hot(0)), "base 0, top bit set": (0, one_hot(nb - 1)),
                 "base 1": (1, pattern), "base p-1, odd exponent": (P - 1, [1] + pattern[1:]), "base p-1, even exponent": (P - 1, [0] + pattern[1:]),
                 "base 7, all bits 1": (7, [1] * nb), "base p-1, all bits 1": (P - 1, [1] * nb), "base 0, all bits 1": (0, [1] * nb),
                 "base 2^32, all bits 0": (1 << 32, [0] * nb)}
        rows = [Row(k, name, [(0, b)] + [(1 + j, v) for j, v in enumerate(bits_)]) for name, (b, bits_) in cases.items()]
    elif t == 21:
        for bits, d in (synth.recursion_gate_params(rec)[21], (3, 3)):
            k, lay = (21, bits, d), zr.coset_layout(bits, d)
            n, xs = lay["n"], zr.subgroup(bits)
            values = _cyc(SPECIAL, 1, 2 * n)
            for shift in (1, 7, P - 1, 0):
                points = {"0": (0, 0), "shift g^0": (shift * xs[0] % P, 0), "shift g^(n-1)": (shift * xs[n - 1] % P, 0), "off the coset": (3, 5),
                          "off the coset in F_p": (5, 0)}
                if shift == 0:
                    points = {"0": (0, 0), "nonzero": (3, 5)}
                for name, pt in points.items():
                    inputs = [(0, shift)] + [(1 + j, v) for j, v in enumerate(values)] + [(lay["point"], pt[0]), (lay["point"] + 1, pt[1])]
                    rows.append(Row(k, "%d points, shift %s, point %s" % (n, hex(shift), name), inputs, (), shift != 0))
    elif t == 22:
        k = (22, 0, 0)
        for name, s in (("all 0", [0] * 24), ("all p-1", [P - 1] * 24), ("SPECIAL", _cyc(SPECIAL, 0, 24)), ("SPECIAL from 9", _cyc(SPECIAL, 9, 24))):
            rows.append(Row(k, name, list(enumerate(s))))
    return rows


def _config(kind):
    return ECC() if 8 <= kind[0] <= 14 and kind != (13, 63, 2) else REC()


def row_cells(row, num_wires):
    """(wires of the row after the restated fill, constraints of the row) on plain integers"""
    g = {"type": row.kind[0], "p0": row.kind[1], "p1": row.kind[2]}
    w = [0] * num_wires
    for c, v in row.inputs:
        assert 0 <= v < P
        w[c] = v
    gc = list(row.consts) + [0] * (2 - len(row.consts))
    src = list(w)

    def put(c, v):
        w[c] = v
    wf.fill_row(g, gc, src, put)
    return w, zr.gate_constraints(_Fp, g, gc, w, [0] * 4)


class EdgeCircuit:
    """name, gate type, in_domain, rows [Row], desc (synth circuit whose wires hold the inputs and the restated outputs), row_of [trace row]"""


def _build(name, t, in_domain, rows, log_n=None, at=None):
    cfgs = {(_config(r.kind).num_wires) for r in rows}
    assert len(cfgs) == 1
    cfg = _config(rows[0].kind)
    cfg.proof_of_work_bits = 0
    lg_n = log_n or max(3, (len(rows) - 1).bit_length())
    b = synth.Builder(cfg, lg_n, seed=0, random_from_row=1 << lg_n)
    at = list(range(len(rows))) if at is None else at
    for r, row in zip(at, rows):
        b.set_rows(np.array([r]), *row.kind)
        w, vals = row_cells(row, cfg.num_wires)
        b.wires[:, r] = np.array(w, np.uint64)
        b.gate_consts[:len(row.consts), r] = np.array(row.consts, np.uint64)
    ec = EdgeCircuit()
    ec.name, ec.type, ec.in_domain, ec.rows, ec.row_of, ec.desc = name, t, in_domain, rows, at, b.build()
    return ec


_CACHE = {}


def classified(t):
    """(in-domain rows, out-of-domain rows, moved labels) of type t: the restated constraints after the restated fill decide"""
    if t not in _CACHE:
        ins, outs, moved = [], [], []
        for row in _rows_of_type(t):
            ok = not any(row_cells(row, _config(row.kind).num_wires)[1])
            (ins if ok else outs).append(row)
            if ok != row.declared_in:
                moved.append((NAMES[t], row.label, "in" if ok else "out"))
        _CACHE[t] = (ins, outs, moved)
    return _CACHE[t]


def circuits():
    """every edge circuit: per type the in-domain one and, where there are such rows, the out-of-domain one; BaseSum<2> rows (63 limbs,
    135 wires) stand in a circuit of their own next to BaseSum<4>'s (136 wires)"""
    out = []
    for t in wf.GENERATOR_TYPES:
        ins, outs, _ = classified(t)
        for in_domain, rows in ((True, ins), (False, outs)):
            groups = {}
            for r in rows:
                groups.setdefault(_config(r.kind).num_wires, []).append(r)
            for nw, rs in sorted(groups.items()):
                suffix = "" if len(groups) == 1 else "-%d" % nw
                out.append(_build("%s%s-%s" % (NAMES[t], suffix, "in" if in_domain else "out"), t, in_domain, rs))
    return out


def subtraction_across_workgroups():
    """2^9 rows: the in-domain U32Subtraction edge rows at trace rows 0, 255, 256 and 511 (the ends of the two workgroups of 256 rows),
    ordinary rows of the same gate between them, NoopGate elsewhere"""
    ins, _, _ = classified(10)
    k = ins[0].kind
    rng = np.random.default_rng(9)
    place = lambda i, c: [(5 * i + j, c[j]) for j in range(3)]
    ordinary = [Row(k, "ordinary %d" % r, [cv for i in range(k[1]) for cv in place(i, [int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 2))])])
                for r in range(60)]
    edge_at = [0, 255, 256, 511]
    rows = [ins[i % len(ins)] for i in range(len(edge_at))] + ordinary
    at = edge_at + [1 + 4 * i for i in range(30)] + [257 + 8 * i for i in range(30)]
    assert len(set(at)) == len(at)
    return _build("U32Subtraction-workgroups", 10, True, rows, log_n=9, at=at)


def scramble_outputs(ec, seed):
    """the circuit's witness with every role-1 cell of its gate rows replaced by a random field element (never the cell's own value)"""
    rng = np.random.default_rng(seed)
    desc = ec.desc
    w = desc.wires.copy()
    for gi, g in enumerate(desc.gates):
        role = np.array(wf.roles(g, desc.num_wires))
        rows = zr.gate_rows(desc, gi)
        cols = np.nonzero(role == 1)[0]
        if len(rows) and len(cols):
            noise = rng.integers(1, P - 1, size=(len(cols), len(rows)), dtype=np.uint64)
            w[np.ix_(cols, rows)] = (desc.wires[np.ix_(cols, rows)].astype(object) + noise.astype(object)) % P
    return w


def role_mask(desc, role_value=1):
    """bool [num_wires][n]: cells whose column has that role on their row's gate"""
    m = np.zeros(desc.wires.shape, bool)
    for gi, g in enumerate(desc.gates):
        role = np.array(wf.roles(g, desc.num_wires))
        rows = zr.gate_rows(desc, gi)
        if len(rows):
            m[np.ix_(role == role_value, rows)] = True
    return m


def first_mismatch(got, want):
    """None, or (column, row, got, wanted) of the first differing cell: what the fill comparisons of the GPU tests assert on"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if bad.size == 0:
        return None
    c, r = (int(x) for x in bad[0])
    return c, r, int(got[c, r]), int(want[c, r])
