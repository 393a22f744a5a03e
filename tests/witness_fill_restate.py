"""glp_witness_fill and glp_witness_columns restated on the CPU: the 20 row-local generators (gate types 1, 3-18, 20-22) on plain
Python integers, one row at a time, with `only_advice`.

Each generator is written from its gate's definition: the outputs are the values the gate's constraints (tests/limb_gates_restate.py,
tests/zeta_identity.py, tests/zeta_identity_recursion.py) force given the inputs -- for types 5-7 along the reference's generators
[REF src/u32/gates/interleave_u32.rs:289-318, uninterleave_to_u32.rs:332-369, uninterleave_to_b32.rs:335-372].  Nothing is shared
with csrc/, oracle/ or synth.py's fillers.

Inputs outside a gate's domain have no satisfying outputs; what is written then is fixed as include/glp.h states it for
glp_witness_fill:
  * inputs are read as canonical u64; a limb or bit generator decomposes only the bits it has wires for (the low 32 bits of a u32 value,
    num_chunks * chunk_bits bits of a comparison input, num_limbs digits of a BaseSum value) and writes the full field value to the
    u32 result / carry wires;
  * ComparisonGate's result wire is the top bit of 2^chunk_bits + most significant difference (what its constraint ties it to);
  * a RandomAccess copy whose index is >= 2^bits is left untouched (claimed element and bits); the extra constants are still written;
  * a CosetInterpolation row with shift 0 gets shifted point 0.
"""
import limb_gates_restate as lg
import zeta_identity_recursion as zr

P = 0xFFFFFFFF00000001
M32 = (1 << 32) - 1
GENERATOR_TYPES = (1,) + tuple(range(3, 19)) + (20, 21, 22)


def _inv(a):
    return pow(a, P - 2, P)


def _e_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def _e_scale(a, s):
    return (a[0] * s % P, a[1] * s % P)


def _digits(v, base, count):
    out = []
    for _ in range(count):
        out.append(v % base)
        v //= base
    return out


def roles(g, num_wires):
    """glp_witness_columns: per wire column 1 = written on rows of gate g, 2 = read as a generator input, 0 = untouched."""
    t, p0, p1 = int(g["type"]), int(g["p0"]), int(g["p1"])
    ins, outs = [], []
    if t == 1:
        outs = list(range(p0))
    elif t == 3:
        for i in range(p0):
            ins += [4 * i, 4 * i + 1, 4 * i + 2]
            outs.append(4 * i + 3)
    elif t == lg.POSEIDON:
        ins = list(range(12)) + [lg.POS_SWAP]
        outs = list(range(12, 24)) + list(range(lg.POS_DELTA, lg.POS_WIRES))
    elif t == lg.U32_INTERLEAVE:
        ins = [2 * i for i in range(p0)]
        outs = [2 * i + 1 for i in range(p0)] + list(range(2 * p0, 34 * p0))
    elif t in (lg.UNINTERLEAVE_U32, lg.UNINTERLEAVE_B32):
        ins = [3 * i for i in range(p0)]
        outs = [3 * i + k for i in range(p0) for k in (1, 2)] + list(range(3 * p0, 67 * p0))
    elif t == lg.U32_ARITHMETIC:
        ins = [6 * i + k for i in range(p0) for k in range(3)]
        outs = [6 * i + k for i in range(p0) for k in (3, 4, 5)] + list(range(6 * p0, 38 * p0))
    elif t == lg.U32_ADD_MANY:
        wd = p0 + 3
        ins = [wd * i + k for i in range(p1) for k in range(p0 + 1)]
        outs = [wd * i + p0 + k for i in range(p1) for k in (1, 2)] + list(range(wd * p1, (wd + 18) * p1))
    elif t == lg.U32_SUBTRACTION:
        ins = [5 * i + k for i in range(p0) for k in range(3)]
        outs = [5 * i + k for i in range(p0) for k in (3, 4)] + list(range(5 * p0, 21 * p0))
    elif t == lg.U32_RANGE_CHECK:
        ins, outs = list(range(p0)), list(range(p0, 17 * p0))
    elif t == lg.COMPARISON:
        ins, outs = [0, 1], list(range(2, lg.comparison_layout(p0, p1)["wires"]))
    elif t == 13:
        ins, outs = [0], list(range(1, 1 + p0))
    elif t == lg.RANDOM_ACCESS:
        lay = lg.random_access_layout(p0, p1)
        for c in range(lay["copies"]):
            o = lay["per_copy"] * c
            ins += [o] + list(range(o + 2, o + 2 + lay["size"]))
            outs.append(o + 1)
        outs += list(range(lay["extras"], lay["wires"]))
    elif t in (15, 16):
        st = 8 if t == 15 else 6
        for i in range(p0):
            ins += list(range(st * i, st * i + st - 2))
            outs += [st * i + st - 2, st * i + st - 1]
    elif t in (17, 18):
        cw = 1 if t == 17 else 2
        outs = [0, 1] + list(range(6 + cw * p0, 6 + cw * p0 + 2 * (p0 - 1)))
        ins = list(range(2, 6 + cw * p0))
    elif t == 20:
        ins, outs = list(range(p0 + 1)), list(range(p0 + 1, 2 * p0 + 2))
    elif t == 21:
        lay = zr.coset_layout(p0, p1)
        ins, outs = list(range(lay["value"])), list(range(lay["value"], lay["wires"]))
    elif t == 22:
        ins, outs = list(range(24)), list(range(24, 48))
    role = [0] * num_wires
    for c in ins:
        if c < num_wires:
            role[c] = 2
    for c in outs:
        if c < num_wires:
            role[c] = 1
    return role


def _poseidon_row(w, put):
    swap = w[lg.POS_SWAP]
    s = [0] * 12
    for i in range(4):
        lhs, rhs = w[i], w[i + 4]
        delta = swap * (rhs - lhs) % P
        put(lg.POS_DELTA + i, delta)
        s[i], s[i + 4] = (lhs + delta) % P, (rhs - delta) % P
    s[8:12] = w[8:12]
    rc = lg.round_constants()
    for rnd in range(30):
        s = [(s[i] + rc[12 * rnd + i]) % P for i in range(12)]
        if 1 <= rnd < 4:
            for i in range(12):
                put(lg.POS_FULL0 + 12 * (rnd - 1) + i, s[i])
        elif 4 <= rnd < 26:
            put(lg.POS_PARTIAL + rnd - 4, s[0])
        elif rnd >= 26:
            for i in range(12):
                put(lg.POS_FULL1 + 12 * (rnd - 26) + i, s[i])
        if 4 <= rnd < 26:
            s[0] = pow(s[0], 7, P)
        else:
            s = [pow(x, 7, P) for x in s]
        s = [(sum(lg.MDS_CIRC[i] * s[(i + r) % 12] for i in range(12)) + lg.MDS_DIAG[r] * s[r]) % P for r in range(12)]
    for i in range(12):
        put(lg.POS_OUT + i, s[i])


def fill_row(g, gc, w, put):
    """The generators of gate g on one row: w = the row's wires (ints, read only), gc = its gate constants; put(column, value)."""
    t, p0, p1 = int(g["type"]), int(g["p0"]), int(g["p1"])
    if t == 1:
        for i in range(p0):
            put(i, gc[i])
    elif t == 3:
        for i in range(p0):
            put(4 * i + 3, (w[4 * i] * w[4 * i + 1] * gc[0] + w[4 * i + 2] * gc[1]) % P)
    elif t == lg.POSEIDON:
        _poseidon_row(w, put)
    elif t == lg.U32_INTERLEAVE:
        for i in range(p0):
            x = w[2 * i] & M32
            bits = [(x >> (31 - k)) & 1 for k in range(32)]              # big-endian
            for k in range(32):
                put(2 * p0 + 32 * i + k, bits[k])
            put(2 * i + 1, sum(b << (2 * (31 - k)) for k, b in enumerate(bits)) % P)
    elif t in (lg.UNINTERLEAVE_U32, lg.UNINTERLEAVE_B32):
        step = 1 if t == lg.UNINTERLEAVE_U32 else 2
        for i in range(p0):
            x = w[3 * i]
            bits = [(x >> (63 - k)) & 1 for k in range(64)]              # big-endian
            for k in range(64):
                put(3 * p0 + 64 * i + k, bits[k])
            put(3 * i + 1, sum(bits[2 * j] << (step * (31 - j)) for j in range(32)) % P)
            put(3 * i + 2, sum(bits[2 * j + 1] << (step * (31 - j)) for j in range(32)) % P)
    elif t == lg.U32_ARITHMETIC:
        for i in range(p0):
            out = (w[6 * i] * w[6 * i + 1] + w[6 * i + 2]) % P
            low, high = out & M32, out >> 32
            put(6 * i + 3, low)
            put(6 * i + 4, high)
            put(6 * i + 5, _inv(M32 - high) if high != M32 else 0)
            for j, d in enumerate(_digits(out, 4, 32)):
                put(6 * p0 + 32 * i + j, d)
    elif t == lg.U32_ADD_MANY:
        wd = p0 + 3
        for i in range(p1):
            total = sum(w[wd * i:wd * i + p0 + 1]) % P
            result, carry = total & M32, total >> 32
            put(wd * i + p0 + 1, result)
            put(wd * i + p0 + 2, carry)
            for j, d in enumerate(_digits(result, 4, 16) + _digits(carry, 4, 2)):
                put(wd * p1 + 18 * i + j, d)
    elif t == lg.U32_SUBTRACTION:
        for i in range(p0):
            diff = (w[5 * i] - w[5 * i + 1] - w[5 * i + 2]) % P
            borrow = 1 if diff > 1 << 32 else 0                          # x - y - borrow < 0 wraps to the top of the field
            result = (diff + (borrow << 32)) % P
            put(5 * i + 3, result)
            put(5 * i + 4, borrow)
            for j, d in enumerate(_digits(result, 4, 16)):
                put(5 * p0 + 16 * i + j, d)
    elif t == lg.U32_RANGE_CHECK:
        for i in range(p0):
            for j, d in enumerate(_digits(w[i], 4, 16)):
                put(p0 + 16 * i + j, d)
    elif t == lg.COMPARISON:
        lay = lg.comparison_layout(p0, p1)
        cb = lay["chunk_bits"]
        a, b = _digits(w[0], 1 << cb, p1), _digits(w[1], 1 << cb, p1)
        msd = 0
        for i in range(p1):
            put(lay["first_chunks"] + i, a[i])
            put(lay["second_chunks"] + i, b[i])
            equal = a[i] == b[i]
            put(lay["dummies"] + i, 1 if equal else _inv((b[i] - a[i]) % P))
            put(lay["equal"] + i, 1 if equal else 0)
            put(lay["inter"] + i, msd if equal else 0)
            if not equal:
                msd = (b[i] - a[i]) % P
        put(lay["msd"], msd)
        bits = _digits(((1 << cb) + msd) % P, 2, cb + 1)
        for j in range(cb + 1):
            put(lay["msd_bits"] + j, bits[j])
        put(lay["result"], bits[cb])
    elif t == 13:
        for j, d in enumerate(_digits(w[0], p1, p0)):
            put(1 + j, d)
    elif t == lg.RANDOM_ACCESS:
        lay = lg.random_access_layout(p0, p1)
        for c in range(lay["copies"]):
            o = lay["per_copy"] * c
            index = w[o]
            if index < lay["size"]:
                put(o + 1, w[o + 2 + index])
                for j, d in enumerate(_digits(index, 2, p0)):
                    put(lay["bits"] + p0 * c + j, d)
        for e in range(lay["extra"]):
            put(lay["extras"] + e, gc[e])
    elif t in (15, 16):
        st = 8 if t == 15 else 6
        for i in range(p0):
            o = st * i
            res = _e_scale(_e_mul((w[o], w[o + 1]), (w[o + 2], w[o + 3])), gc[0])
            if t == 15:
                res = _e_add(res, _e_scale((w[o + 4], w[o + 5]), gc[1]))
            put(o + st - 2, res[0])
            put(o + st - 1, res[1])
    elif t in (17, 18):
        cw = 1 if t == 17 else 2
        alpha, acc = (w[2], w[3]), (w[4], w[5])
        for i in range(p0):
            c = 6 + cw * i
            acc = _e_add(_e_mul(acc, alpha), (w[c], w[c + 1] if cw == 2 else 0))
            dst = 6 + cw * p0 + 2 * i if i + 1 < p0 else 0
            put(dst, acc[0])
            put(dst + 1, acc[1])
    elif t == 20:
        cur = 1
        for i in range(p0):
            bit = w[1 + (p0 - 1 - i)]                                    # most significant bit first
            cur = cur * cur * (bit * w[0] + 1 - bit) % P
            put(p0 + 2 + i, cur)
        put(p0 + 1, cur)
    elif t == 21:
        lay = zr.coset_layout(p0, p1)
        n, ni, d = lay["n"], lay["ni"], p1
        xs = zr.subgroup(p0)
        n_inv = _inv(n)
        x = _e_scale((w[lay["point"]], w[lay["point"] + 1]), _inv(w[0]) if w[0] else 0)
        put(lay["shifted"], x[0])
        put(lay["shifted"] + 1, x[1])
        ev, pr, j = (0, 0), (1, 0), 0
        for c in range(ni + 1):
            end = min(n, d + c * (d - 1))
            while j < end:
                dx = ((x[0] - xs[j]) % P, x[1])
                ev = _e_add(_e_mul(ev, dx), _e_scale(_e_mul((w[1 + 2 * j], w[2 + 2 * j]), pr), xs[j] * n_inv % P))
                pr = _e_mul(pr, dx)
                j += 1
            if c < ni:
                for k in range(2):
                    put(lay["evals"] + 2 * c + k, ev[k])
                    put(lay["prods"] + 2 * c + k, pr[k])
        put(lay["value"], ev[0])
        put(lay["value"] + 1, ev[1])
    elif t == 22:
        for k in range(2):
            for r in range(12):
                put(24 + 2 * r + k, (sum(lg.MDS_CIRC[i] * w[2 * ((i + r) % 12) + k] for i in range(12)) + lg.MDS_DIAG[r] * w[2 * r + k]) % P)


def fill(desc, wires, only_advice=False):
    """glp_witness_fill on a copy of wires [num_wires][n]: every row's generators once.  A generator reads the row as it was handed
    in -- its inputs are never its own outputs.  only_advice: columns below num_routed_wires are never written."""
    out = wires.copy()
    nsel, nr = int(desc.num_selectors), int(desc.num_routed_wires)
    for gi, g in enumerate(desc.gates):
        if int(g["type"]) not in GENERATOR_TYPES:
            continue
        for r in zr.gate_rows(desc, gi):
            r = int(r)
            w = [int(v) for v in wires[:, r]]
            gc = [int(v) for v in desc.constants[nsel:, r]]

            def put(col, val, r=r):
                assert 0 <= val < P
                if not only_advice or col >= nr:
                    out[col, r] = val
            fill_row(g, gc, w, put)
    return out
