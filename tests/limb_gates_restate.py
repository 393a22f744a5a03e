"""Constraint bodies of gate types 4-12 and 14 -- PoseidonGate, the reference's three u32 gates, the five plonky2_u32 gates and
RandomAccessGate -- over the abstract field of tests/zeta_identity.py (_Fp: one trace row; _Fp2: the openings at zeta), each in the
gate's own constraint order.

Written from the gates' definitions: for types 5-7 the reference's `eval_unfiltered` [REF src/u32/gates/interleave_u32.rs:84-135,
uninterleave_to_u32.rs:93-150, uninterleave_to_b32.rs:95-150], for the others the published plonky2 0.1.x / plonky2_u32 crates (gates/
poseidon.rs, gates/random_access.rs; arithmetic_u32.rs, add_many_u32.rs, subtraction_u32.rs, range_check_u32.rs, comparison.rs) as
include/glp.h names them.  Plain Python integers; nothing is imported from the library, from csrc/ or from oracle/.  The 360 round
constants are data (tests/golden/poseidon_round_constants.npy); tests/test_limb_gates_restate.py pins them to the reference's
known-answer vector through the permutation below, and pins every body to oracle proofs through the vanishing identity at zeta.
"""
import os

import numpy as np

P = 0xFFFFFFFF00000001
POSEIDON, U32_INTERLEAVE, UNINTERLEAVE_U32, UNINTERLEAVE_B32 = 4, 5, 6, 7
U32_ARITHMETIC, U32_ADD_MANY, U32_SUBTRACTION, U32_RANGE_CHECK, COMPARISON, RANDOM_ACCESS = 8, 9, 10, 11, 12, 14
LIMB_GATES = (4, 5, 6, 7, 8, 9, 10, 11, 12, 14)

# Poseidon over Goldilocks, width 12: 4 + 4 full rounds around 22 partial ones, x^7, MDS = circulant(MDS_CIRC) + diag(MDS_DIAG)
MDS_CIRC = (17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20)
MDS_DIAG = (8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
HALF_FULL, PARTIAL = 4, 22
_RC = None


def round_constants():
    global _RC
    if _RC is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_round_constants.npy")
        _RC = [int(x) for x in np.load(path)]
        assert len(_RC) == 12 * (2 * HALF_FULL + PARTIAL)
    return _RC


# PoseidonGate's wires (gates/poseidon.rs): input, output, swap, delta, then the S-box inputs of full rounds 1-3, of the partial rounds
# and of the last four full rounds
POS_IN, POS_OUT, POS_SWAP, POS_DELTA, POS_FULL0, POS_PARTIAL, POS_FULL1, POS_WIRES = 0, 12, 24, 25, 29, 65, 87, 135


def _sum(F, xs):
    acc = F.zero
    for x in xs:
        acc = F.add(acc, x)
    return acc


def _horner(F, digits_msb_first, base):
    acc = F.zero
    for d in digits_msb_first:
        acc = F.add(F.mul(acc, F.lift(base)), d)
    return acc


def _range_product(F, x, size):
    """prod_{v < size} (x - v): zero iff x is one of 0 .. size - 1"""
    acc = F.one
    for v in range(size):
        acc = F.mul(acc, F.sub(x, F.lift(v)))
    return acc


def _pow7(F, x):
    x2 = F.mul(x, x)
    x3 = F.mul(x2, x)
    return F.mul(F.mul(x3, x3), x)


def _mds(F, s):
    return [F.add(_sum(F, [F.mul(F.lift(MDS_CIRC[i]), s[(i + r) % 12]) for i in range(12)]), F.mul(F.lift(MDS_DIAG[r]), s[r]))
            for r in range(12)]


def _add_constants(F, s, rnd):
    rc = round_constants()
    return [F.add(s[i], F.lift(rc[12 * rnd + i])) for i in range(12)]


def poseidon_permute(state):
    """The permutation on integers (for the known-answer pin of the constants and for the generator restatement)."""
    F = _IntField
    s = [int(x) % P for x in state]
    for rnd in range(2 * HALF_FULL + PARTIAL):
        s = _add_constants(F, s, rnd)
        if HALF_FULL <= rnd < HALF_FULL + PARTIAL:
            s[0] = _pow7(F, s[0])
        else:
            s = [_pow7(F, x) for x in s]
        s = _mds(F, s)
    return s


class _IntField:
    zero, one = 0, 1
    lift = staticmethod(lambda x: int(x) % P)
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)


def _poseidon(F, w):
    swap = w[POS_SWAP]
    out = [F.mul(swap, F.sub(swap, F.one))]
    s = [None] * 12
    for i in range(4):
        lhs, rhs, delta = w[POS_IN + i], w[POS_IN + 4 + i], w[POS_DELTA + i]
        out.append(F.sub(F.mul(swap, F.sub(rhs, lhs)), delta))
        s[i], s[i + 4] = F.add(lhs, delta), F.sub(rhs, delta)
    s[8:12] = w[POS_IN + 8:POS_IN + 12]
    rnd = 0
    for r in range(HALF_FULL):
        s = _add_constants(F, s, rnd)
        if r:
            ins = w[POS_FULL0 + 12 * (r - 1):POS_FULL0 + 12 * r]
            out += [F.sub(s[i], ins[i]) for i in range(12)]
            s = list(ins)
        s = _mds(F, [_pow7(F, x) for x in s])
        rnd += 1
    for r in range(PARTIAL):
        s = _add_constants(F, s, rnd)
        out.append(F.sub(s[0], w[POS_PARTIAL + r]))
        s[0] = _pow7(F, w[POS_PARTIAL + r])
        s = _mds(F, s)
        rnd += 1
    for r in range(HALF_FULL):
        s = _add_constants(F, s, rnd)
        ins = w[POS_FULL1 + 12 * r:POS_FULL1 + 12 * (r + 1)]
        out += [F.sub(s[i], ins[i]) for i in range(12)]
        s = _mds(F, [_pow7(F, x) for x in ins])
        rnd += 1
    out += [F.sub(s[i], w[POS_OUT + i]) for i in range(12)]
    return out


def _interleave(F, w, ops):
    # [REF src/u32/gates/interleave_u32.rs:84-135]: 32 big-endian bits per op after the 2 ops routed wires
    out = []
    for i in range(ops):
        bits = w[2 * ops + 32 * i:2 * ops + 32 * (i + 1)]
        out.append(F.sub(_horner(F, bits, 2), w[2 * i]))
        out.append(F.sub(_horner(F, bits, 4), w[2 * i + 1]))
        out += [_range_product(F, b, 2) for b in bits]
    return out


def _uninterleave(F, w, ops, b32):
    # [REF src/u32/gates/uninterleave_to_u32.rs:93-150, uninterleave_to_b32.rs:95-150]: 64 big-endian bits of x_interleaved; bits
    # 2 j -> x_evens, 2 j + 1 -> x_odds, weight 2^(31 - j) (U32) or 4^(31 - j) (B32)
    out = []
    for i in range(ops):
        bits = w[3 * ops + 64 * i:3 * ops + 64 * (i + 1)]
        out.append(F.sub(_horner(F, bits, 2), w[3 * i]))
        ev = od = F.zero
        for j in range(32):
            coeff = F.lift(1 << ((2 if b32 else 1) * (31 - j)))
            ev, od = F.add(ev, F.mul(coeff, bits[2 * j])), F.add(od, F.mul(coeff, bits[2 * j + 1]))
        out += [F.sub(ev, w[3 * i + 1]), F.sub(od, w[3 * i + 2])]
        out += [_range_product(F, b, 2) for b in bits]
    return out


def _limbs_msb_first(F, w, first, count, out):
    """The range product of each base-4 limb, most significant first as plonky2_u32 visits them; returns the limbs in that order."""
    limbs = [w[first + j] for j in reversed(range(count))]
    out += [_range_product(F, x, 4) for x in limbs]
    return limbs


def _u32_arithmetic(F, w, ops):
    # arithmetic_u32.rs: m0 m1 + addend = high 2^32 + low, canonical (high = 2^32 - 1 forces low = 0 through the inverse wire)
    out = []
    for i in range(ops):
        m0, m1, addend, low, high, inverse = w[6 * i:6 * i + 6]
        hi_not_max = F.sub(F.mul(inverse, F.sub(F.lift((1 << 32) - 1), high)), F.one)
        out.append(F.mul(hi_not_max, low))
        out.append(F.sub(F.add(F.mul(high, F.lift(1 << 32)), low), F.add(F.mul(m0, m1), addend)))
        limbs = _limbs_msb_first(F, w, 6 * ops + 32 * i, 32, out)
        out.append(F.sub(_horner(F, limbs[16:], 4), low))
        out.append(F.sub(_horner(F, limbs[:16], 4), high))
    return out


def _u32_add_many(F, w, addends, ops):
    # add_many_u32.rs: sum of the addends and the carry in = carry out 2^32 + result; 16 result limbs, 2 carry limbs
    out, wd = [], addends + 3
    for i in range(ops):
        o = wd * i
        result, carry = w[o + addends + 1], w[o + addends + 2]
        out.append(F.sub(F.add(F.mul(carry, F.lift(1 << 32)), result), _sum(F, w[o:o + addends + 1])))
        limbs = _limbs_msb_first(F, w, wd * ops + 18 * i, 18, out)
        out.append(F.sub(_horner(F, limbs[2:], 4), result))
        out.append(F.sub(_horner(F, limbs[:2], 4), carry))
    return out


def _u32_subtraction(F, w, ops):
    # subtraction_u32.rs: result = x - y - borrow in + 2^32 borrow out, result in 16 limbs, borrow out a bit
    out = []
    for i in range(ops):
        x, y, borrow_in, result, borrow_out = w[5 * i:5 * i + 5]
        out.append(F.sub(result, F.add(F.sub(F.sub(x, y), borrow_in), F.mul(F.lift(1 << 32), borrow_out))))
        limbs = _limbs_msb_first(F, w, 5 * ops + 16 * i, 16, out)
        out.append(F.sub(_horner(F, limbs, 4), result))
        out.append(F.mul(borrow_out, F.sub(F.one, borrow_out)))
    return out


def _u32_range_check(F, w, count):
    # range_check_u32.rs: per input 16 little-endian base-4 limbs
    out = []
    for i in range(count):
        limbs = w[count + 16 * i:count + 16 * (i + 1)]
        out.append(F.sub(_horner(F, reversed(limbs), 4), w[i]))
        out += [_range_product(F, x, 4) for x in limbs]
    return out


def comparison_layout(num_bits, num_chunks):
    cb = -(-num_bits // num_chunks)
    lay = {"chunk_bits": cb, "first": 0, "second": 1, "result": 2, "msd": 3, "first_chunks": 4, "second_chunks": 4 + num_chunks,
           "dummies": 4 + 2 * num_chunks, "equal": 4 + 3 * num_chunks, "inter": 4 + 4 * num_chunks, "msd_bits": 4 + 5 * num_chunks}
    lay["wires"] = lay["msd_bits"] + cb + 1
    return lay


def _comparison(F, w, num_bits, num_chunks):
    # comparison.rs (first <= second): little-endian chunks; the most significant differing chunk decides
    lay = comparison_layout(num_bits, num_chunks)
    cb = lay["chunk_bits"]
    a = w[lay["first_chunks"]:lay["first_chunks"] + num_chunks]
    b = w[lay["second_chunks"]:lay["second_chunks"] + num_chunks]
    out = [F.sub(_horner(F, reversed(a), 1 << cb), w[0]), F.sub(_horner(F, reversed(b), 1 << cb), w[1])]
    msd = F.zero
    for i in range(num_chunks):
        out += [_range_product(F, a[i], 1 << cb), _range_product(F, b[i], 1 << cb)]
        diff = F.sub(b[i], a[i])
        dummy, equal, inter = w[lay["dummies"] + i], w[lay["equal"] + i], w[lay["inter"] + i]
        out.append(F.sub(F.mul(diff, dummy), F.sub(F.one, equal)))
        out.append(F.mul(equal, diff))
        out.append(F.sub(inter, F.mul(equal, msd)))
        msd = F.add(inter, F.mul(F.sub(F.one, equal), diff))
    out.append(F.sub(w[lay["msd"]], msd))
    bits = w[lay["msd_bits"]:lay["msd_bits"] + cb + 1]
    out += [F.mul(x, F.sub(F.one, x)) for x in bits]
    out.append(F.sub(F.add(F.lift(1 << cb), w[lay["msd"]]), _horner(F, reversed(bits), 2)))
    out.append(F.sub(w[lay["result"]], bits[cb]))
    return out


def random_access_layout(bits, p1):
    copies, extra, size = p1 & 0xFFFF, p1 >> 16, 1 << bits
    lay = {"copies": copies, "extra": extra, "size": size, "per_copy": 2 + size, "extras": (2 + size) * copies}
    lay["bits"] = lay["extras"] + extra
    lay["wires"] = lay["bits"] + bits * copies
    return lay


def _random_access(F, w, gc, bits, p1):
    # random_access.rs: per copy index, claimed element, 2^bits list items; then the extra constants; then the index bits (advice)
    lay = random_access_layout(bits, p1)
    out = []
    for c in range(lay["copies"]):
        o = lay["per_copy"] * c
        index, claimed, items = w[o], w[o + 1], list(w[o + 2:o + 2 + lay["size"]])
        bs = w[lay["bits"] + bits * c:lay["bits"] + bits * (c + 1)]
        out += [F.mul(b, F.sub(b, F.one)) for b in bs]
        out.append(F.sub(_horner(F, reversed(bs), 2), index))
        for b in bs:
            items = [F.add(items[2 * k], F.mul(b, F.sub(items[2 * k + 1], items[2 * k]))) for k in range(len(items) // 2)]
        out.append(F.sub(items[0], claimed))
    out += [F.sub(gc[i], w[lay["extras"] + i]) for i in range(lay["extra"])]
    return out


def limb_gate_constraints(F, g, gc, w):
    """Unfiltered constraints of a gate of LIMB_GATES at one point; gc = gate constants, w = wires, in F."""
    t, p0, p1 = int(g["type"]), int(g["p0"]), int(g["p1"])
    if t == POSEIDON:
        return _poseidon(F, w)
    if t == U32_INTERLEAVE:
        return _interleave(F, w, p0)
    if t in (UNINTERLEAVE_U32, UNINTERLEAVE_B32):
        return _uninterleave(F, w, p0, t == UNINTERLEAVE_B32)
    if t == U32_ARITHMETIC:
        return _u32_arithmetic(F, w, p0)
    if t == U32_ADD_MANY:
        return _u32_add_many(F, w, p0, p1)
    if t == U32_SUBTRACTION:
        return _u32_subtraction(F, w, p0)
    if t == U32_RANGE_CHECK:
        return _u32_range_check(F, w, p0)
    if t == COMPARISON:
        return _comparison(F, w, p0, p1)
    if t == RANDOM_ACCESS:
        return _random_access(F, w, gc, p0, p1)
    raise NotImplementedError("gate type %d" % t)
