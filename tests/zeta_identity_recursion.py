"""The recursion gates -- ExponentiationGate, CosetInterpolationGate, PoseidonMdsGate (recalled from plonky2 0.1.x, D = 2) -- restated
over the abstract field of tests/zeta_identity.py, and the vanishing identity at zeta with these bodies next to that module's.

The fields, the proof layout and the transcript replay come from tests/zeta_identity.py; the gate bodies and the identity below are
written from the gates' definitions and share no code with csrc/ or with synth.py's fillers.  tests/test_recursion_gates.py pins
`check` against oracle proofs before anything relies on it.
"""
import numpy as np

import limb_gates_restate as lg
import zeta_identity as zi
from zeta_identity import P, _Fp, _Fp2, _alg_mul, challenges, proof_layout

GATE_BASE_SUM = 13           # the helper gate whose limbs feed ExponentiationGate's power bits
GATE_EXPONENTIATION, GATE_COSET_INTERPOLATION, GATE_POSEIDON_MDS = 20, 21, 22
RECURSION = (GATE_EXPONENTIATION, GATE_COSET_INTERPOLATION, GATE_POSEIDON_MDS)

# Poseidon's MDS matrix over Goldilocks, width 12: circulant first row and diagonal
MDS_CIRC = (17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20)
MDS_DIAG = (8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
POW2_GEN = 1753635133440165772           # of order 2^32 (plonky2's POWER_OF_TWO_GENERATOR)


def subgroup(bits):
    """g^0 .. g^(2^bits - 1) for the g of order 2^bits plonky2 uses (primitive_root_of_unity)."""
    g = pow(POW2_GEN, 1 << (32 - bits), P)
    assert pow(g, 1 << bits, P) == 1 and (bits == 0 or pow(g, 1 << (bits - 1), P) != 1)
    return [pow(g, i, P) for i in range(1 << bits)]


def coset_layout(bits, d):
    """Wire offsets of CosetInterpolationGate(subgroup_bits = bits, degree = d)."""
    n = 1 << bits
    ni = (n - 2) // (d - 1)
    lay = {"n": n, "ni": ni, "shift": 0, "values": 1, "point": 1 + 2 * n, "value": 3 + 2 * n, "evals": 5 + 2 * n,
           "prods": 5 + 2 * n + 2 * ni, "shifted": 5 + 2 * n + 4 * ni}
    lay["wires"], lay["routed"] = lay["shifted"] + 2, 1 + 2 * (n + 2)
    return lay


def _alg_scale(F, a, s):
    return (F.mul(a[0], s), F.mul(a[1], s))


def _alg_sub(F, a, b):
    return (F.sub(a[0], b[0]), F.sub(a[1], b[1]))


def _alg_add(F, a, b):
    return (F.add(a[0], b[0]), F.add(a[1], b[1]))


def recursion_constraints(F, g, w):
    """Unfiltered constraints of a recursion gate at one point; w = wires in F."""
    t, p0, p1 = int(g["type"]), int(g["p0"]), int(g["p1"])
    out = []
    if t == GATE_BASE_SUM:                      # BaseSumGate<B>: sum_j limb_j B^j - wire 0, then prod_{x < B} (limb_j - x) per limb
        limbs, base, acc = w[1:1 + p0], p1, F.zero
        for limb in reversed(limbs):
            acc = F.add(F.mul(acc, F.lift(base)), limb)
        out.append(F.sub(acc, w[0]))
        for limb in limbs:
            prod = F.one
            for x in range(base):
                prod = F.mul(prod, F.sub(limb, F.lift(x)))
            out.append(prod)
    elif t == GATE_EXPONENTIATION:
        n = p0
        bits, inter = w[1:1 + n], w[n + 2:2 * n + 2]
        for i in range(n):
            prev = F.one if i == 0 else F.mul(inter[i - 1], inter[i - 1])
            bit = bits[n - 1 - i]
            out.append(F.sub(F.mul(prev, F.sub(F.add(F.mul(bit, w[0]), F.one), bit)), inter[i]))
        out.append(F.sub(w[n + 1], inter[n - 1]))
    elif t == GATE_POSEIDON_MDS:
        for r in range(12):
            for k in range(2):
                acc = F.mul(F.lift(MDS_DIAG[r]), w[2 * r + k])
                for i in range(12):
                    acc = F.add(acc, F.mul(F.lift(MDS_CIRC[i]), w[2 * ((i + r) % 12) + k]))
                out.append(F.sub(w[24 + 2 * r + k], acc))
    elif t == GATE_COSET_INTERPOLATION:
        lay = coset_layout(p0, p1)
        n, ni, d = lay["n"], lay["ni"], p1
        pair = lambda o: (w[o], w[o + 1])
        xs = subgroup(p0)
        n_inv = pow(n, P - 2, P)
        x = pair(lay["shifted"])
        out += list(_alg_sub(F, _alg_scale(F, x, w[0]), pair(lay["point"])))
        ev, pr = (F.zero, F.zero), (F.one, F.zero)
        chunks = [(0, d)] + [(d + i * (d - 1), min(d + (i + 1) * (d - 1), n)) for i in range(ni)]
        for c, (a, b_) in enumerate(chunks):
            for j in range(a, b_):
                dx = (F.sub(x[0], F.lift(xs[j])), x[1])
                term = _alg_scale(F, _alg_mul(F, pair(lay["values"] + 2 * j), pr), F.lift(xs[j] * n_inv))
                ev = _alg_add(F, _alg_mul(F, ev, dx), term)
                pr = _alg_mul(F, pr, dx)
            if c < ni:
                ie, ip = pair(lay["evals"] + 2 * c), pair(lay["prods"] + 2 * c)
                out += list(_alg_sub(F, ie, ev)) + list(_alg_sub(F, ip, pr))
                ev, pr = ie, ip
        assert chunks[-1][1] == n
        out += list(_alg_sub(F, pair(lay["value"]), ev))
    else:
        raise NotImplementedError("gate type %d" % t)
    return out


def gate_constraints(F, g, gc, w, pih):
    """tests/zeta_identity.py's gates, the recursion gates and the limb gates of tests/limb_gates_restate.py (types 4-12 and 14)."""
    if int(g["type"]) in RECURSION + (GATE_BASE_SUM,):
        return recursion_constraints(F, g, w)
    if int(g["type"]) in lg.LIMB_GATES:
        return lg.limb_gate_constraints(F, g, gc, w)
    return zi.gate_constraints(F, g, gc, w, pih)


def gate_rows(desc, gate_index):
    """Trace rows that carry gate `gate_index` (any number of selector polynomials)."""
    return np.nonzero(desc.constants[int(desc.gates[gate_index]["selector_index"])] == gate_index)[0]


def row_constraints(desc, gate_index, row, wires=None):
    """Base-field constraints of gate `gate_index` on trace row `row` (unfiltered); wires: a replacement for desc.wires."""
    g = desc.gates[gate_index]
    src = desc.wires if wires is None else wires
    w = [int(x) for x in src[:, row]]
    gc = [int(x) for x in desc.constants[desc.num_selectors:, row]]
    return gate_constraints(_Fp, g, gc, w, [0, 0, 0, 0])


def check(desc, proof, digest, hasher=0):
    """True iff, for every challenge, sum_k term_k alpha^k == Z_H(zeta) sum_j zeta^(n j) q_j(zeta), the terms being L_0 (Z - 1), the
    partial-product checks and the selector-filtered gate constraints at zeta (plonk/vanishing_poly.rs eval_vanishing_poly)."""
    F = _Fp2
    proof = np.asarray(proof, np.uint64)
    betas, gammas, alphas, zeta, pih = challenges(desc, proof, digest, hasher)
    lay = proof_layout(desc)

    def opened(name):
        o, cnt = lay[name]
        return [(int(proof[o + 2 * k]), int(proof[o + 2 * k + 1])) for k in range(cnt)]
    cs, sg, lw, zs, zn, pp, q = (opened(k) for k in ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q"))
    lg, nch, nsel = int(desc.degree_bits), int(desc.num_challenges), int(desc.num_selectors)
    nr, qdf, npp = int(desc.num_routed_wires), int(desc.quotient_degree_factor), int(desc.num_partial_products)
    zn_pow = zeta
    for _ in range(lg):
        zn_pow = F.mul(zn_pow, zn_pow)
    z_h = F.sub(zn_pow, F.one)
    l0 = F.mul(z_h, F.inv(F.mul(F.lift(1 << lg), F.sub(zeta, F.one))))
    terms = [F.mul(l0, F.sub(zs[i], F.one)) for i in range(nch)]
    for i in range(nch):
        beta, gamma = F.lift(betas[i]), F.lift(gammas[i])
        chain = [zs[i]] + pp[i * npp:(i + 1) * npp] + [zn[i]]
        for c in range(npp + 1):
            num = den = F.one
            for j in range(c * qdf, min((c + 1) * qdf, nr)):
                s_id = F.mul(zeta, F.lift(int(desc.k_is[j])))
                num = F.mul(num, F.add(F.add(lw[j], F.mul(beta, s_id)), gamma))
                den = F.mul(den, F.add(F.add(lw[j], F.mul(beta, sg[j])), gamma))
            terms.append(F.sub(F.mul(chain[c], num), F.mul(chain[c + 1], den)))
    per_gate = [F.zero] * int(desc.num_gate_constraints)
    for g in desc.gates:
        s = cs[int(g["selector_index"])]
        filt = F.one
        for i in range(int(g["group_start"]), int(g["group_end"])):
            if i != int(g["row"]):
                filt = F.mul(filt, F.sub(F.lift(i), s))
        if nsel > 1:
            filt = F.mul(filt, F.sub(F.lift(zi.UNUSED_SELECTOR), s))
        vals = gate_constraints(F, g, cs[nsel:], lw, pih)
        assert len(vals) == int(g["num_constraints"])
        for k, v in enumerate(vals):
            per_gate[k] = F.add(per_gate[k], F.mul(filt, v))
    terms += per_gate
    for i in range(nch):
        alpha, lhs, rhs = F.lift(alphas[i]), F.zero, F.zero
        for v in reversed(terms):
            lhs = F.add(F.mul(lhs, alpha), v)
        for k in reversed(range(qdf)):
            rhs = F.add(F.mul(rhs, zn_pow), q[i * qdf + k])
        if lhs != F.mul(z_h, rhs):
            return False
    return True
