"""An independent restatement of plonky2's vanishing-polynomial check at zeta (plonk/verifier.rs `verify_with_challenges`
+ plonk/vanishing_poly.rs `eval_vanishing_poly`), in plain Python integers.

It replays the transcript with the oracle's Challenger from the caps in the proof words (include/glp.h layout), evaluates
  L_0(zeta) (Z(zeta) - 1),  the partial-product chunk checks,  selector filter x gate constraints,
reduces them with powers of each alpha and compares with Z_H(zeta) * sum_j zeta^(n j) q_j(zeta).  It shares no code with the
library's verifier; tests/test_ext_gates.py pins it against oracle proofs first.

Gate bodies are written once over an abstract field: F_P (one trace row, base-field wires) or F_P2 (openings at zeta).
"""
import numpy as np

P = 0xFFFFFFFF00000001
W7 = 7                      # X^2 = 7 in F_p^2, Y^2 = 7 in the extension algebra over it
UNUSED_SELECTOR = 0xFFFFFFFF

GATE_NOOP, GATE_CONSTANT, GATE_PUBLIC_INPUT, GATE_ARITHMETIC = 0, 1, 2, 3
GATE_ARITHMETIC_EXTENSION, GATE_MUL_EXTENSION, GATE_REDUCING, GATE_REDUCING_EXTENSION = 15, 16, 17, 18
SUPPORTED = (GATE_NOOP, GATE_CONSTANT, GATE_PUBLIC_INPUT, GATE_ARITHMETIC, GATE_ARITHMETIC_EXTENSION, GATE_MUL_EXTENSION,
             GATE_REDUCING, GATE_REDUCING_EXTENSION)


class _Fp:
    """The base field; elements are ints in [0, P)."""
    zero, one = 0, 1

    @staticmethod
    def lift(x): return int(x) % P
    @staticmethod
    def add(a, b): return (a + b) % P
    @staticmethod
    def sub(a, b): return (a - b) % P
    @staticmethod
    def mul(a, b): return a * b % P


class _Fp2:
    """F_p[X]/(X^2 - 7); elements are (a, b) = a + b X."""
    zero, one = (0, 0), (1, 0)

    @staticmethod
    def lift(x): return (int(x) % P, 0)
    @staticmethod
    def add(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
    @staticmethod
    def sub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
    @staticmethod
    def mul(a, b): return ((a[0] * b[0] + W7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)

    @staticmethod
    def inv(a):
        nrm = (a[0] * a[0] - W7 * a[1] * a[1]) % P
        ni = pow(nrm, P - 2, P)
        return (a[0] * ni % P, (P - a[1]) * ni % P)


def _alg_mul(F, a, b):
    """Quadratic extension algebra over F: (a0 + a1 Y)(b0 + b1 Y) = (a0 b0 + 7 a1 b1) + (a0 b1 + a1 b0) Y."""
    return (F.add(F.mul(a[0], b[0]), F.mul(F.lift(W7), F.mul(a[1], b[1]))), F.add(F.mul(a[0], b[1]), F.mul(a[1], b[0])))


def gate_constraints(F, g, gc, w, pih):
    """Unfiltered constraints of gate g (dict with type, p0, p1) at one point: gc = gate constants (selectors removed),
    w = wires, pih = public-input hash (4 base elements), all in F."""
    t, p0 = int(g["type"]), int(g["p0"])
    out = []
    if t == GATE_CONSTANT:
        out = [F.sub(gc[i], w[i]) for i in range(p0)]
    elif t == GATE_PUBLIC_INPUT:
        out = [F.sub(w[i], F.lift(pih[i])) for i in range(4)]
    elif t == GATE_ARITHMETIC:
        for i in range(p0):
            m0, m1, ad, o = w[4 * i:4 * i + 4]
            out.append(F.sub(o, F.add(F.mul(F.mul(m0, m1), gc[0]), F.mul(ad, gc[1]))))
    elif t in (GATE_ARITHMETIC_EXTENSION, GATE_MUL_EXTENSION):
        st = 8 if t == GATE_ARITHMETIC_EXTENSION else 6
        for i in range(p0):
            o = st * i
            pr = _alg_mul(F, (w[o], w[o + 1]), (w[o + 2], w[o + 3]))
            comp = [F.mul(pr[k], gc[0]) for k in range(2)]
            if t == GATE_ARITHMETIC_EXTENSION:
                comp = [F.add(comp[k], F.mul(w[o + 4 + k], gc[1])) for k in range(2)]
            out += [F.sub(w[o + st - 2 + k], comp[k]) for k in range(2)]
    elif t in (GATE_REDUCING, GATE_REDUCING_EXTENSION):
        cw = 1 if t == GATE_REDUCING else 2
        alpha, acc = (w[2], w[3]), (w[4], w[5])
        for i in range(p0):
            c = 6 + cw * i
            coeff = (w[c], F.zero) if cw == 1 else (w[c], w[c + 1])
            a = 6 + cw * p0 + 2 * i if i + 1 < p0 else 0
            nxt = (w[a], w[a + 1])
            pr = _alg_mul(F, acc, alpha)
            out += [F.sub(F.add(pr[k], coeff[k]), nxt[k]) for k in range(2)]
            acc = nxt
    elif t != GATE_NOOP:
        raise NotImplementedError("gate type %d" % t)
    return out


def row_constraints(desc, gate_index, row):
    """Base-field constraints of gate `gate_index` on trace row `row` of a synth circuit (unfiltered)."""
    g = desc.gates[gate_index]
    w = [int(x) for x in desc.wires[:, row]]
    gc = [int(x) for x in desc.constants[desc.num_selectors:, row]]
    pih = [0, 0, 0, 0]
    return gate_constraints(_Fp, g, gc, w, pih)


def proof_layout(desc):
    """Word offsets of the three caps, of each opening category and of the public inputs in a proof."""
    cap = 4 << int(desc.cap_height)
    nc, nr, nw = int(desc.num_constants), int(desc.num_routed_wires), int(desc.num_wires)
    nch, npp, qdf = int(desc.num_challenges), int(desc.num_partial_products), int(desc.quotient_degree_factor)
    lay, o = {"wires_cap": 0, "zs_cap": cap, "q_cap": 2 * cap}, 3 * cap
    for name, cnt in (("constants", nc), ("sigmas", nr), ("wires", nw), ("zs", nch), ("zs_next", nch), ("pp", nch * npp),
                      ("q", nch * qdf)):
        lay[name] = (o, cnt)
        o += 2 * cnt
    return lay


def challenges(desc, proof, digest, hasher=0):
    """betas, gammas, alphas, zeta of the proof's transcript (plonk/get_challenges.rs up to zeta)."""
    from oracle import oracle
    proof = np.asarray(proof, np.uint64)
    lay = proof_layout(desc)
    cap = 4 << int(desc.cap_height)
    nch = int(desc.num_challenges)
    npi = len(desc.public_inputs)
    pi = [int(x) for x in proof[len(proof) - npi:]] if npi else []
    pih = [int(x) for x in oracle.hash_no_pad(pi)] if npi else [0, 0, 0, 0]
    ch = oracle.Challenger(hasher)
    obs_hash = ch.observe_hashes if hasher else ch.observe
    obs_hash(np.asarray(digest, np.uint64))
    ch.observe(np.asarray(pih, np.uint64))          # InnerHasher = Poseidon in both configurations: 4 field elements
    obs_hash(proof[lay["wires_cap"]:lay["wires_cap"] + cap])
    betas, gammas = ch.get_n(nch), ch.get_n(nch)
    obs_hash(proof[lay["zs_cap"]:lay["zs_cap"] + cap])
    alphas = ch.get_n(nch)
    obs_hash(proof[lay["q_cap"]:lay["q_cap"] + cap])
    zeta = tuple(ch.get_ext())
    return betas, gammas, alphas, zeta, pih


def check(desc, proof, digest, hasher=0):
    """True iff vanishing(zeta) == Z_H(zeta) * reduce_with_powers(quotient chunks, zeta^n) for every challenge."""
    F = _Fp2
    proof = np.asarray(proof, np.uint64)
    betas, gammas, alphas, zeta, pih = challenges(desc, proof, digest, hasher)
    lay = proof_layout(desc)

    def ext(name):
        o, cnt = lay[name]
        return [(int(proof[o + 2 * k]), int(proof[o + 2 * k + 1])) for k in range(cnt)]
    cs, sg, lw, zs, zn, pp, q = (ext(k) for k in ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q"))
    lg, nch = int(desc.degree_bits), int(desc.num_challenges)
    n, nr, qdf, npp = 1 << lg, int(desc.num_routed_wires), int(desc.quotient_degree_factor), int(desc.num_partial_products)
    nsel = int(desc.num_selectors)
    k_is = [int(x) for x in desc.k_is]
    zpow = zeta
    for _ in range(lg):
        zpow = F.mul(zpow, zpow)
    zh = F.sub(zpow, F.one)
    l0 = F.mul(zh, F.inv(F.mul(F.sub(zeta, F.one), F.lift(n))))
    terms = [F.mul(l0, F.sub(zs[i], F.one)) for i in range(nch)]
    for i in range(nch):
        for c in range(npp + 1):
            num, den = F.one, F.one
            for j in range(c * qdf, min((c + 1) * qdf, nr)):
                num = F.mul(num, F.add(F.add(lw[j], F.mul(zeta, F.lift(k_is[j] * betas[i]))), F.lift(gammas[i])))
                den = F.mul(den, F.add(F.add(lw[j], F.mul(sg[j], F.lift(betas[i]))), F.lift(gammas[i])))
            prev = zs[i] if c == 0 else pp[i * npp + c - 1]
            nxt = zn[i] if c == npp else pp[i * npp + c]
            terms.append(F.sub(F.mul(prev, num), F.mul(nxt, den)))
    gate_terms = [F.zero] * int(desc.num_gate_constraints)
    for g in desc.gates:
        s = cs[int(g["selector_index"])]
        filt = F.one
        for i in range(int(g["group_start"]), int(g["group_end"])):
            if i != int(g["row"]):
                filt = F.mul(filt, F.sub(F.lift(i), s))
        if nsel > 1:
            filt = F.mul(filt, F.sub(F.lift(UNUSED_SELECTOR), s))
        for k, v in enumerate(gate_constraints(F, g, cs[nsel:], lw, pih)):
            gate_terms[k] = F.add(gate_terms[k], F.mul(filt, v))
    terms += gate_terms
    for i in range(nch):
        van = F.zero
        for v in reversed(terms):
            van = F.add(F.mul(van, F.lift(alphas[i])), v)
        t = F.zero
        for k in reversed(range(qdf)):
            t = F.add(F.mul(t, zpow), q[i * qdf + k])
        if van != F.mul(zh, t):
            return False
    return True
