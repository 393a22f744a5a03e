"""Python restatement of plonky2's FRI over a GENERAL FriInstanceInfo, on the oracle's primitives (field, fft, Merkle, Challenger):
`verify_fri_proof` (fri/verifier.rs) and `PolynomialBatch::prove_openings` (fri/oracle.rs, fri/prover.rs) with the smallest
proof-of-work witness.  Test infrastructure for test_fri_openings.py (which pins it against the oracle's own prover and verifier on
the plonk instance) and test_gpu_fri_openings.py (which holds glp_fri_* to it word for word).

An instance is an `Instance`: the oracles' leaf shapes, the points with their column ranges, the FRI parameters.  Extension elements
are pairs of Python ints (a, b) = a + b X, X^2 = 7.  FriProof words: include/glp.h, glp_fri_proof."""
import ctypes

import numpy as np

P = 0xFFFFFFFF00000001
GEN = 7
SALT_SIZE = 4


# ------------------------------------------------------------------ F_p^2 on Python ints
def e_add(x, y): return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)
def e_sub(x, y): return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)
def e_mul(x, y): return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)
def e_scale(x, s): return (x[0] * s % P, x[1] * s % P)


def e_inv(x):
    ni = pow((x[0] * x[0] - 7 * x[1] * x[1]) % P, P - 2, P)
    return (x[0] * ni % P, (P - x[1]) * ni % P)


def e_pow(x, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = e_mul(r, x)
        x = e_mul(x, x)
        e >>= 1
    return r


def brev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def eval_ext(coeffs, z):
    """`PolynomialCoeffs::to_extension().eval(z)`: Horner over base-field coefficients in natural order"""
    acc = (0, 0)
    for c in reversed([int(v) for v in coeffs]):
        acc = e_mul(acc, z)
        acc = ((acc[0] + c) % P, acc[1])
    return acc


def periodic_opening(C, log_n, z):
    """f(z) for f = sum_p C[p mod len(C)] X^p with deg f < n = 2^log_n and m = len(C) dividing n, in closed form:
    (sum_i C_i z^i) (z^n - 1) / (z^m - 1).  The reference for openings too long to walk term by term (pinned against eval_ext in
    test_fri_openings.py)."""
    head, zi = (0, 0), (1, 0)
    for c in C:
        head = e_add(head, e_scale(zi, int(c)))
        zi = e_mul(zi, z)
    num = e_sub(e_pow(z, 1 << log_n), (1, 0))
    return e_mul(head, e_mul(num, e_inv(e_sub(zi, (1, 0)))))


# ------------------------------------------------------------------ instance, oracles
class Instance:
    """points: [((a, b), [(oracle, col_begin, num_cols), ...]), ...]; ncols / salted: per oracle"""

    def __init__(self, log_n, rate_bits, cap_height, hasher, ncols, salted, points, arity_bits, pow_bits, num_query_rounds):
        self.log_n, self.rate_bits, self.cap_height, self.hasher = log_n, rate_bits, cap_height, hasher
        self.ncols, self.salted = list(ncols), list(salted)
        self.points = [((int(z[0]), int(z[1])), [tuple(int(v) for v in r) for r in ranges]) for z, ranges in points]
        self.arity_bits, self.pow_bits, self.nq = list(arity_bits), pow_bits, num_query_rounds
        self.lgN = log_n + rate_bits
        self.leaf_len = [c + (SALT_SIZE if s else 0) for c, s in zip(self.ncols, self.salted)]

    def columns(self, b):
        """(oracle, column) of every polynomial of point b, in order"""
        return [(o, c) for o, cb, nc in self.points[b][1] for c in range(cb, cb + nc)]

    @property
    def num_openings(self):
        return sum(len(self.columns(b)) for b in range(len(self.points)))

    def layout(self):
        """(queries offset, query stride, final_poly offset, final_len, pow offset, total) of the FriProof words"""
        capw = 4 << self.cap_height
        q = sum(ll + 4 * (self.lgN - self.cap_height) for ll in self.leaf_len)
        lg = self.lgN
        for ab in self.arity_bits:
            lg -= ab
            q += (2 << ab) + 4 * (lg - self.cap_height)
        final_len = 1 << (lg - self.rate_bits)
        o_q = capw * len(self.arity_bits)
        o_f = o_q + q * self.nq
        return o_q, q, o_f, final_len, o_f + 2 * final_len, o_f + 2 * final_len + 1


class Committed:
    """one oracle as the prover holds it: coefficients [ncols][n] (natural order), Merkle leaves [N][leaf_len] in plonky2's leaf
    order (salts last), digests, cap"""

    def __init__(self, coeffs, leaves, digests, cap):
        self.coeffs, self.leaves, self.digests, self.cap = coeffs, leaves, digests, cap


def commit(oracle, coeffs, rate_bits, cap_height, hasher=0, salts=None):
    """PolynomialBatch::from_coeffs; salts [N][4] (per Merkle leaf) make it the blinded form"""
    ref = oracle.batch_from_coeffs(coeffs, rate_bits, cap_height, hasher=hasher)
    if salts is None:
        return Committed(ref.coeffs, ref.leaves, ref.digests, ref.cap)
    leaves = np.ascontiguousarray(np.concatenate([ref.leaves, np.asarray(salts, np.uint64)], axis=1))
    with oracle._Hasher(hasher):
        dig, cap = oracle.merkle_build(leaves, cap_height)
    return Committed(ref.coeffs, leaves, dig, cap)


# ------------------------------------------------------------------ transcript helpers
def challenger_state(ch):
    """(sponge state [12], pending inputs) of the oracle's Challenger (struct: st[12], in[8], nin)"""
    raw = np.frombuffer(ctypes.string_at(ch._buf, 8 * 21), dtype=np.uint64)
    nin = int(np.frombuffer(ctypes.string_at(ctypes.addressof(ch._buf) + 8 * 20, 4), dtype=np.int32)[0])
    return raw[:12].copy(), raw[12:12 + nin].copy()


def challenger_clone(oracle, ch):
    c2 = oracle.Challenger(ch.hasher)
    ctypes.memmove(c2._buf, ch._buf, len(ch._buf))
    return c2


def pow_smallest(oracle, ch, bits):
    """fri_proof_of_work with the smallest witness: candidates in increasing order on the transcript's own sponge"""
    st, pend = challenger_state(ch)
    st[:len(pend)] = pend
    permute = oracle.keccak_permute if ch.hasher == 1 else oracle.poseidon_permute
    cand = 0
    while True:
        t = st.copy()
        t[len(pend)] = cand
        if bits == 0 or int(permute(t)[7]) >> (64 - bits) == 0:
            return cand
        cand += 1


# ------------------------------------------------------------------ prove_openings
def prove_openings(oracle, inst, oracles, ch):
    """-> (openings [num_openings] ext pairs, FriProof words).  ch: the transcript right after the openings were observed (it is
    advanced through the query indices)."""
    n, N, lgN = 1 << inst.log_n, 1 << inst.lgN, inst.lgN
    openings = [[eval_ext(oracles[o].coeffs[c], z) for o, c in inst.columns(b)] for b, (z, _) in enumerate(inst.points)]
    alpha = tuple(ch.get_ext())
    fp = [(0, 0)] * n
    for b, (z, _) in enumerate(inst.points):
        re, im, ap = np.zeros(n, np.uint64), np.zeros(n, np.uint64), (1, 0)
        for o, c in inst.columns(b):
            re = oracle.vec_add(re, oracle.vec_scale(oracles[o].coeffs[c], ap[0]))
            im = oracle.vec_add(im, oracle.vec_scale(oracles[o].coeffs[c], ap[1]))
            ap = e_mul(ap, alpha)
        # divide_by_linear(z): b_(k-1) = b_k z + c_k from the top; the remainder (the reduced opening) is dropped
        acc, quot = (0, 0), [(0, 0)] * n
        for i in range(n - 1, -1, -1):
            acc = e_add(e_mul(acc, z), (int(re[i]), int(im[i])))
            if i > 0:
                quot[i - 1] = acc
        fp = [e_add(e_mul(f, ap), q) for f, q in zip(fp, quot)]          # ap = alpha^(len_b): alpha.shift_poly
    o_q, stride, o_f, final_len, o_pow, total = inst.layout()
    words = np.zeros(total, np.uint64)
    capw = 4 << inst.cap_height
    coeffs = fp + [(0, 0)] * (N - n)
    length, lglen, shift = N, lgN, GEN
    trees = []
    for r, ab in enumerate(inst.arity_bits):
        va = oracle.coset_fft(np.array([c[0] for c in coeffs[:length]], np.uint64), shift)
        vb = oracle.coset_fft(np.array([c[1] for c in coeffs[:length]], np.uint64), shift)
        perm = oracle.bitrev_perm(lglen)
        leaves = np.ascontiguousarray(np.stack([va[perm], vb[perm]], axis=1).reshape(length >> ab, 2 << ab))
        with oracle._Hasher(inst.hasher):
            dig, cap = oracle.merkle_build(leaves, inst.cap_height)
        words[r * capw:(r + 1) * capw] = cap.reshape(-1)
        ch.observe_hashes(cap)
        trees.append((leaves, dig))
        beta = tuple(ch.get_ext())
        arity = 1 << ab
        nxt = []
        for k in range(length >> ab):
            acc = (0, 0)
            for t in range(arity - 1, -1, -1):
                acc = e_add(e_mul(acc, beta), coeffs[k * arity + t])
            nxt.append(acc)
        coeffs, length, lglen, shift = nxt, length >> ab, lglen - ab, pow(shift, arity, P)
    for i in range(final_len):
        words[o_f + 2 * i], words[o_f + 2 * i + 1] = coeffs[i]
    ch.observe(words[o_f:o_f + 2 * final_len])
    wit = pow_smallest(oracle, ch, inst.pow_bits)
    words[o_pow] = wit
    ch.observe([wit])
    resp = ch.get()
    assert inst.pow_bits == 0 or resp >> (64 - inst.pow_bits) == 0
    for q in range(inst.nq):
        x = ch.get() % N
        w = o_q + q * stride
        for ob in oracles:
            ll = ob.leaves.shape[1]
            words[w:w + ll] = ob.leaves[x]; w += ll
            sib = oracle.merkle_prove(ob.digests, N, inst.cap_height, x).reshape(-1)
            words[w:w + sib.size] = sib; w += sib.size
        nl = N
        for (leaves, dig), ab in zip(trees, inst.arity_bits):
            nl >>= ab
            x >>= ab
            words[w:w + (2 << ab)] = leaves[x]; w += 2 << ab
            sib = oracle.merkle_prove(dig, nl, inst.cap_height, x).reshape(-1)
            words[w:w + sib.size] = sib; w += sib.size
        assert w == o_q + (q + 1) * stride
    return [e for pt in openings for e in pt], words


# ------------------------------------------------------------------ verify_fri_proof
def verify_fri_proof(oracle, inst, caps, openings, words, ch):
    """0 if the FriProof verifies for the instance, the oracles' caps and the claimed openings (flat, points in order); else a
    positive code naming the failed check (the numbering of the oracle's glo_verify).  ch: the transcript right after the openings."""
    words = np.asarray(words, np.uint64)
    o_q, stride, o_f, final_len, o_pow, total = inst.layout()
    if words.size != total or (words >= np.uint64(P)).any():
        return 1
    N, lgN, capw, depth0 = 1 << inst.lgN, inst.lgN, 4 << inst.cap_height, inst.lgN - inst.cap_height
    alpha = tuple(ch.get_ext())
    betas = []
    for r in range(len(inst.arity_bits)):
        ch.observe_hashes(words[r * capw:(r + 1) * capw].reshape(-1, 4))
        betas.append(tuple(ch.get_ext()))
    ch.observe(words[o_f:o_f + 2 * final_len])
    ch.observe(words[o_pow:o_pow + 1])
    resp = ch.get()
    if inst.pow_bits and resp >> (64 - inst.pow_bits) != 0:
        return 2
    # PrecomputedReducedOpenings: per point, sum_j alpha^j v_j
    reds, k = [], 0
    for b in range(len(inst.points)):
        red, ap = (0, 0), (1, 0)
        for _ in inst.columns(b):
            red = e_add(red, e_mul(ap, tuple(int(v) for v in openings[k])))
            ap = e_mul(ap, alpha)
            k += 1
        reds.append(red)
    wN = oracle.root_of_unity(lgN)
    final = [(int(words[o_f + 2 * i]), int(words[o_f + 2 * i + 1])) for i in range(final_len)]
    for q in range(inst.nq):
        x = ch.get() % N
        w = o_q + q * stride
        evals = []
        for o, ll in enumerate(inst.leaf_len):
            leaf, path = words[w:w + ll], words[w + ll:w + ll + 4 * depth0]
            if not oracle.merkle_verify(leaf, x, caps[o], path, hasher=inst.hasher):
                return 4
            evals.append(leaf)
            w += ll + 4 * depth0
        sx = GEN * pow(wN, brev(x, lgN), P) % P
        # fri_combine_initial; the salts at the end of a leaf are never named
        s = (0, 0)
        for b, (z, _) in enumerate(inst.points):
            r, ap = (0, 0), (1, 0)
            for o, c in inst.columns(b):
                r = e_add(r, e_scale(ap, int(evals[o][c])))
                ap = e_mul(ap, alpha)
            s = e_add(e_mul(s, ap), e_mul(e_sub(r, reds[b]), e_inv(e_sub((sx, 0), z))))
        old, sub_x, lg = s, sx, lgN
        for r, ab in enumerate(inst.arity_bits):
            arity = 1 << ab
            ev = words[w:w + 2 * arity]
            lg -= ab
            sd = lg - inst.cap_height
            path = words[w + 2 * arity:w + 2 * arity + 4 * sd]
            coset, within = x >> ab, x & (arity - 1)
            if (int(ev[2 * within]), int(ev[2 * within + 1])) != old:
                return 5
            # compute_evaluation: interpolate {(x g^i, P(x g^i))} and evaluate at beta
            gA = oracle.root_of_unity(ab)
            start = sub_x * pow(gA, arity - brev(within, ab), P) % P
            pts = [(start * pow(gA, i, P) % P, 0) for i in range(arity)]
            vals = [(int(ev[2 * brev(i, ab)]), int(ev[2 * brev(i, ab) + 1])) for i in range(arity)]
            acc = (0, 0)
            for i in range(arity):
                num, den = (1, 0), (1, 0)
                for j in range(arity):
                    if j != i:
                        num = e_mul(num, e_sub(betas[r], pts[j]))
                        den = e_mul(den, e_sub(pts[i], pts[j]))
                acc = e_add(acc, e_mul(vals[i], e_mul(num, e_inv(den))))
            old = acc
            if not oracle.merkle_verify(ev, coset, words[r * capw:(r + 1) * capw].reshape(-1, 4), path, hasher=inst.hasher):
                return 6
            sub_x = pow(sub_x, arity, P)
            x = coset
            w += 2 * arity + 4 * sd
        acc = (0, 0)
        for cf in reversed(final):
            acc = e_add(e_scale(acc, sub_x), cf)
        if acc != old:
            return 7
    return 0


# ------------------------------------------------------------------ the plonk instance of a circuit description
def plonk_instance(desc, zeta, zk=False):
    """FriInstanceInfo of plonky2's `CommonCircuitData::get_fri_instance`: zeta opens all four oracles in full, g zeta the Z columns"""
    nch, lg = int(desc.num_challenges), int(desc.degree_bits)
    ncols = [int(desc.num_constants) + int(desc.num_routed_wires), int(desc.num_wires), nch * (1 + int(desc.num_partial_products)),
             nch * int(desc.quotient_degree_factor)]
    g = (pow(1753635133440165772, 1 << (32 - lg), P), 0)
    zeta = (int(zeta[0]), int(zeta[1]))
    points = [(zeta, [(o, 0, ncols[o]) for o in range(4)]), (e_mul(g, zeta), [(2, 0, nch)])]
    return Instance(lg, int(desc.rate_bits), int(desc.cap_height), int(getattr(desc, "hasher", 0)), ncols, [False] + [zk] * 3, points,
                    list(desc.reduction_arity_bits), int(desc.proof_of_work_bits), int(desc.num_query_rounds))


def plonk_openings_to_points(desc, op):
    """OpeningSet order of the proof (constants, sigmas, wires, zs, zs_next, partial products, quotient; [count][2]) -> the order of
    plonk_instance's points: (constants_sigmas, wires, zs, partial products, quotient), then (zs_next)"""
    op = np.asarray(op, np.uint64).reshape(-1, 2)
    nch = int(desc.num_challenges)
    a = int(desc.num_constants) + int(desc.num_routed_wires) + int(desc.num_wires) + nch
    return np.concatenate([op[:a], op[a + nch:], op[a:a + nch]])
