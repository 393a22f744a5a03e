// verifier.hip -- `CircuitData::verify(proof)` for the proofs this library produces [REF src/ecdsa/gadgets/ecdsa.rs:352,
// src/zkdsa/circuits/mod.rs:346: every reference test ends in `data.verify(proof)`].
//
// Restates plonky2 0.1.4 `plonk/verifier.rs::verify_with_challenges`, `plonk/vanishing_poly.rs::eval_vanishing_poly`,
// `gates/*::eval_unfiltered` (extension-field form), `fri/verifier.rs::{verify_fri_proof, fri_combine_initial,
// compute_evaluation}` and `hash/merkle_proofs.rs::verify_merkle_proof_to_cap`.
//
// Verification is a few thousand Poseidon permutations and one constraint evaluation at a single point: glp_verify runs on
// the host, like the transcript, and touches no device memory (the circuit handle supplies the gate table, the coset
// shifts, the digest and the constants/sigmas cap).  It shares no code with the CPU checker the tests use: the two
// verifiers and the two provers are cross-checked against each other in tests/test_gpu_prove.py.
//
// The FRI query rounds are stated twice, once per side: verify_fri_host below (glp_verify, the independent host restatement)
// and k_fri_verify_queries (verify_dev.h), the one device kernel behind glp_verify_batch (the plonk instance of a circuit) and
// glp_fri_verify* (fri_verify.inc: any instance).  Both report a failure as the same status word (FV_*), query_failure() words it.
#include <chrono>
#include <string>
#include <thread>
#include "host_pool.h"
#include "merkle.h"
#include "prover_types.h"
#include "transcript_dev.h"
#include "verify_dev.h"

namespace {

struct E {          // F_{p^2} element with operators (host only)
    ext2 v;
    E() : v(e_from(0)) {}
    E(ext2 x) : v(x) {}
    explicit E(u64 x) : v(e_from(x % P)) {}
};
inline E operator+(E a, E b) { return E(e_add(a.v, b.v)); }
inline E operator-(E a, E b) { return E(e_sub(a.v, b.v)); }
inline E operator*(E a, E b) { return E(e_mul(a.v, b.v)); }
inline E operator*(E a, u64 s) { return E(e_scale(a.v, s % P)); }
inline bool operator==(E a, E b) { return e_eq(a.v, b.v); }
inline E rd(const u64 *p) { return E(e_make(p[0], p[1])); }
inline E inv(E a) { return E(e_inv(a.v)); }
inline E epow(E a, u64 e) { return E(e_pow(a.v, e)); }
const E ONE = E((u64)1), ZERO = E((u64)0);

E range_product(E v, u32 bound) {
    E p = ONE;
    for (u32 x = 0; x < bound; x++) p = p * (v - E((u64)x));
    return p;
}
// ExtensionAlgebra<F_p^2, 2> product: (a0 + a1 Y)(b0 + b1 Y) = (a0 b0 + 7 a1 b1) + (a0 b1 + a1 b0) Y
void alg_mul(E a0, E a1, E b0, E b1, E &r0, E &r1) {
    r0 = a0 * b0 + a1 * b1 * glf::W;
    r1 = a0 * b1 + a1 * b0;
}
E sbox7(E x) { const E x2 = x * x, x4 = x2 * x2, x3 = x * x2; return x3 * x4; }
void mds(E s[12]) {     // circulant + diagonal, entries < 64: both coordinates accumulate unreduced in 128 bits, one reduction per row and coordinate
    static const u64 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    E o[12];
    for (int r = 0; r < 12; r++) {
        unsigned __int128 a = 0, b = 0;
        for (int i = 0; i < 12; i++) {
            const ext2 &x = s[(i + r) % 12].v;
            a += (unsigned __int128)x.a * C[i];
            b += (unsigned __int128)x.b * C[i];
        }
        if (r == 0) { a += (unsigned __int128)s[0].v.a * 8; b += (unsigned __int128)s[0].v.b * 8; }
        o[r] = E(e_make(reduce128((u64)a, (u64)(a >> 64)), reduce128((u64)b, (u64)(b >> 64))));
    }
    for (int r = 0; r < 12; r++) s[r] = o[r];
}

// unfiltered constraints of one gate at one point: w = local wires, gc = the gate's constants (selectors removed)
void gate_constraints(const glp_gate &g, const E *gc, const E *w, const u64 pih[4], std::vector<E> &out) {
    out.assign(g.num_constraints, ZERO);
    u32 k = 0;
    auto emit = [&](E v) { out.at(k++) = v; };
    switch (g.type) {
    case GLP_GATE_CONSTANT:
        for (u32 i = 0; i < g.p0; i++) emit(gc[i] - w[i]);
        break;
    case GLP_GATE_PUBLIC_INPUT:
        for (u32 i = 0; i < 4; i++) emit(w[i] - E(pih[i]));
        break;
    case GLP_GATE_ARITHMETIC:
        for (u32 i = 0; i < g.p0; i++) emit(w[4 * i + 3] - (w[4 * i] * w[4 * i + 1] * gc[0] + w[4 * i + 2] * gc[1]));
        break;
    case GLP_GATE_POSEIDON: {
        // wires: inputs 0..11, outputs 12..23, swap 24, delta 25..28, full_sbox_0 (rounds 1..3) from 29, partial_sbox from
        // 65, full_sbox_1 from 87; naive round schedule (same S-box inputs as plonky2's sparse form)
        const E swap = w[24];
        E st[12];
        emit(swap * (swap - ONE));
        for (int i = 0; i < 4; i++) emit(swap * (w[i + 4] - w[i]) - w[25 + i]);
        for (int i = 0; i < 4; i++) { st[i] = w[i] + w[25 + i]; st[i + 4] = w[i + 4] - w[25 + i]; }
        for (int i = 8; i < 12; i++) st[i] = w[i];
        int rc = 0;
        for (int r = 0; r < 4; r++) {
            for (int i = 0; i < 12; i++) st[i] = st[i] + E(pos::RC[rc + i]);
            rc += 12;
            if (r != 0) for (int i = 0; i < 12; i++) { const E in = w[29 + 12 * (r - 1) + i]; emit(st[i] - in); st[i] = in; }
            for (int i = 0; i < 12; i++) st[i] = sbox7(st[i]);
            mds(st);
        }
        for (int r = 0; r < 22; r++) {
            for (int i = 0; i < 12; i++) st[i] = st[i] + E(pos::RC[rc + i]);
            rc += 12;
            const E in = w[65 + r];
            emit(st[0] - in);
            st[0] = sbox7(in);
            mds(st);
        }
        for (int r = 0; r < 4; r++) {
            for (int i = 0; i < 12; i++) st[i] = st[i] + E(pos::RC[rc + i]);
            rc += 12;
            for (int i = 0; i < 12; i++) { const E in = w[87 + 12 * r + i]; emit(st[i] - in); st[i] = in; }
            for (int i = 0; i < 12; i++) st[i] = sbox7(st[i]);
            mds(st);
        }
        for (int i = 0; i < 12; i++) emit(st[i] - w[12 + i]);
        break;
    }
    case GLP_GATE_U32_INTERLEAVE:       // [REF src/u32/gates/interleave_u32.rs:84-135]
        for (u32 i = 0; i < g.p0; i++) {
            const E *bits = w + 2 * g.p0 + 32 * i;      // big-endian
            E cx = ZERO, cxi = ZERO;
            for (int b = 0; b < 32; b++) { cx = cx * (u64)2 + bits[b]; cxi = cxi * (u64)4 + bits[b]; }
            emit(cx - w[2 * i]);
            emit(cxi - w[2 * i + 1]);
            for (int b = 0; b < 32; b++) emit(bits[b] * (bits[b] - ONE));
        }
        break;
    case GLP_GATE_UNINTERLEAVE_U32:     // [REF src/u32/gates/uninterleave_to_u32.rs:93-150]
    case GLP_GATE_UNINTERLEAVE_B32:     // [REF src/u32/gates/uninterleave_to_b32.rs:95-150]
        for (u32 i = 0; i < g.p0; i++) {
            const E *bits = w + 3 * g.p0 + 64 * i;
            E cxi = ZERO, ce = ZERO, co = ZERO;
            for (int b = 0; b < 64; b++) cxi = cxi * (u64)2 + bits[b];
            for (int j = 0; j < 32; j++) {
                const u64 coeff = g.type == GLP_GATE_UNINTERLEAVE_U32 ? ((u64)1 << (31 - j)) : ((u64)1 << (2 * (31 - j)));
                ce = ce + bits[2 * j] * coeff;
                co = co + bits[2 * j + 1] * coeff;
            }
            emit(cxi - w[3 * i]);
            emit(ce - w[3 * i + 1]);
            emit(co - w[3 * i + 2]);
            for (int b = 0; b < 64; b++) emit(bits[b] * (bits[b] - ONE));
        }
        break;
    case GLP_GATE_U32_ARITHMETIC: {     // per op: m0, m1, addend, out_lo, out_hi, inverse; then 32 base-4 limbs per op
        const u32 n = g.p0;
        for (u32 i = 0; i < n; i++) {
            const E m0 = w[6 * i], m1 = w[6 * i + 1], ad = w[6 * i + 2], lo = w[6 * i + 3], hi = w[6 * i + 4], iv = w[6 * i + 5];
            emit((iv * (E((u64)0xFFFFFFFFull) - hi) - ONE) * lo);
            emit(hi * ((u64)1 << 32) + lo - (m0 * m1 + ad));
            E cl = ZERO, ch = ZERO;
            const E *limbs = w + 6 * n + 32 * i;
            for (int j = 31; j >= 0; j--) {
                emit(range_product(limbs[j], 4));
                if (j < 16) cl = cl * (u64)4 + limbs[j]; else ch = ch * (u64)4 + limbs[j];
            }
            emit(cl - lo);
            emit(ch - hi);
        }
        break;
    }
    case GLP_GATE_U32_ADD_MANY: {       // per op: addends, carry_in, result, carry_out; then 16 + 2 base-4 limbs per op
        const u32 na = g.p0, n = g.p1, wd = na + 3;
        for (u32 i = 0; i < n; i++) {
            E sum = w[wd * i + na];
            for (u32 j = 0; j < na; j++) sum = sum + w[wd * i + j];
            const E res = w[wd * i + na + 1], car = w[wd * i + na + 2];
            emit(car * ((u64)1 << 32) + res - sum);
            E cr = ZERO, cc = ZERO;
            const E *limbs = w + wd * n + 18 * i;
            for (int j = 17; j >= 0; j--) {
                emit(range_product(limbs[j], 4));
                if (j < 16) cr = cr * (u64)4 + limbs[j]; else cc = cc * (u64)4 + limbs[j];
            }
            emit(cr - res);
            emit(cc - car);
        }
        break;
    }
    case GLP_GATE_U32_SUBTRACTION: {    // per op: x, y, borrow_in, result, borrow_out; then 16 base-4 limbs per op
        const u32 n = g.p0;
        for (u32 i = 0; i < n; i++) {
            const E x = w[5 * i], y = w[5 * i + 1], bi = w[5 * i + 2], res = w[5 * i + 3], bo = w[5 * i + 4];
            emit(res - (x - y - bi + bo * ((u64)1 << 32)));
            E cl = ZERO;
            const E *limbs = w + 5 * n + 16 * i;
            for (int j = 15; j >= 0; j--) { emit(range_product(limbs[j], 4)); cl = cl * (u64)4 + limbs[j]; }
            emit(cl - res);
            emit(bo * (ONE - bo));
        }
        break;
    }
    case GLP_GATE_U32_RANGE_CHECK: {    // inputs 0..n-1, then 16 base-4 limbs per input (little-endian)
        const u32 n = g.p0;
        for (u32 i = 0; i < n; i++) {
            const E *aux = w + n + 16 * i;
            E sum = ZERO;
            for (int j = 15; j >= 0; j--) sum = sum * (u64)4 + aux[j];
            emit(sum - w[i]);
            for (int j = 0; j < 16; j++) emit(range_product(aux[j], 4));
        }
        break;
    }
    case GLP_GATE_COMPARISON: {
        const u32 nb = g.p0, ncx = g.p1, cb = (nb + ncx - 1) / ncx, cs = 1u << cb;
        const E *a = w + 4, *b = a + ncx, *ed = b + ncx, *ce = ed + ncx, *iv = ce + ncx, *mb = iv + ncx;
        E ca = ZERO, cbv = ZERO;
        for (int i = (int)ncx - 1; i >= 0; i--) { ca = ca * (u64)cs + a[i]; cbv = cbv * (u64)cs + b[i]; }
        emit(ca - w[0]);
        emit(cbv - w[1]);
        E msd = ZERO;
        for (u32 i = 0; i < ncx; i++) {
            emit(range_product(a[i], cs));
            emit(range_product(b[i], cs));
            const E diff = b[i] - a[i];
            emit(diff * ed[i] - (ONE - ce[i]));
            emit(ce[i] * diff);
            emit(iv[i] - ce[i] * msd);
            msd = iv[i] + (ONE - ce[i]) * diff;
        }
        emit(w[3] - msd);
        E bc = ZERO;
        for (u32 j = 0; j <= cb; j++) emit(mb[j] * (ONE - mb[j]));
        for (int j = (int)cb; j >= 0; j--) bc = bc * (u64)2 + mb[j];
        emit(E((u64)cs) + w[3] - bc);
        emit(w[2] - mb[cb]);
        break;
    }
    case GLP_GATE_BASE_SUM: {
        const u32 nl = g.p0, B = g.p1;
        E sum = ZERO;
        for (int j = (int)nl - 1; j >= 0; j--) sum = sum * (u64)B + w[1 + j];
        emit(sum - w[0]);
        for (u32 j = 0; j < nl; j++) emit(range_product(w[1 + j], B));
        break;
    }
    case GLP_GATE_RANDOM_ACCESS: {
        const u32 bits = g.p0, copies = g.p1 & 0xFFFF, nextra = g.p1 >> 16, vs = 1u << bits;
        const u32 routed = (2 + vs) * copies + nextra;
        for (u32 c = 0; c < copies; c++) {
            const E *base = w + (2 + vs) * c, *bw = w + routed + bits * c;
            std::vector<E> list(base + 2, base + 2 + vs);
            E idx = ZERO;
            for (u32 b = 0; b < bits; b++) emit(bw[b] * (bw[b] - ONE));
            for (int b = (int)bits - 1; b >= 0; b--) idx = idx * (u64)2 + bw[b];
            emit(idx - base[0]);
            u32 len = vs;
            for (u32 b = 0; b < bits; b++) {
                for (u32 j = 0; j < len / 2; j++) list[j] = list[2 * j] + bw[b] * (list[2 * j + 1] - list[2 * j]);
                len /= 2;
            }
            emit(list[0] - base[1]);
        }
        for (u32 e = 0; e < nextra; e++) emit(gc[e] - w[(2 + vs) * copies + e]);
        break;
    }
    // Extension-field gates at zeta: each wire opening is in F_p^2, so an ext value at wires [a, a+1] is an element of plonky2's
    // ExtensionAlgebra (w[a], w[a+1]) over F_p^2, Y^2 = 7; a constant scales both coefficients, a base coefficient lifts to (c, 0).
    // The two constraints of an op are the two algebra coefficients (recalled, unpinned: DESIGN.md).
    case GLP_GATE_ARITHMETIC_EXTENSION:
        for (u32 i = 0; i < g.p0; i++) {
            const E *o = w + 8 * i;
            E p0, p1;
            alg_mul(o[0], o[1], o[2], o[3], p0, p1);
            emit(o[6] - (p0 * gc[0] + o[4] * gc[1]));
            emit(o[7] - (p1 * gc[0] + o[5] * gc[1]));
        }
        break;
    case GLP_GATE_MUL_EXTENSION:
        for (u32 i = 0; i < g.p0; i++) {
            const E *o = w + 6 * i;
            E p0, p1;
            alg_mul(o[0], o[1], o[2], o[3], p0, p1);
            emit(o[4] - p0 * gc[0]);
            emit(o[5] - p1 * gc[0]);
        }
        break;
    case GLP_GATE_REDUCING:
    case GLP_GATE_REDUCING_EXTENSION: {
        const u32 nco = g.p0, cw = g.type == GLP_GATE_REDUCING ? 1u : 2u, accs = 6 + cw * nco;
        E a0 = w[4], a1 = w[5];
        for (u32 i = 0; i < nco; i++) {
            const E *co = w + 6 + cw * i, *ac = w + (i + 1 < nco ? accs + 2 * i : 0);
            E p0, p1;
            alg_mul(a0, a1, w[2], w[3], p0, p1);
            emit(p0 + co[0] - ac[0]);
            emit(cw == 2 ? p1 + co[1] - ac[1] : p1 - ac[1]);
            a0 = ac[0]; a1 = ac[1];
        }
        break;
    }
    // The recursion gates at zeta.  ExponentiationGate's wires are base-field targets: plain F_p^2 arithmetic on the openings.
    // CosetInterpolationGate's values, points and intermediates and PoseidonMdsGate's inputs / outputs are ext targets, i.e.
    // algebra elements on wire pairs; the shift, the domain points x_i = g^i and the weights w_i = x_i / N are scalars.
    // Exponentiation and CosetInterpolation: recalled, unpinned; PoseidonMds: pinned through the Poseidon MDS constants.
    case GLP_GATE_EXPONENTIATION: {
        const u32 nb = g.p0;
        E prev = ONE;
        for (u32 i = 0; i < nb; i++) {
            const E bit = w[nb - i], cur = w[nb + 2 + i];
            emit(prev * (bit * w[0] + ONE - bit) - cur);
            prev = cur * cur;
        }
        emit(w[nb + 1] - w[2 * nb + 1]);
        break;
    }
    case GLP_GATE_COSET_INTERPOLATION: {
        const u32 np = 1u << g.p0, d = g.p1, ni = (np - 2) / (d - 1);
        const u32 o_pt = 1 + 2 * np, o_ie = o_pt + 4, o_ip = o_ie + 2 * ni, o_sp = o_ip + 2 * ni;
        const u64 gen = root_of_unity((int)g.p0), ninv = glf::inv((u64)np);
        const E x0 = w[o_sp], x1 = w[o_sp + 1];
        emit(x0 * w[0] - w[o_pt]);
        emit(x1 * w[0] - w[o_pt + 1]);
        E e0 = ZERO, e1 = ZERO, q0 = ONE, q1 = ZERO;
        u64 xi = 1;
        u32 j = 0;
        for (u32 c = 0; c <= ni; c++) {
            const u32 end = std::min(np, d + c * (d - 1));
            for (; j < end; j++, xi = glf::mul(xi, gen)) {
                const E d0 = x0 - E(xi);
                E a0, a1, b0, b1;
                alg_mul(e0, e1, d0, x1, a0, a1);                          // eval (x - x_i)
                alg_mul(w[1 + 2 * j], w[2 + 2 * j], q0, q1, b0, b1);      // value_i prod
                const u64 wi = glf::mul(xi, ninv);
                e0 = a0 + b0 * wi; e1 = a1 + b1 * wi;
                alg_mul(q0, q1, d0, x1, a0, a1);
                q0 = a0; q1 = a1;
            }
            if (c < ni) {
                emit(w[o_ie + 2 * c] - e0); emit(w[o_ie + 2 * c + 1] - e1);
                emit(w[o_ip + 2 * c] - q0); emit(w[o_ip + 2 * c + 1] - q1);
                e0 = w[o_ie + 2 * c]; e1 = w[o_ie + 2 * c + 1]; q0 = w[o_ip + 2 * c]; q1 = w[o_ip + 2 * c + 1];
            }
        }
        emit(w[o_pt + 2] - e0);
        emit(w[o_pt + 3] - e1);
        break;
    }
    case GLP_GATE_POSEIDON_MDS: {
        E c0[12], c1[12];
        for (int i = 0; i < 12; i++) { c0[i] = w[2 * i]; c1[i] = w[2 * i + 1]; }
        mds(c0);
        mds(c1);
        for (int i = 0; i < 12; i++) { emit(w[24 + 2 * i] - c0[i]); emit(w[24 + 2 * i + 1] - c1[i]); }
        break;
    }
    default: break;    // NoopGate
    }
}

size_t brev(size_t x, int bits) {
    size_t r = 0;
    for (int i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}

// hash/merkle_proofs.rs verify_merkle_proof_to_cap
bool merkle_ok(int hasher, const u64 *leaf, size_t ncols, size_t index, const u64 *cap, const u64 *path, u32 depth) {
    u64 cur[4] = {0, 0, 0, 0};
    const bool kec25 = hasher == GLP_HASH_KECCAK25;
    if (kec25) kec::host_hash_or_noop(leaf, ncols, cur);
    else if (ncols <= 4) for (size_t i = 0; i < ncols; i++) cur[i] = leaf[i];       // hash_or_noop
    else host_hash_no_pad(leaf, ncols, cur);
    for (u32 d = 0; d < depth; d++) {
        u64 nxt[4];
        if (kec25) { if (index & 1) kec::two_to_one(path + 4 * d, cur, nxt); else kec::two_to_one(cur, path + 4 * d, nxt); }
        else if (index & 1) pos::two_to_one(path + 4 * d, cur, nxt); else pos::two_to_one(cur, path + 4 * d, nxt);
        memcpy(cur, nxt, 32);
        index >>= 1;
    }
    return memcmp(cur, cap + 4 * index, 32) == 0;
}

// What the transcript yields for the FRI half of the verification (fri/verifier.rs): challenges, the reduced openings and the
// query indices.  verify_front fills it (canonical-form check, plonk/get_challenges.rs, proof of work, the vanishing-polynomial
// identity at zeta); the query rounds then run on the host (verify_fri_host: glp_verify) or on the device (glp_verify_batch).
struct VChal {
    E zeta, zeta_next, fri_alpha, red0, red1, shift1;
    std::vector<E> fri_betas;
    std::vector<u64> x_index;
};
#define FAIL(...) return set_error(GLP_ERR_PROVE, __VA_ARGS__)
// unfiltered constraints of a gate of type GLP_GATE_PROGRAM at one point: the program read over F_p^2 (the semantics of
// glp_gate_program_eval_ext for one gate; include/glp.h, "GATE PROGRAMS IN A CIRCUIT").  lc = every constant polynomial, selectors first;
// glp_circuit_create_prog has checked every index the walk uses.
void program_constraints(const glp_circuit::Program &pr, const E *lc, const E *w, const u64 pih[4], u32 num_constraints, std::vector<E> &out) {
    out.assign(num_constraints, ZERO);
    std::vector<E> regs(pr.nregs, ZERO);
    u32 k = 0;
    auto operand = [&](u32 f) -> E {
        const u32 kind = f & 7, pl = f >> 3;
        switch (kind) {
        case GLP_GP_REG: return regs[pl];
        case GLP_GP_COL: {
            const u32 col = pl & ((1u << GLP_GP_COL_ORACLE_SHIFT) - 1);
            return pl >> GLP_GP_COL_ORACLE_SHIFT ? w[col] : lc[col];
        }
        case GLP_GP_IMM: return E(pr.pool[pl]);
        default: return E(pih[pl]);     // GLP_GP_PARAM
        }
    };
    for (const u64 ins : pr.code) {
        const u32 op = (u32)ins & 15, dst = ((u32)ins >> GLP_GP_DST_SHIFT) & 31;
        if (op == GLP_GP_OP_END) break;
        const E a = operand((u32)(ins >> GLP_GP_A_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1));
        if (op == GLP_GP_OP_EMIT) { out.at(k++) = a; continue; }
        if (op == GLP_GP_OP_MOV) { regs[dst] = a; continue; }
        const E b = operand((u32)(ins >> GLP_GP_B_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1));
        regs[dst] = op == GLP_GP_OP_ADD ? a + b : op == GLP_GP_OP_SUB ? a - b : a * b;
    }
}
// field elements (and Poseidon digests) must be canonical; a KeccakHash<25> digest is 25 bytes in a 4-word slot
int verify_canonical(const glp_circuit *cc, const u64 *proof) {
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    {
        const bool kec25 = d.hasher == GLP_HASH_KECCAK25;
        const size_t dig_lo[2] = {0, L.fri_caps}, dig_hi[2] = {L.openings, L.queries};        // cap regions
        auto in_caps = [&](size_t i) { return (i >= dig_lo[0] && i < dig_hi[0]) || (i >= dig_lo[1] && i < dig_hi[1]); };
        std::vector<unsigned char> is_dig(kec25 ? L.total : 0, 0);
        if (kec25) {
            for (size_t i = 0; i < L.queries; i++) is_dig[i] = in_caps(i);
            for (u32 q = 0; q < d.num_query_rounds; q++) {
                size_t o = L.queries + (size_t)q * L.query_stride;
                for (int k = 0; k < 4; k++) { o += L.leaf_len[k]; for (size_t j = 0; j < 4 * (size_t)L.depth0; j++) is_dig[o + j] = 1; o += 4 * (size_t)L.depth0; }
                for (u32 r = 0; r < d.num_reductions; r++) {
                    o += (size_t)2 << d.reduction_arity_bits[r];
                    for (size_t j = 0; j < 4 * (size_t)L.step_depth[r]; j++) is_dig[o + j] = 1;
                    o += 4 * (size_t)L.step_depth[r];
                }
            }
        }
        size_t run = 0;
        for (size_t i = 0; i < L.total; i++) {
            if (kec25 && is_dig[i]) { if ((run & 3) == 3 && proof[i] > 0xFF) FAIL("digest at word %zu is longer than 25 bytes", i - 3); run++; continue; }
            run = 0;
            if (proof[i] >= P) FAIL("proof word %zu is not a canonical field element", i);
        }
    }
    return GLP_OK;
}
// vanishing(zeta) == Z_H(zeta) * reduce_with_powers(quotient chunks, zeta^n)     (plonk/verifier.rs), given the challenges
int verify_vanishing(const glp_circuit *cc, const u64 *proof, const u64 *betas, const u64 *gammas, const u64 *alphas, const E &zeta, const u64 pih[4]);

int verify_vanishing(const glp_circuit *cc, const u64 *proof, const u64 *betas, const u64 *gammas, const u64 *alphas, const E &zeta, const u64 pih[4]) {
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const int lg = (int)d.degree_bits;
    const size_t n = (size_t)1 << lg;
    const u32 nch = d.num_challenges, nr = d.num_routed_wires, nw = d.num_wires, nc = d.num_constants;
    const u32 qdf = d.quotient_degree_factor, npp = d.num_partial_products, nchunks = npp + 1;
    const u64 *op = proof + L.openings;
    const u64 *p_cs = op, *p_w = op + 2 * (nc + nr), *p_zs = p_w + 2 * nw, *p_zn = p_zs + 2 * nch;
    const u64 *p_pp = p_zn + 2 * nch, *p_q = p_pp + 2 * nch * npp;
    {
        std::vector<E> lc(nc), sg(nr), lw(nw), zs(nch), zn(nch), pp((size_t)nch * npp);
        for (u32 k = 0; k < nc; k++) lc[k] = rd(p_cs + 2 * k);
        for (u32 k = 0; k < nr; k++) sg[k] = rd(p_cs + 2 * (nc + k));
        for (u32 k = 0; k < nw; k++) lw[k] = rd(p_w + 2 * k);
        for (u32 k = 0; k < nch; k++) { zs[k] = rd(p_zs + 2 * k); zn[k] = rd(p_zn + 2 * k); }
        for (u32 k = 0; k < nch * npp; k++) pp[k] = rd(p_pp + 2 * k);
        E zpow = zeta;
        for (int i = 0; i < lg; i++) zpow = zpow * zpow;
        const E zh = zpow - ONE;
        if (zeta == ONE) FAIL("zeta = 1");
        const E l0 = zh * inv((zeta - ONE) * ((u64)n % P));
        std::vector<E> terms;
        terms.reserve(nch + nch * nchunks + d.num_gate_constraints);
        for (u32 i = 0; i < nch; i++) terms.push_back(l0 * (zs[i] - ONE));
        for (u32 i = 0; i < nch; i++)
            for (u32 c = 0; c < nchunks; c++) {
                E num = ONE, den = ONE;
                for (u32 j = c * qdf; j < (c + 1) * qdf && j < nr; j++) {
                    num = num * (lw[j] + zeta * cc->k_is[j] * betas[i] + E(gammas[i]));
                    den = den * (lw[j] + sg[j] * betas[i] + E(gammas[i]));
                }
                const E prev = c == 0 ? zs[i] : pp[i * npp + c - 1];
                const E next = c == nchunks - 1 ? zn[i] : pp[i * npp + c];
                terms.push_back(prev * num - next * den);
            }
        std::vector<E> gate_terms(d.num_gate_constraints, ZERO), tmp;
        for (u32 gi = 0; gi < d.num_gates; gi++) {
            const glp_gate &g = cc->gates[gi];
            const E s = lc[g.selector_index];
            E filter = ONE;
            for (u32 i = g.group_start; i < g.group_end; i++)
                if (i != g.row) filter = filter * (E((u64)i) - s);
            if (d.num_selectors > 1) filter = filter * (E((u64)0xFFFFFFFFull) - s);       // UNUSED_SELECTOR
            if (g.type == GLP_GATE_PROGRAM) program_constraints(cc->programs[g.p0], lc.data(), lw.data(), pih, g.num_constraints, tmp);
            else gate_constraints(g, lc.data() + d.num_selectors, lw.data(), pih, tmp);
            for (u32 i = 0; i < g.num_constraints; i++) gate_terms[i] = gate_terms[i] + filter * tmp[i];
        }
        terms.insert(terms.end(), gate_terms.begin(), gate_terms.end());
        for (u32 i = 0; i < nch; i++) {
            E van = ZERO;
            for (size_t k = terms.size(); k-- > 0;) van = van * alphas[i] + terms[k];
            E t = ZERO;
            for (u32 k = qdf; k-- > 0;) t = t * zpow + rd(p_q + 2 * (i * qdf + k));
            if (!(van == zh * t)) FAIL("Mismatch between evaluation and opening of quotient polynomial (challenge %u)", i);
        }
    }
    return GLP_OK;
}

int verify_front(const glp_circuit *cc, const u64 *proof, VChal &vc) {
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const int lg = (int)d.degree_bits, rb = (int)d.rate_bits, lgN = lg + rb;
    const size_t n = (size_t)1 << lg, N = n << rb;
    const u32 nch = d.num_challenges, nr = d.num_routed_wires, nw = d.num_wires, nc = d.num_constants;
    const u32 qdf = d.quotient_degree_factor, npp = d.num_partial_products, capn = 1u << d.cap_height;
    (void)n;
    {
        const int rc0 = verify_canonical(cc, proof);
        if (rc0 != GLP_OK) return rc0;
    }

    // ---- transcript (plonk/get_challenges.rs)
    u64 pih[4];
    host_hash_no_pad(proof + L.pis, d.num_public_inputs, pih);
    Challenger ch((int)d.hasher);
    ch.observe_hashes(cc->digest, 1);
    ch.observe(pih, 4);
    ch.observe_hashes(proof + L.caps, capn);
    u64 betas[MAXCH], gammas[MAXCH], alphas[MAXCH];
    for (u32 i = 0; i < nch; i++) betas[i] = ch.get();
    for (u32 i = 0; i < nch; i++) gammas[i] = ch.get();
    ch.observe_hashes(proof + L.caps + capn * 4, capn);
    for (u32 i = 0; i < nch; i++) alphas[i] = ch.get();
    ch.observe_hashes(proof + L.caps + 2 * capn * 4, capn);
    const E zeta(ch.get_ext());
    const u64 *op = proof + L.openings;
    const u64 *p_cs = op, *p_w = op + 2 * (nc + nr), *p_zs = p_w + 2 * nw, *p_zn = p_zs + 2 * nch;
    const u64 *p_pp = p_zn + 2 * nch, *p_q = p_pp + 2 * nch * npp;
    ch.observe(p_cs, 2 * (nc + nr)); ch.observe(p_w, 2 * nw); ch.observe(p_zs, 2 * nch);
    ch.observe(p_pp, 2 * (size_t)nch * npp); ch.observe(p_q, 2 * (size_t)nch * qdf); ch.observe(p_zn, 2 * nch);
    const E fri_alpha(ch.get_ext());
    std::vector<E> fri_betas(d.num_reductions);
    for (u32 r = 0; r < d.num_reductions; r++) {
        ch.observe_hashes(proof + L.fri_caps + (size_t)r * capn * 4, capn);
        fri_betas[r] = E(ch.get_ext());
    }
    ch.observe(proof + L.final_poly, 2 * (size_t)L.final_len);
    ch.observe(proof + L.pow, 1);
    const u64 pow_resp = ch.get();
    if (d.proof_of_work_bits && (pow_resp >> (64 - d.proof_of_work_bits)) != 0) FAIL("Invalid proof of work witness.");
    {
        const int rcv = verify_vanishing(cc, proof, betas, gammas, alphas, zeta, pih);
        if (rcv != GLP_OK) return rcv;
    }

    // ---- FRI (fri/verifier.rs): reduced openings and query indices
    const E zeta_next = zeta * root_of_unity(lg);
    E red0 = ZERO, red1 = ZERO;            // PrecomputedReducedOpenings
    {
        const u64 *parts[5] = {p_cs, p_w, p_zs, p_pp, p_q};
        const size_t lens[5] = {(size_t)nc + nr, nw, nch, (size_t)nch * npp, (size_t)nch * qdf};
        E ap = ONE;
        for (int k = 0; k < 5; k++)
            for (size_t j = 0; j < lens[k]; j++) { red0 = red0 + ap * rd(parts[k] + 2 * j); ap = ap * fri_alpha; }
        ap = ONE;
        for (size_t j = 0; j < nch; j++) { red1 = red1 + ap * rd(p_zn + 2 * j); ap = ap * fri_alpha; }
    }
    vc.zeta = zeta; vc.zeta_next = zeta_next; vc.fri_alpha = fri_alpha; vc.red0 = red0; vc.red1 = red1;
    vc.shift1 = epow(fri_alpha, nch);
    vc.fri_betas = fri_betas;
    vc.x_index.resize(d.num_query_rounds);
    for (u32 q = 0; q < d.num_query_rounds; q++) vc.x_index[q] = ch.get() % (u64)N;
    (void)lgN;
#undef FAIL
    return GLP_OK;
}

// messages of the query rounds, shared by the host and the device path (word: the status word of k_fri_verify_queries, verify_dev.h)
int query_failure(u32 q, u32 word) {
    const u32 check = word & 0xFF, detail = word >> 8;
    switch (check) {
    case FV_POINT: return set_error(GLP_ERR_PROVE, "query point equals an opening point");
    case FV_INITIAL: return set_error(GLP_ERR_PROVE, "Invalid Merkle proof (query %u, initial tree %d)", q, (int)detail);
    case FV_FOLD: return set_error(GLP_ERR_PROVE, "FRI consistency check failed (query %u, reduction %u)", q, detail);
    case FV_LAYER: return set_error(GLP_ERR_PROVE, "Invalid Merkle proof (query %u, reduction %u)", q, detail);
    default: return set_error(GLP_ERR_PROVE, "Final polynomial evaluation is invalid (query %u)", q);
    }
}

int verify_fri_host(const glp_circuit *cc, const u64 *proof, const VChal &vc) {
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const int lg = (int)d.degree_bits, rb = (int)d.rate_bits, lgN = lg + rb;
    const u32 nch = d.num_challenges, capn = 1u << d.cap_height;
    const E zeta = vc.zeta, zeta_next = vc.zeta_next, fri_alpha = vc.fri_alpha, red0 = vc.red0, red1 = vc.red1, shift1 = vc.shift1;
    const std::vector<E> &fri_betas = vc.fri_betas;
#define FAIL(CHECK, DETAIL) return query_failure(q, (CHECK) | ((u32)(DETAIL) << 8))
    const u64 *caps4[4] = {cc->cs_cap.data(), proof + L.caps, proof + L.caps + capn * 4, proof + L.caps + 2 * capn * 4};
    size_t cols_total = 0;
    for (int k = 0; k < 4; k++) cols_total += L.oracle_cols[k];
    const E shift0 = epow(fri_alpha, cols_total);
    const u64 wN = root_of_unity(lgN);
    for (u32 q = 0; q < d.num_query_rounds; q++) {
        size_t x_index = (size_t)vc.x_index[q];
        const u64 *w = proof + L.queries + (size_t)q * L.query_stride;
        const u64 *evals[4];
        for (int k = 0; k < 4; k++) {
            evals[k] = w;
            // the Merkle path covers the whole leaf, salts included; fri_combine_initial reads its first oracle_cols values (unsalted_eval)
            if (!merkle_ok((int)d.hasher, w, L.leaf_len[k], x_index, caps4[k], w + L.leaf_len[k], L.depth0))
                FAIL(FV_INITIAL, k);
            w += L.leaf_len[k] + 4 * (size_t)L.depth0;
        }
        u64 subgroup_x = mul(GEN, pow(wN, (u64)brev(x_index, lgN)));
        E old_eval;
        {   // fri_combine_initial: batch 0 = every polynomial at zeta, batch 1 = the Z's at g zeta
            E r0 = ZERO, ap = ONE;
            for (int k = 0; k < 4; k++)
                for (u32 j = 0; j < L.oracle_cols[k]; j++) { r0 = r0 + ap * evals[k][j]; ap = ap * fri_alpha; }
            E r1 = ZERO;
            ap = ONE;
            for (u32 j = 0; j < nch; j++) { r1 = r1 + ap * evals[2][j]; ap = ap * fri_alpha; }
            const E sx((u64)subgroup_x);
            if (sx == zeta || sx == zeta_next) FAIL(FV_POINT, 0);
            E sum = ZERO;
            sum = sum * shift0 + (r0 - red0) * inv(sx - zeta);
            sum = sum * shift1 + (r1 - red1) * inv(sx - zeta_next);
            old_eval = sum;
        }
        for (u32 r = 0; r < d.num_reductions; r++) {
            const u32 ab = d.reduction_arity_bits[r], arity = 1u << ab;
            const u64 *ev = w, *path = w + 2 * arity;
            const size_t coset_index = x_index >> ab, within = x_index & (arity - 1);
            if (!(rd(ev + 2 * within) == old_eval)) FAIL(FV_FOLD, r);
            {   // compute_evaluation: interpolate the coset and evaluate at beta
                const u64 gA = root_of_unity((int)ab);
                const u64 coset_start = mul(subgroup_x, pow(gA, (u64)(arity - brev(within, (int)ab))));
                std::vector<E> pts(arity), vals(arity);
                u64 y = 1;
                for (u32 i = 0; i < arity; i++) {
                    pts[i] = E(mul(coset_start, y));
                    vals[i] = rd(ev + 2 * brev(i, (int)ab));
                    y = mul(y, gA);
                }
                E acc = ZERO;
                for (u32 i = 0; i < arity; i++) {
                    E num = ONE, den = ONE;
                    for (u32 j = 0; j < arity; j++)
                        if (j != i) { num = num * (fri_betas[r] - pts[j]); den = den * (pts[i] - pts[j]); }
                    acc = acc + vals[i] * num * inv(den);
                }
                old_eval = acc;
            }
            if (!merkle_ok((int)d.hasher, ev, 2 * (size_t)arity, coset_index, proof + L.fri_caps + (size_t)r * capn * 4, path, L.step_depth[r]))
                FAIL(FV_LAYER, r);
            for (u32 i = 0; i < ab; i++) subgroup_x = sqr(subgroup_x);
            x_index = coset_index;
            w += 2 * (size_t)arity + 4 * (size_t)L.step_depth[r];
        }
        E acc = ZERO;       // final_poly.eval(subgroup_x)
        for (u32 i = L.final_len; i-- > 0;) acc = acc * (u64)subgroup_x + rd(proof + L.final_poly + 2 * (size_t)i);
        if (!(acc == old_eval)) FAIL(FV_FINAL, 0);
    }
#undef FAIL
    return GLP_OK;
}
int verify_impl(const glp_circuit *cc, const u64 *proof) {
    VChal vc;
    GLP_TRY(verify_front(cc, proof, vc));
    return verify_fri_host(cc, proof, vc);
}
}  // namespace

// ------------------------------------------------------------------------------------------ query rounds on the device
// glp_verify_batch (a GPU verifier for batch self-checking; every reference driver proves and then
// verifies [REF src/zkdsa/circuits/mod.rs:341-347, src/ecdsa/gadgets/ecdsa.rs:349-352]).  Per proof the transcript, the proof of
// work and the one constraint evaluation at zeta stay on host threads (verify_front: a few dozen permutations); the query
// rounds -- K x num_query_rounds independent checks, each a few dozen to a few hundred permutations (Merkle paths of the four
// initial oracles and of every FRI layer), `fri_combine_initial`, the arity-2^k interpolations and the final polynomial -- are
// one launch of k_fri_verify_queries (verify_dev.h) on the plonk instance of the circuit: a 16-lane group per (proof, query),
// hashes in the 12-lane cooperative form (poseidon.h permute_coop: ~5x lower latency per hash than one state per lane, which is
// what matters for a chain of dependent hashes), the alpha-combination and the Lagrange terms spread over the lanes of the group.
//
// What surrounds that launch is the same for glp_verify_batch and glp_fri_verify* (fri_verify.inc) and stands here once.
namespace {
// The proofs go up (pageable host memory: the copy blocks its caller) on a thread of their own while the host half runs.  done() joins
// it; so does the destructor, when the call returns early or a host task throws.  Declared after the Scratch whose buffers it fills.
struct Uploader {
    hipError_t err = hipSuccess;
    std::thread t;
    template <class F> Uploader(glp_ctx *c, F copies) : t([this, c, copies] { err = hipSetDevice(c->device); if (err == hipSuccess) err = copies(); }) {}
    Uploader(const Uploader &) = delete;
    ~Uploader() { if (t.joinable()) t.join(); }
    int done() { t.join(); return err == hipSuccess ? GLP_OK : set_error(GLP_ERR_HIP, "upload of the proofs: %s", hipGetErrorString(err)); }
};
// every query round of every proof in one launch, timed as `stage`
int launch_queries(glp_ctx *c, int hasher, const char *stage, const FVArgs &a) {
    StageScope st(c, stage, 8.0 * a.K * a.total);
    const unsigned nblocks = (unsigned)(((size_t)a.K * a.nq + 15) / 16);
    if (hasher == GLP_HASH_KECCAK25) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fri_verify_queries<GLP_HASH_KECCAK25>), dim3(nblocks), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fri_verify_queries<GLP_HASH_POSEIDON>), dim3(nblocks), dim3(256), 0, c->stream, a);
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}
// its status words, back on the host (a copy into pageable memory blocks its caller until the stream gets there)
int read_status(glp_ctx *c, const FVArgs &a, std::vector<u32> &hs) {
    hs.resize((size_t)a.K * a.nq);
    GLP_HIP(hipMemcpyAsync(hs.data(), a.status, hs.size() * 4, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}
// why[k] is empty for the proofs the host half accepted: for those the first failing check of the first failing query becomes the
// reason (reason(q, status word)); then the verdict and the reason of every proof go out
template <class Reason>
void write_verdicts(u32 K, u32 nq, const std::vector<u32> &hs, std::vector<std::string> &why, Reason reason, int32_t *status_out, char *reasons_out) {
    for (u32 k = 0; k < K; k++) {
        for (u32 q = 0; q < nq && why[k].empty(); q++)
            if (hs[(size_t)k * nq + q]) why[k] = reason(q, hs[(size_t)k * nq + q]);
        status_out[k] = why[k].empty() ? GLP_OK : GLP_ERR_PROVE;
        if (reasons_out) {
            char *o = reasons_out + (size_t)k * GLP_REASON_LEN;
            memset(o, 0, GLP_REASON_LEN);
            strncpy(o, why[k].c_str(), GLP_REASON_LEN - 1);
        }
    }
}
}  // namespace

extern "C" int glp_verify_batch(glp_ctx *c, const glp_circuit *cc, uint32_t K, const uint64_t *proofs, int32_t *status_out, char *reasons_out) {
    GLP_REQUIRE(c && cc && proofs && status_out, "null argument");
    GLP_REQUIRE(cc->ctx == c, "circuit belongs to another context");
    GLP_REQUIRE(K >= 1 && K <= 65536, "glp_verify_batch: batch of %u proofs outside 1..65536", K);
    GLP_TRY(bind(c));
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const u32 nq = d.num_query_rounds, nred = d.num_reductions, nch = d.num_challenges, capn = 1u << d.cap_height;
    GLP_REQUIRE(L.total <= 0xFFFFFFFFu, "glp_verify_batch: proofs of %zu words (the query kernel takes a cap stride below 2^32 words)", L.total);
    // one host block: the K per-proof tables (FT_*), then the range program of the plonk instance (tests/fri_restate.py::plonk_instance):
    // every column of the four oracles at zeta (point 0), the Z columns also at g zeta (point 1)
    const u32 tstride = (FT_XIDX + nq + 3) & ~3u;
    const size_t prog_at = (size_t)K * tstride;
    u32 prog[15], leaf_off = 0;
    for (u32 o = 0; o < 4; o++) {
        prog[3 * o] = leaf_off; prog[3 * o + 1] = 0; prog[3 * o + 2] = L.oracle_cols[o];
        if (o == 2) { prog[12] = leaf_off; prog[13] = 0; prog[14] = nch; }
        leaf_off += L.leaf_len[o] + 4 * L.depth0;
    }
    std::vector<std::string> why(K);        // empty: accepted so far
    std::vector<u64> hv(prog_at + (sizeof(prog) + 7) / 8, 0);
    memcpy(&hv[prog_at], prog, sizeof(prog));
    const size_t proof_bytes = (size_t)K * L.total * 8;
    Scratch sc(c);
    u64 *dev_proofs = nullptr, *dev_hv = nullptr;
    u32 *dev_status = nullptr;
    GLP_TRY(sc.words(&dev_proofs, (size_t)K * L.total));
    GLP_TRY(sc.words(&dev_hv, hv.size()));
    GLP_TRY(sc.array(&dev_status, (size_t)K * nq));
    const bool trace = getenv("GLP_BATCH_TRACE") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    const u64 *host_prog = &hv[prog_at];
    Uploader up(c, [=] {        // the proofs, and behind them the range program: nothing waits for it on the calling thread
        hipError_t e = hipMemcpyAsync(dev_proofs, proofs, proof_bytes, hipMemcpyHostToDevice, c->stream);
        return e != hipSuccess ? e : hipMemcpyAsync(dev_hv + prog_at, host_prog, sizeof(prog), hipMemcpyHostToDevice, c->stream);
    });
    // PoseidonGoldilocksConfig: the K transcripts run on the device, as the batch prover's do (transcript_dev.h; the uploaded proofs are
    // the image its kernels read).  The host keeps the canonical-form scan (beside the upload) and the vanishing-polynomial identity
    // (beside the query rounds).  KeccakGoldilocksConfig, or GLP_VERIFY_HOST_TRANSCRIPT=1: everything of verify_front on host threads.
    const bool dev_tr = d.hasher == GLP_HASH_POSEIDON && getenv("GLP_VERIFY_HOST_TRANSCRIPT") == nullptr;
    u64 *dev_chal = nullptr, *dev_qpp = nullptr, *dev_apow = nullptr, *dev_zetas = nullptr;
    u32 *dev_err = nullptr;
    std::vector<u64> h_back;
    const u64 *h_chal = nullptr, *h_qpp = nullptr, *h_apow = nullptr, *h_zetas = nullptr;
    const u32 *h_err = nullptr;
    hipEvent_t ev_chal = nullptr;
    struct EvGuard { hipEvent_t &e; ~EvGuard() { if (e) (void)hipEventDestroy(e); } } evg{ev_chal};
    double t_front = 0, t_up = 0;
    if (!dev_tr) {
        // host half, one proof per task on the context's pool: canonical form, transcript, proof of work, vanishing polynomial at zeta
        ctx_host_pool(c).run(K, [&](size_t k) {
            VChal v;
            if (verify_front(cc, proofs + k * L.total, v) != GLP_OK) { why[k] = g_last_error; return; }
            u64 *o = &hv[k * tstride];
            auto put = [&](u32 at, const E &e) { o[at] = e.v.a; o[at + 1] = e.v.b; };
            put(FT_ALPHA, v.fri_alpha); put(FT_Z, v.zeta); put(FT_Z + 2, v.zeta_next); put(FT_RED, v.red0); put(FT_RED + 2, v.red1);
            for (u32 r = 0; r < nred; r++) put(FT_BETAS + 2 * r, v.fri_betas[r]);
            for (u32 q = 0; q < nq; q++) o[FT_XIDX + q] = v.x_index[q];
        });
        // device half: every query round of every proof in one launch.  Proofs the host half already rejected still ride along
        // (their slots hold zero challenges and every index is in range); their device status is ignored.
        t_front = since();
        GLP_TRY(up.done());
        t_up = since();
        GLP_HIP(hipMemcpyAsync(dev_hv, hv.data(), prog_at * 8, hipMemcpyHostToDevice, c->stream));
    } else {
        ctx_host_pool(c).run(K, [&](size_t k) {
            if (verify_canonical(cc, proofs + k * L.total) != GLP_OK) why[k] = g_last_error;
        });
        t_front = since();
        GLP_TRY(up.done());
        t_up = since();
        const u32 total_cols = L.oracle_cols[0] + L.oracle_cols[1] + L.oracle_cols[2] + L.oracle_cols[3];
        u64 *dch, *dev_apl, *dev_fap, *dev_fpp, *dev_betas, *dev_idx;
        GLP_TRY(sc.words(&dch, (size_t)K * DCH_WORDS));
        // betas | gammas, public-input hash, alpha powers, zetas, error bits: one block, one copy back
        const size_t w_chal = (size_t)K * 2 * MAXCH, w_qpp = (size_t)K * 3 * MAXCH, w_apow = (size_t)K * nch * 2, w_zetas = (size_t)K * 4, w_err = (K + 1) / 2;
        u64 *dev_back;
        GLP_TRY(sc.words(&dev_back, w_chal + w_qpp + w_apow + w_zetas + w_err));
        dev_chal = dev_back; dev_qpp = dev_chal + w_chal; dev_apow = dev_qpp + w_qpp; dev_zetas = dev_apow + w_apow; dev_err = (u32 *)(dev_zetas + w_zetas);
        GLP_TRY(sc.words(&dev_apl, (size_t)K * nch * 2 * APL_WORDS));
        GLP_TRY(sc.words(&dev_fap, (size_t)K * 2 * total_cols));
        GLP_TRY(sc.words(&dev_fpp, (size_t)K * 10));
        GLP_TRY(sc.words(&dev_betas, (size_t)std::max<u32>(nred, 1) * K * 2));
        GLP_TRY(sc.words(&dev_idx, (size_t)K * nq));
        GLP_HIP(hipMemsetAsync(dev_back, 0, (w_chal + w_qpp + w_apow + w_zetas + w_err) * 8, c->stream));
        TrGeo g;
        g.dch = dch; g.image = dev_proofs; g.total = L.total; g.K = K; g.capn = capn; g.nch = nch;
        const dim3 tg((K + 15) / 16), tb(256);
        const size_t cap4 = (size_t)capn * 4;
        // a cap is "copied" from the image onto itself: source = image + offset with the proof stride, destination offset the same
        hipLaunchKernelGGL(k_tr_begin, tg, tb, 0, c->stream, g, cc->digest[0], cc->digest[1], cc->digest[2], cc->digest[3], L.pis, d.num_public_inputs,
                           dev_proofs + L.caps, L.total, L.caps, dev_chal, dev_qpp);
        hipLaunchKernelGGL(k_tr_alphas, tg, tb, 0, c->stream, g, dev_proofs + L.caps + cap4, L.total, L.caps + cap4, 2u, dev_apow, dev_apl);
        hipLaunchKernelGGL(k_tr_zeta, tg, tb, 0, c->stream, g, dev_proofs + L.caps + 2 * cap4, L.total, L.caps + 2 * cap4, d.degree_bits,
                           root_of_unity((int)d.degree_bits), dev_zetas, dev_err);
        OpenGeo og;
        memset(&og, 0, sizeof(og));
        for (int b = 0; b < 4; b++) og.cols[b] = L.oracle_cols[b];
        og.openings_off = L.openings; og.nch = nch; og.npp = d.num_partial_products; og.nopen = (u32)L.nopen;
        hipLaunchKernelGGL(k_tr_fri_alpha, tg, tb, 0, c->stream, g, og, dev_zetas, dev_fap, dev_fpp);
        for (u32 r = 0; r < nred; r++)
            hipLaunchKernelGGL(k_tr_beta, tg, tb, 0, c->stream, g, dev_proofs + L.fri_caps + r * cap4, L.total, L.fri_caps + r * cap4, dev_betas + (size_t)r * K * 2);
        hipLaunchKernelGGL(k_trv_final, tg, tb, 0, c->stream, g, L.final_poly, 2u * L.final_len);
        hipLaunchKernelGGL(k_trv_queries, tg, tb, 0, c->stream, g, d.proof_of_work_bits, L.pow, nq, (u64)1 << (d.degree_bits + d.rate_bits), dev_idx, dev_err);
        hipLaunchKernelGGL(k_trv_pack, dim3((K + 255) / 256), dim3(256), 0, c->stream, K, tstride, dev_fap, total_cols, dev_fpp, dev_betas, nred, dev_idx, nq, dev_hv);
        GLP_HIP(hipGetLastError());
        // what the host's half of the check needs comes back while the query rounds run
        h_back.resize(w_chal + w_qpp + w_apow + w_zetas + w_err);
        GLP_HIP(hipMemcpyAsync(h_back.data(), dev_back, h_back.size() * 8, hipMemcpyDeviceToHost, c->stream));
        GLP_HIP(hipEventCreateWithFlags(&ev_chal, hipEventDisableTiming));
        GLP_HIP(hipEventRecord(ev_chal, c->stream));
        h_chal = h_back.data(); h_qpp = h_chal + w_chal; h_apow = h_qpp + w_qpp; h_zetas = h_apow + w_apow; h_err = (const u32 *)(h_zetas + w_zetas);
    }
    // the FRI part of a proof, fri_caps | queries | final_poly | pow, is the FriProof layout the kernel reads (layer caps at offset 0); the
    // circuit's constants / sigmas cap is shared, the three caps of a proof sit at its front
    FVArgs a;
    memset(&a, 0, sizeof(a));
    a.proofs = dev_proofs + L.fri_caps; a.table = dev_hv; a.prog = (const u32 *)(dev_hv + prog_at); a.status = dev_status;
    a.total = L.total; a.queries = L.queries - L.fri_caps; a.query_stride = L.query_stride; a.final_poly = L.final_poly - L.fri_caps;
    a.tstride = tstride; a.nq = nq; a.K = K; a.lgN = d.degree_bits + d.rate_bits; a.cap_height = d.cap_height; a.depth0 = L.depth0; a.nred = nred;
    a.final_len = L.final_len; a.nor = 4; a.npts = 2; a.nranges[0] = 4; a.nranges[1] = 1;
    a.caps[0] = cc->cs->digests + 4 * merkle_cap_offset((size_t)1 << a.lgN, (int)d.cap_height);
    for (u32 o = 1; o < 4; o++) { a.caps[o] = dev_proofs + L.caps + (size_t)(o - 1) * capn * 4; a.cap_stride[o] = (u32)L.total; }
    for (u32 o = 0; o < 4; o++) a.leaf_len[o] = L.leaf_len[o];
    for (u32 r = 0; r < nred; r++) { a.ab[r] = d.reduction_arity_bits[r]; a.step_depth[r] = L.step_depth[r]; a.gA[r] = root_of_unity((int)d.reduction_arity_bits[r]); }
    a.wN = root_of_unity((int)a.lgN);
    GLP_TRY(launch_queries(c, (int)d.hasher, "verify_queries", a));
    double t_chal = 0, t_van = 0;
    if (dev_tr) {
        GLP_HIP(hipEventSynchronize(ev_chal));
        t_chal = since();
        // same order of checks as verify_front: canonical form (above), proof of work, then the identity at zeta
        ctx_host_pool(c).run(K, [&](size_t k) {
            if (!why[k].empty()) return;
            if (h_err[k] & 8u) { set_error(GLP_ERR_PROVE, "Invalid proof of work witness."); why[k] = g_last_error; return; }
            u64 alphas[MAXCH] = {0, 0, 0, 0};
            for (u32 i = 0; i < nch; i++) alphas[i] = h_apow[(k * nch + i) * 2 + 1];
            const E zeta(e_make(h_zetas[4 * k], h_zetas[4 * k + 1]));
            if (verify_vanishing(cc, proofs + k * L.total, &h_chal[k * 2 * MAXCH], &h_chal[k * 2 * MAXCH + MAXCH], alphas, zeta, &h_qpp[k * 3 * MAXCH + 2 * MAXCH]) != GLP_OK)
                why[k] = g_last_error;
        });
        t_van = since();
    }
    // (enqueued only now: the identity at zeta ran beside the query rounds)
    std::vector<u32> hs;
    GLP_TRY(read_status(c, a, hs));
    if (trace) {
        if (dev_tr) fprintf(stderr, "[glp_verify_batch K=%u dev] canonical scan %.3f ms | upload done at %.3f | challenges back at %.3f | identity at zeta done at %.3f | query rounds done at %.3f ms\n",
                            K, t_front, t_up, t_chal, t_van, since());
        else fprintf(stderr, "[glp_verify_batch K=%u] host half %.3f ms | upload done at %.3f | query rounds done at %.3f ms\n", K, t_front, t_up, since());
    }
    write_verdicts(K, nq, hs, why, [](u32 q, u32 word) { query_failure(q, word); return g_last_error; }, status_out, reasons_out);
    return GLP_OK;
}

extern "C" int glp_verify(const glp_circuit *cc, const uint64_t *proof_words) {
    GLP_REQUIRE(cc && proof_words, "null argument");
    return verify_impl(cc, proof_words);
}
// Same, with the caller's buffer length stated: a truncated or over-long buffer is an argument error, never a read past it.
extern "C" int glp_verify_n(const glp_circuit *cc, const uint64_t *proof_words, size_t num_words) {
    GLP_REQUIRE(cc && proof_words, "null argument");
    GLP_REQUIRE(num_words == cc->L.total, "proof has %zu words, a proof of this circuit has %zu", num_words, (size_t)cc->L.total);
    return verify_impl(cc, proof_words);
}

#include "fri_verify.inc"
