// biguint_dev.h -- integer arithmetic on little-endian u32 limbs for the free units of witness generation (include/glp.h, "witness
// generation, the dataflow half": GLP_WGEN_*), one text for the device (witness.hip) and for a plain host program
// (examples/biguint_host.cpp, which tests/test_biguint_host.py compares with Python integers).
//
// What is restated: the `run_once` bodies of the reference's generators that belong to no gate
//   NonNativeAddition / MultipleAdds / Subtraction / Multiplication / Inverse Generator   [REF src/ecdsa/gadgets/nonnative.rs:475-490,
//                                                                                          553-576, 648-663, 727-740, 797-809]
//   BigUintDivRemGenerator                                                                 [REF src/ecdsa/gadgets/biguint.rs:342-349]
//   GLVDecompositionGenerator = decompose_secp256k1_scalar       [REF src/ecdsa/gadgets/glv.rs:122-133, src/ecdsa/curve/glv.rs:38-77]
// Inputs outside a generator's domain (the Rust code panics there) give the fixed results include/glp.h states; nothing here can spin:
// every loop has a trip count given by limb counts or a compile-time bound (the division corrects a digit at most twice, the inverse
// is a binary extended GCD capped at its worst case of 64 steps per limb of the modulus), and nothing read from a witness
// becomes a cell.  One count does come from values: BIGUINT_DIV_REM divides by the divisor's limbs up to its highest non-zero one, which
// indexes the local arrays of the division and sets its trip counts, bounded by the declared limb count (at most 8).
//
// Lengths.  A template argument C* >= 0 fixes a limb count at compile time: with every count fixed and the loops unrolled, the arrays
// below are only ever indexed by constants and live in registers.  C* = -1 takes the count from the argument beside it; those
// instances index by loop variables and their arrays go to scratch on the device (the general-length instance).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BIG_HD __host__ __device__ inline
#else
#define BIG_HD inline
#endif
// BIG_UNROLL asks for the full unrolling of a loop only in an instance whose counts are compile-time constants: U, a constant of the
// enclosing function, is 32 there (above every limb count, so the loop is unrolled whole) and 1, "leave the loop alone", where the
// count comes at run time.  A loop of a compile-time instance that is not unrolled is then a compiler warning, and no other loop is.
#if defined(__clang__)
#define BIG_UNROLL _Pragma("clang loop unroll_count(U)")
#else
#define BIG_UNROLL
#endif
#define BIG_U(constant) constexpr int U = (constant) ? 32 : 1; (void)U

namespace big {

constexpr int MAX_LIMBS = 18;     // an operand (GLP_WGEN_MAX_LIMBS)
constexpr int MAX_MOD = 8;        // a modulus or a divisor

// the kinds of include/glp.h
constexpr uint32_t K_EQUALITY = 1, K_ADD = 2, K_MULTI_ADD = 3, K_SUB = 4, K_MUL = 5, K_INV = 6, K_DIV_REM = 7, K_GLV = 8;

// the two correction branches of the division, counted by the host program; `twice`: the digits whose estimate was corrected both times
struct Stats { uint64_t qhat_corrections, add_backs, twice; };

template <int CN> BIG_HD void zero(uint32_t *r, int n_) {
    const int n = CN >= 0 ? CN : n_;
    BIG_U(CN >= 0);
    BIG_UNROLL for (int i = 0; i < n; i++) r[i] = 0;
}
template <int CN> BIG_HD void copy(uint32_t *r, const uint32_t *a, int n_) {
    const int n = CN >= 0 ? CN : n_;
    BIG_U(CN >= 0);
    BIG_UNROLL for (int i = 0; i < n; i++) r[i] = a[i];
}
// r = a + b, returns the carry; r may be a or b
template <int CN> BIG_HD uint32_t add(uint32_t *r, const uint32_t *a, const uint32_t *b, int n_) {
    const int n = CN >= 0 ? CN : n_;
    BIG_U(CN >= 0);
    uint64_t c = 0;
    BIG_UNROLL for (int i = 0; i < n; i++) { c += (uint64_t)a[i] + b[i]; r[i] = (uint32_t)c; c >>= 32; }
    return (uint32_t)c;
}
// r = a - b, returns the borrow; r may be a or b
template <int CN> BIG_HD uint32_t sub(uint32_t *r, const uint32_t *a, const uint32_t *b, int n_) {
    const int n = CN >= 0 ? CN : n_;
    BIG_U(CN >= 0);
    uint64_t bo = 0;
    BIG_UNROLL for (int i = 0; i < n; i++) { const uint64_t t = (uint64_t)a[i] - b[i] - bo; r[i] = (uint32_t)t; bo = (t >> 32) & 1; }
    return (uint32_t)bo;
}
// a >= b
template <int CN> BIG_HD bool geq(const uint32_t *a, const uint32_t *b, int n_) {
    const int n = CN >= 0 ? CN : n_;
    BIG_U(CN >= 0);
    uint64_t bo = 0;
    BIG_UNROLL for (int i = 0; i < n; i++) bo = (((uint64_t)a[i] - b[i] - bo) >> 32) & 1;
    return bo == 0;
}
template <int CN> BIG_HD bool is_zero(const uint32_t *a, int n_) {
    const int n = CN >= 0 ? CN : n_;
    BIG_U(CN >= 0);
    uint32_t o = 0;
    BIG_UNROLL for (int i = 0; i < n; i++) o |= a[i];
    return o == 0;
}
// a >>= 1 with `top` shifted into the highest bit
template <int CN> BIG_HD void shr1(uint32_t *a, uint32_t top, int n_) {
    const int n = CN >= 0 ? CN : n_;
    BIG_U(CN >= 0);
    BIG_UNROLL for (int i = 0; i < n; i++) a[i] = (a[i] >> 1) | ((i + 1 < n ? a[i + 1] : top) << 31);
}
// schoolbook product r[na + nb] = a * b
template <int CNA, int CNB> BIG_HD void mul(uint32_t *r, const uint32_t *a, int na_, const uint32_t *b, int nb_) {
    const int na = CNA >= 0 ? CNA : na_, nb = CNB >= 0 ? CNB : nb_;
    BIG_U(CNA >= 0 && CNB >= 0);
    BIG_UNROLL for (int i = 0; i < na + nb; i++) r[i] = 0;
    BIG_UNROLL for (int i = 0; i < na; i++) {
        uint64_t c = 0;
        BIG_UNROLL for (int j = 0; j < nb; j++) { c += (uint64_t)a[i] * b[j] + r[i + j]; r[i + j] = (uint32_t)c; c >>= 32; }
        r[i + nb] = (uint32_t)c;
    }
}

// Long division (Knuth D): q[na] = a / b, r[nb] = a % b for 1 <= nb <= MAX_MOD, na <= MAX_LIMBS and b[nb - 1] != 0.  A quotient digit
// is estimated from the two leading limbs, corrected at most twice against the third, and once more (the add-back) when the
// multiply-subtract still borrows.
template <int CNA, int CNB> BIG_HD void divrem(uint32_t *q, uint32_t *r, const uint32_t *a, int na_, const uint32_t *b, int nb_, Stats *st) {
    const int na = CNA >= 0 ? CNA : na_, nb = CNB >= 0 ? CNB : nb_;
    BIG_U(CNA >= 0 && CNB >= 0);
    if (na < nb) {
        BIG_UNROLL for (int i = 0; i < na; i++) q[i] = 0;
        BIG_UNROLL for (int i = 0; i < nb; i++) r[i] = i < na ? a[i] : 0;
        return;
    }
    uint32_t un[MAX_LIMBS + 1], vn[MAX_MOD];
    const int s = __builtin_clz(b[nb - 1]);
    BIG_UNROLL for (int i = 0; i < nb; i++) vn[i] = (uint32_t)(((((uint64_t)b[i] << 32) | (i ? b[i - 1] : 0)) << s) >> 32);
    BIG_UNROLL for (int i = 0; i < na; i++) un[i] = (uint32_t)(((((uint64_t)a[i] << 32) | (i ? a[i - 1] : 0)) << s) >> 32);
    un[na] = (uint32_t)(((uint64_t)a[na - 1] << s) >> 32);
    const uint64_t B = (uint64_t)1 << 32, vtop = vn[nb - 1], vsec = nb >= 2 ? vn[nb >= 2 ? nb - 2 : 0] : 0;
    BIG_UNROLL for (int i = na - nb + 1; i < na; i++) q[i] = 0;
    BIG_UNROLL for (int j = na - nb; j >= 0; j--) {
        const uint64_t num = ((uint64_t)un[j + nb] << 32) | un[j + nb - 1];
        uint64_t qhat = num / vtop, rhat = num % vtop;
        const uint64_t u3 = nb >= 2 ? un[j + (nb >= 2 ? nb - 2 : 0)] : 0;
        BIG_UNROLL for (int t = 0; t < 2; t++)
            if (rhat < B && (qhat >= B || qhat * vsec > ((rhat << 32) | u3))) {
                qhat--; rhat += vtop;
                if (st) { st->qhat_corrections++; st->twice += t; }       // a correction at t = 1 follows one at t = 0: without it nothing changed
            }
        int64_t k = 0, t = 0;                        // un[j .. j + nb] -= qhat * vn
        BIG_UNROLL for (int i = 0; i < nb; i++) {
            const uint64_t p = qhat * vn[i];
            t = (int64_t)un[i + j] - k - (int64_t)(p & 0xFFFFFFFFull);
            un[i + j] = (uint32_t)t;
            k = (int64_t)(p >> 32) - (t >> 32);
        }
        t = (int64_t)un[j + nb] - k;
        un[j + nb] = (uint32_t)t;
        if (t < 0) {                                 // one too many: add the divisor back
            qhat--;
            uint64_t c = 0;
            BIG_UNROLL for (int i = 0; i < nb; i++) { c += (uint64_t)un[i + j] + vn[i]; un[i + j] = (uint32_t)c; c >>= 32; }
            un[j + nb] += (uint32_t)c;
            if (st) st->add_backs++;
        }
        q[j] = (uint32_t)qhat;
    }
    BIG_UNROLL for (int i = 0; i < nb; i++) r[i] = (uint32_t)(((((uint64_t)un[i + 1] << 32) | un[i]) >> s));
}

// number of limbs up to the highest non-zero one (0 for zero), n <= MAX_LIMBS
BIG_HD int used_limbs(const uint32_t *a, int n) {
    int u = 0;
    for (int i = 0; i < n; i++) if (a[i]) u = i + 1;
    return u;
}

// r[nm] = a mod m for a modulus of nm limbs with m[nm - 1] != 0 (`from_noncanonical_biguint`)
template <int CNA, int CNM> BIG_HD void reduce(uint32_t *r, const uint32_t *a, int na_, const uint32_t *m, int nm_, Stats *st) {
    uint32_t q[MAX_LIMBS];
    divrem<CNA, CNM>(q, r, a, na_, m, nm_, st);
}

// inv[nm] = x^-1 mod m for odd m >= 3 and x < m; returns false (inv = 0) when x = 0 or gcd(x, m) != 1.  Binary extended GCD with
// a = u x, b = v x (mod m): a step halves a (and u modulo m), after subtracting the smaller odd number if a is odd; every step takes a
// bit off a or b, so 64 steps per limb is the worst case and the loop is capped there.
template <int CNM> BIG_HD bool modinv(uint32_t *inv, const uint32_t *x, const uint32_t *m, int nm_) {
    const int nm = CNM >= 0 ? CNM : nm_;
    BIG_U(CNM >= 0);
    uint32_t a[MAX_MOD], b[MAX_MOD], u[MAX_MOD], v[MAX_MOD];
    copy<CNM>(a, x, nm); copy<CNM>(b, m, nm); zero<CNM>(u, nm); zero<CNM>(v, nm);
    u[0] = 1;
    for (int step = 0; step < 64 * nm; step++) {
        if (is_zero<CNM>(a, nm)) continue;           // done: the remaining steps do nothing
        if (a[0] & 1) {
            if (!geq<CNM>(a, b, nm)) {
                BIG_UNROLL for (int i = 0; i < nm; i++) { const uint32_t ta = a[i], tu = u[i]; a[i] = b[i]; b[i] = ta; u[i] = v[i]; v[i] = tu; }
            }
            sub<CNM>(a, a, b, nm);
            if (sub<CNM>(u, u, v, nm)) add<CNM>(u, u, m, nm);      // u - v mod m
        }
        shr1<CNM>(a, 0, nm);
        uint32_t top = 0;
        if (u[0] & 1) top = add<CNM>(u, u, m, nm);                 // (u + m) / 2: m is odd
        shr1<CNM>(u, top, nm);
    }
    bool one = b[0] == 1 && is_zero<CNM>(a, nm);
    BIG_UNROLL for (int i = 1; i < nm; i++) one = one && b[i] == 0;
    BIG_UNROLL for (int i = 0; i < nm; i++) inv[i] = one ? v[i] : 0;
    return one;
}

// ---- secp256k1's GLV decomposition [REF src/ecdsa/curve/glv.rs:11-77]; the constants are the reference's u64 limbs, split
struct Glv {
    uint32_t n[8], half[8], a1[4], minus_b1[4], a2[5];
};
BIG_HD Glv glv_constants() {
    Glv g = {{0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
             {0x681B20A0u, 0xDFE92F46u, 0x57A4501Du, 0x5D576E73u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu},      // n / 2
             {0x9284EB15u, 0xE86C90E4u, 0xA7D46BCDu, 0x3086D221u},                                  // A1 = B2
             {0x0ABFE4C3u, 0x6F547FA9u, 0x010E8828u, 0xE4437ED6u},                                  // MINUS_B1
             {0x9D44CFD8u, 0x57C1108Du, 0xA8E2F3F6u, 0x14CA50F7u, 1u}};                             // A2
    return g;
}
// r[8] = round(c * k / n) mod n for a constant c of 4 limbs: the rounding division of Ratio::round (n is odd: no ties)
BIG_HD void glv_round(uint32_t *r, const uint32_t *c, const uint32_t *k, const Glv &g, Stats *st) {
    uint32_t p[12], q[12], rem[8], twice[9];
    mul<-1, -1>(p, c, 4, k, 8);
    divrem<-1, -1>(q, rem, p, 12, g.n, 8, st);
    twice[8] = add<-1>(twice, rem, rem, 8);
    const bool up = twice[8] || !geq<-1>(g.n, twice, 8);          // 2 rem > n
    uint32_t carry = up ? 1 : 0;
    for (int i = 0; i < 12; i++) { const uint64_t t = (uint64_t)q[i] + carry; q[i] = (uint32_t)t; carry = (uint32_t)(t >> 32); }
    uint32_t qq[12];
    divrem<-1, -1>(qq, r, q, 12, g.n, 8, st);                      // from_noncanonical_biguint
}
// r[8] = a[na] * b[nb] mod n, na + nb <= MAX_LIMBS
BIG_HD void glv_mulmod(uint32_t *r, const uint32_t *a, int na, const uint32_t *b, int nb, const Glv &g, Stats *st) {
    uint32_t p[MAX_LIMBS], q[MAX_LIMBS];
    mul<-1, -1>(p, a, na, b, nb);
    divrem<-1, -1>(q, r, p, na + nb, g.n, 8, st);
}
BIG_HD void glv_submod(uint32_t *r, const uint32_t *a, const uint32_t *b, const Glv &g) {     // a - b mod n for a, b < n
    if (sub<-1>(r, a, b, 8)) add<-1>(r, r, g.n, 8);
}
// k[8] (any value: reduced first) -> |k1|, |k2| (8 limbs each; the generator's targets have 4) and the two signs
BIG_HD void glv_decompose(uint32_t *k1, uint32_t *k2, uint32_t *k1_neg, uint32_t *k2_neg, const uint32_t *k_in, Stats *st) {
    const Glv g = glv_constants();
    uint32_t k[8], c1[8], c2[8], t[8], u[8];
    reduce<-1, -1>(k, k_in, 8, g.n, 8, st);
    glv_round(c1, g.a1, k, g, st);                   // B2 = A1
    glv_round(c2, g.minus_b1, k, g, st);
    glv_mulmod(t, c1, 8, g.a1, 4, g, st);
    glv_submod(k1, k, t, g);
    glv_mulmod(t, c2, 8, g.a2, 5, g, st);
    glv_submod(k1, k1, t, g);                        // k1 = k - c1 A1 - c2 A2
    glv_mulmod(t, c1, 8, g.minus_b1, 4, g, st);
    glv_mulmod(u, c2, 8, g.a1, 4, g, st);
    glv_submod(k2, t, u, g);                         // k2 = c1 MINUS_B1 - c2 B2
    *k1_neg = !geq<-1>(g.half, k1, 8);               // k1 > n / 2
    if (*k1_neg) sub<-1>(k1, g.n, k1, 8);
    *k2_neg = !geq<-1>(g.half, k2, 8);
    if (*k2_neg) sub<-1>(k2, g.n, k2, 8);
}

// how many cells of a unit's run are inputs and outputs (the operand orders of include/glp.h)
BIG_HD uint32_t num_in(uint32_t kind, const uint16_t *len) {
    switch (kind) {
    case K_MULTI_ADD: return (uint32_t)len[0] * len[1];
    case K_INV: case K_GLV: return len[0];
    default: return (uint32_t)len[0] + len[1];
    }
}
BIG_HD uint32_t num_out(uint32_t kind, const uint16_t *len) {
    switch (kind) {
    case K_INV: return (uint32_t)len[1] + len[2];
    case K_GLV: return (uint32_t)len[1] + len[2] + len[3] + len[4];
    default: return (uint32_t)len[2] + len[3];
    }
}

// the instance with every count a compile-time 8: an 8-limb modulus and 8-limb operands (ADD, SUB: a, b, sum; MUL: and overflow; INV: x,
// inv, div) -- what the secp256k1 gadgets emit almost everywhere
BIG_HD bool all8(uint32_t kind, const uint16_t *len, int nm) {
    if (nm != 8 || len[0] != 8 || len[1] != 8 || len[2] != 8) return false;
    return kind == K_INV || (kind == K_MUL && len[3] == 8) || ((kind == K_ADD || kind == K_SUB) && len[3] == 1);
}

// ---- one free unit.  RD rd(i): limb i of the unit's inputs in the order of its cell run (the low 32 bits of the cell); WR wr(i, v):
// output cell i of the run gets the u32 v.  len[] is the unit's operand lengths (include/glp.h), m[8] / nm its modulus with m[nm - 1]
// != 0 (kinds 2..6).  C8 = true is the instance for an 8-limb modulus with every operand 8 limbs long (kinds ADD, SUB, MUL, INV): all
// counts are compile-time constants.  EQUALITY is field arithmetic and is not here.
template <int CN, class WR> BIG_HD void store(WR &wr, int at, const uint32_t *v, int have_, int want_) {
    BIG_U(CN >= 0);
    const int have = CN >= 0 ? CN : have_, want = CN >= 0 ? CN : want_;      // a result wider than its cells is truncated, a narrower one padded
    BIG_UNROLL for (int i = 0; i < want; i++) wr(at + i, i < have ? v[i] : 0u);
}
template <bool C8, class RD, class WR>
BIG_HD void run_unit(uint32_t kind, const uint16_t *len, const uint32_t *m, int nm_, RD rd, WR wr, Stats *st) {
    constexpr int CN = C8 ? 8 : -1, C2N = C8 ? 16 : -1;
    BIG_U(C8);
    const int nm = C8 ? 8 : nm_;
    uint32_t a[MAX_LIMBS], b[MAX_LIMBS], ra[MAX_MOD + 1], rb[MAX_MOD + 1];
    const int la = C8 ? 8 : len[0], lb = C8 ? 8 : len[1];
    if (kind == K_ADD || kind == K_SUB || kind == K_MUL) {
        BIG_UNROLL for (int i = 0; i < la; i++) a[i] = rd(i);
        BIG_UNROLL for (int i = 0; i < lb; i++) b[i] = rd(la + i);
        reduce<CN, CN>(ra, a, la, m, nm, st);
        reduce<CN, CN>(rb, b, lb, m, nm, st);
    }
    switch (kind) {
    case K_ADD: {                                    // overflow iff a + b > m, strictly: a + b = m gives sum = m
        ra[nm] = add<CN>(ra, ra, rb, nm);
        const bool over = ra[nm] || (geq<CN>(ra, m, nm) && !geq<CN>(m, ra, nm));
        if (over) sub<CN>(ra, ra, m, nm);
        store<CN, WR>(wr, 0, ra, nm, len[2]);
        wr(C8 ? 8 : len[2], over ? 1u : 0u);
        break;
    }
    case K_SUB: {
        const bool over = sub<CN>(ra, ra, rb, nm) != 0;
        if (over) add<CN>(ra, ra, m, nm);
        store<CN, WR>(wr, 0, ra, nm, len[2]);
        wr(C8 ? 8 : len[2], over ? 1u : 0u);
        break;
    }
    case K_MUL: {
        uint32_t p[2 * MAX_MOD], q[2 * MAX_MOD];
        mul<CN, CN>(p, ra, nm, rb, nm);
        divrem<C2N, CN>(q, ra, p, 2 * nm, m, nm, st);
        store<CN, WR>(wr, 0, ra, nm, len[2]);
        store<CN, WR>(wr, C8 ? 8 : len[2], q, 2 * nm, len[3]);
        break;
    }
    case K_INV: {                                    // in: x   out: inv, div = floor(x inv / m); both 0 when there is no inverse
        uint32_t p[2 * MAX_MOD], q[2 * MAX_MOD], inv[MAX_MOD];
        BIG_UNROLL for (int i = 0; i < la; i++) a[i] = rd(i);
        reduce<CN, CN>(ra, a, la, m, nm, st);
        modinv<CN>(inv, ra, m, nm);
        mul<CN, CN>(p, ra, nm, inv, nm);
        divrem<C2N, CN>(q, rb, p, 2 * nm, m, nm, st);
        store<CN, WR>(wr, 0, inv, nm, len[1]);
        store<CN, WR>(wr, C8 ? 8 : len[1], q, 2 * nm, len[2]);
        break;
    }
    default: break;
    }
    if (C8) return;
    switch (kind) {
    case K_MULTI_ADD: {                              // len[0] summands of len[1] limbs, each reduced; overflow = the quotient's low limb
        uint32_t acc[MAX_MOD + 1], q[MAX_MOD + 1];
        zero<-1>(acc, nm + 1);
        for (int s = 0; s < (int)len[0]; s++) {
            for (int i = 0; i < lb; i++) a[i] = rd(s * lb + i);
            reduce<-1, -1>(ra, a, lb, m, nm, st);
            ra[nm] = 0;
            add<-1>(acc, acc, ra, nm + 1);
        }
        divrem<-1, -1>(q, ra, acc, nm + 1, m, nm, st);
        store<-1, WR>(wr, 0, ra, nm, len[2]);
        wr(len[2], q[0]);
        break;
    }
    case K_DIV_REM: {                                // in: a, b   out: div, rem; a zero divisor gives div = rem = 0
        uint32_t q[MAX_LIMBS], r[MAX_MOD];
        for (int i = 0; i < la; i++) a[i] = rd(i);
        for (int i = 0; i < lb; i++) b[i] = rd(la + i);
        const int nb = used_limbs(b, lb);
        zero<-1>(q, MAX_LIMBS); zero<-1>(r, MAX_MOD);
        if (nb) divrem<-1, -1>(q, r, a, la, b, nb, st);
        store<-1, WR>(wr, 0, q, la, len[2]);
        store<-1, WR>(wr, len[2], r, nb, len[3]);
        break;
    }
    case K_GLV: {                                    // in: k (8)   out: k1, k2 (len[1], len[2]: 4 in the circuit), k1_neg, k2_neg
        uint32_t k1[8], k2[8], n1, n2;
        for (int i = 0; i < 8; i++) a[i] = rd(i);
        glv_decompose(k1, k2, &n1, &n2, a, st);
        store<-1, WR>(wr, 0, k1, 8, len[1]);
        store<-1, WR>(wr, len[1], k2, 8, len[2]);
        wr(len[1] + len[2], n1);
        wr(len[1] + len[2] + 1, n2);
        break;
    }
    default: break;
    }
}

}  // namespace big
