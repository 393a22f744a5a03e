// quotient_kernels.inc -- K6: the gate bodies (gate_terms), the carry-free accumulators they feed (acc.h) and the kernels that evaluate the
// vanishing polynomial over Z_H.  Included by prover.hip; launched by stage_quotient_eval / stage_quotient_coeffs (prover_stages.inc);
// the limb-gate launch plan k_quotient_limbs walks is built by build_quotient_plan (circuit_create.inc).
#include <type_traits>
#include "acc.h"

struct QArgs {                      // per circuit and FRI domain: the same for every proof of a batch
    const u64 *cs;                  // coset-major LDE [ncols][R][n] of constants ++ sigmas
    const DevGate *gates;
    const u64 *k_is;
    u64 shift_r[MAXR], zh[MAXR], zh_inv[MAXR];   // per evaluated plane
    u64 w_n, n_field;
    u32 lg, rb, step, nc, nsel, nr, nw, nch, npp, qdf, num_gates, nterms, many_selectors, gate_mode;
    u32 k_ratio;                    // != 0: k_is[j] = k_ratio^j (plonky2's get_unique_coset_shifts: powers of the generator 7)
    const u64 *l0;                  // [Rq][n]: L_0(x) = Z_H(x) / (n (x - 1)) on the evaluated planes (k_l0_table)
};
struct QProof {                     // per proof
    const u64 *wl, *zl;             // coset-major LDEs of the wires and of Z ++ partial products
    u64 *out;                       // [nch][Rq][n]
    const u64 *apow;                // [nch][nterms] powers of the alphas
    const u64 *apl;                 // the same powers as 22-bit limbs of m and of m 2^32, APL_WORDS words per power (AccHL)
    u64 betas[MAXCH], gammas[MAXCH], pih[4];
};
// many-proofs batch (glp_prove_batch): blockIdx.z = proof; arrays advance by a stride per proof, challenges and the public-input
// hash come from pp[proof][3 MAXCH] (betas, gammas, pih).  pp == nullptr: a single proof described by the QProof kernel argument.
struct QBatch { const u64 *pp; size_t wl_stride, zl_stride, out_stride, apow_stride; };
static_assert(MAXCH == 4, "pp layout: 4 betas, 4 gammas, 4 words of the public-input hash");
__device__ __forceinline__ QProof q_proof(const QProof &p0, const QBatch &b) {
    QProof p = p0;
    if (b.pp) {
        const size_t k = blockIdx.z;
        p.wl += k * b.wl_stride; p.zl += k * b.zl_stride; p.out += k * b.out_stride; p.apow += k * b.apow_stride; p.apl += APL_WORDS * k * b.apow_stride;
        const u64 *q = b.pp + k * 3 * MAXCH;
        _Pragma("unroll") for (int c = 0; c < MAXCH; c++) { p.betas[c] = q[c]; p.gammas[c] = q[MAXCH + c]; p.pih[c] = q[2 * MAXCH + c]; }
    }
    return p;
}
// L_0 on the evaluated planes.  One thread owns position q of every plane and inverts the Rq denominators n (x_rq - 1)
// with ONE field inversion (Montgomery's trick) instead of one per point inside k_quotient.
struct L0Args { u64 shift_r[MAXR], zh[MAXR]; u64 w_n, n_field; u32 lg; };      // filled by coset_plane_tables (prover_stages.inc)
__global__ __launch_bounds__(256) void k_l0_table(L0Args a, u64 *out, u32 Rq) {
    const size_t n = (size_t)1 << a.lg;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const u64 wq = dpow(a.w_n, q);
    u64 d[MAXR], pre[MAXR];
    u64 run = 1;
    for (u32 rq = 0; rq < Rq; rq++) {            // x is never 1 on a coset g W^r H: every denominator is invertible
        d[rq] = mul(a.n_field, sub(mul(a.shift_r[rq], wq), 1));
        pre[rq] = run;
        run = mul(run, d[rq]);
    }
    u64 iv = inv(run);
    for (int rq = (int)Rq - 1; rq >= 0; rq--) {
        out[(size_t)rq * n + q] = mul(a.zh[rq], mul(iv, pre[rq]));
        iv = mul(iv, d[rq]);
    }
}
// selector filter of one gate at one point: prod_{i in group, i != row} (i - s) [* (UNUSED - s)]
__device__ __forceinline__ u64 gate_filter(const QArgs &a, const DevGate &g, size_t N, size_t slot) {
    const u64 s = a.cs[(size_t)g.selector_index * N + slot];
    u64 filter = 1;
    for (u32 i = g.group_start; i < g.group_end; i++)
        if (i != g.row) filter = mul(filter, sub((u64)i, s));
    if (a.many_selectors) filter = mul(filter, sub(0xFFFFFFFFull, s));
    return filter;
}
// The unfiltered constraints of one gate, multiplied into the carry-free accumulators ga[c] (+= constraint_k alpha_c^(k0 + k)).
// HEAD_ONLY (the four base-4 limb gates of plonky2_u32): skip the limb columns -- their range products, base-4 sums and the
// sum-equals-wire constraints -- which k_quotient_limbs evaluates for all fused gates from ONE read of the wire planes.
// The sink of the constraints is the type of `ga`: the accumulators AccHL[MAXCH] of the quotient kernels, or any other type with a member
// emit(k, v) that is handed constraint k's value v (a u64, not always canonical) as it stands -- the witness checker's (witness_check.inc).
template <int NCH, int TYPE, bool HEAD_ONLY = false, class GA>
__device__ __forceinline__ void gate_terms(const QArgs &a, const QProof &p, const DevGate &g, size_t N, size_t slot, u32 k0, GA &ga) {
    const u32 nt = a.nterms;
    const u64 *W = p.wl + slot;                       // wire j  -> W[j * N]
    const u64 *GC = a.cs + (size_t)a.nsel * N + slot; // gate constant i -> GC[i * N]
    {
        const u64 *ap = p.apl + APL_WORDS * (size_t)k0;
#define EMIT(k, v)                                                                     \
    do {                                                                               \
        const u64 _v = (v);                                                            \
        if constexpr (std::is_same<GA, AccHL[MAXCH]>::value) {                         \
        _Pragma("unroll") for (int c2 = 0; c2 < NCH; c2++) acc3_fma(ga[c2], _v, ap + APL_WORDS * ((size_t)c2 * nt + (k)));   \
        } else ga.emit((u32)(k), _v);                                                  \
    } while (0)
// Base-4 limb columns LIMBS[j*N], j = COUNT-1 .. 0: eight loads are issued before their values are used (the gate
// loops have run-time bounds, so the compiler cannot software-pipeline them itself).  Constraint index KIDX may use _j.
#define LIMBS4_DESC(LIMBS, COUNT, SPLIT, KIDX, ACCLO, ACCHI)                                                      \
    {                                                                                                             \
        Base4Sum _slo, _shi;                                                                                      \
        b4_zero(_slo); b4_zero(_shi);                                                                             \
        for (int _j0 = (int)(COUNT); _j0 > 0; _j0 -= 8) {                                                         \
            u64 _lv[8];                                                                                            \
            _Pragma("unroll") for (int _t = 0; _t < 8; _t++) if (_t < _j0) _lv[_t] = (LIMBS)[(size_t)(_j0 - 1 - _t) * N]; \
            _Pragma("unroll") for (int _t = 0; _t < 8; _t++) if (_t < _j0) {                                      \
                const int _j = _j0 - 1 - _t;                                                                      \
                EMIT((KIDX), range_product(_lv[_t], 4));                                                           \
                if (_j < (int)(SPLIT)) b4_add(_slo, _lv[_t], (u32)_j); else b4_add(_shi, _lv[_t], (u32)(_j - (int)(SPLIT))); \
            }                                                                                                     \
        }                                                                                                         \
        ACCLO = b4_value(_slo);                                                                                   \
        if ((int)(COUNT) > (int)(SPLIT)) ACCHI = b4_value(_shi);                                                  \
    }
        switch (TYPE >= 0 ? (u32)TYPE : g.type) {   // TYPE >= 0: the switch folds to one case at compile time
        case GLP_GATE_CONSTANT:
            for (u32 i = 0; i < g.p0; i++) EMIT(i, sub(GC[(size_t)i * N], W[(size_t)i * N]));
            break;
        case GLP_GATE_PUBLIC_INPUT:
            for (u32 i = 0; i < 4; i++) EMIT(i, sub(W[(size_t)i * N], p.pih[i]));
            break;
        case GLP_GATE_ARITHMETIC: {
            const u64 c0 = GC[0], c1 = GC[N];
            for (u32 i = 0; i < g.p0; i++) {
                const u64 m0 = W[(size_t)(4 * i) * N], m1 = W[(size_t)(4 * i + 1) * N];
                const u64 ad = W[(size_t)(4 * i + 2) * N], o = W[(size_t)(4 * i + 3) * N];
                EMIT(i, sub(o, add(mul(mul(m0, m1), c0), mul(ad, c1))));
            }
            break;
        }
        case GLP_GATE_POSEIDON: {
            // gates/poseidon.rs: wires = inputs 0..11, outputs 12..23, swap 24, delta 25..28, full_sbox_0(r=1..3)
            // from 29, partial_sbox from 65, full_sbox_1 from 87.  The S-box inputs are the only place wires enter, so any
            // schedule of the linear layers gives the constraints plonky2's sparse-matrix schedule gives: this is the
            // permutation's own gfx950 schedule (poseidon.h: non-canonical values between layers, the next round's constants
            // folded into the linear layer, partial rounds in blocks of 3 / 4 / 4 / 4 / 4 / 3) with the wire taking the
            // place of the state wherever an S-box is entered.
#if defined(__HIP_DEVICE_COMPILE__)
            u32 k = 0;
            u64 st[12];
            const u64 swap = W[(size_t)24 * N];
            EMIT(k, mul_nc(swap, sub(swap, 1))); k++;
            for (u32 i = 0; i < 4; i++) {
                const u64 lhs = W[(size_t)i * N], rhs = W[(size_t)(i + 4) * N], dl = W[(size_t)(25 + i) * N];
                EMIT(k, sub(mul(swap, sub(rhs, lhs)), dl)); k++;
                st[i] = add(lhs, dl); st[i + 4] = sub(rhs, dl);
            }
            for (u32 i = 8; i < 12; i++) st[i] = W[(size_t)i * N];
            for (u32 i = 0; i < 12; i++) st[i] = add(st[i], pos::RC[i]);
            pos::sbox_layer_nc(st);
            pos::mds_add_nc(st, pos::RCN.k[0]);
            for (u32 r = 1; r < 4; r++) {
                for (u32 i = 0; i < 12; i++) { const u64 in = W[(size_t)(29 + 12 * (r - 1) + i) * N]; EMIT(k, add_cnc(neg(in), st[i])); k++; st[i] = in; }
                pos::sbox_layer_nc(st);
                if (r < 3) pos::mds_add_nc(st, pos::RCN.k[r]);       // round 3's linear layer is part of the merged block
            }
            u32 pr = 0;                                              // partial round of the block's first S-box
            auto wire_in = [&](int j, u64 z) {
                const u64 in = W[(size_t)(65 + pr + (u32)j) * N];
                EMIT(k, add_cnc(neg(in), z)); k++;
                return in;
            };
            pos::partial_block_nc<3, true>(st, pos::PBM[0], wire_in); pr += 3;
            for (int b = 0; b < 4; b++) { pos::partial_block_nc<4, false>(st, pos::PB4[b], wire_in); pr += 4; }
            pos::partial_block_nc<3, false>(st, pos::PB3[0], wire_in);
            for (u32 r = 0; r < 4; r++) {
                for (u32 i = 0; i < 12; i++) { const u64 in = W[(size_t)(87 + 12 * r + i) * N]; EMIT(k, add_cnc(neg(in), st[i])); k++; st[i] = in; }
                pos::sbox_layer_nc(st);
                pos::mds_add_nc(st, r < 3 ? pos::RCN.k[4 + r] : pos::RC_ZERO);
            }
            for (u32 i = 0; i < 12; i++) { EMIT(k, add_cnc(neg(W[(size_t)(12 + i) * N]), st[i])); k++; }
#endif
            break;
        }
        case GLP_GATE_U32_INTERLEAVE: {
            u32 k = 0;
            for (u32 i = 0; i < g.p0; i++) {
                const u64 xw = W[(size_t)(2 * i) * N], xi = W[(size_t)(2 * i + 1) * N];
                const u64 *bits = W + (size_t)(2 * g.p0 + 32 * i) * N;
                u64 cx = 0, cxi = 0;
                const u32 kb = k + 2;
                for (u32 b = 0; b < 32; b++) {
                    const u64 bit = bits[(size_t)b * N];
                    cx = add(dbl(cx), bit);
                    cxi = add(dbl(dbl(cxi)), bit);
                    EMIT(kb + b, mul_nc(bit, sub(bit, 1)));
                }
                EMIT(k, sub(cx, xw));
                EMIT(k + 1, sub(cxi, xi));
                k += 34;
            }
            break;
        }
        case GLP_GATE_UNINTERLEAVE_U32:
        case GLP_GATE_UNINTERLEAVE_B32: {
            u32 k = 0;
            for (u32 i = 0; i < g.p0; i++) {
                const u64 xi = W[(size_t)(3 * i) * N], xe = W[(size_t)(3 * i + 1) * N], xo = W[(size_t)(3 * i + 2) * N];
                const u64 *bits = W + (size_t)(3 * g.p0 + 64 * i) * N;
                u64 cxi = 0, ce = 0, co = 0;
                const u32 kb = k + 3;
                for (u32 j = 0; j < 32; j++) {   // Horner from the most significant bit: coeff 2^(31-j) or 4^(31-j)
                    const u64 be = bits[(size_t)(2 * j) * N], bo = bits[(size_t)(2 * j + 1) * N];
                    cxi = add(dbl(add(dbl(cxi), be)), bo);
                    if (g.type == GLP_GATE_UNINTERLEAVE_U32) { ce = add(dbl(ce), be); co = add(dbl(co), bo); }
                    else { ce = add(dbl(dbl(ce)), be); co = add(dbl(dbl(co)), bo); }
                    EMIT(kb + 2 * j, mul_nc(be, sub(be, 1)));
                    EMIT(kb + 2 * j + 1, mul_nc(bo, sub(bo, 1)));
                }
                EMIT(k, sub(cxi, xi));
                EMIT(k + 1, sub(ce, xe));
                EMIT(k + 2, sub(co, xo));
                k += 67;
            }
            break;
        }
        case GLP_GATE_U32_ARITHMETIC: {
            u32 k = 0; const u32 nops = g.p0;
            for (u32 i = 0; i < nops; i++) {
                const u64 m0 = W[(size_t)(6 * i) * N], m1 = W[(size_t)(6 * i + 1) * N], ad = W[(size_t)(6 * i + 2) * N];
                const u64 lo = W[(size_t)(6 * i + 3) * N], hi = W[(size_t)(6 * i + 4) * N], iv = W[(size_t)(6 * i + 5) * N];
                const u64 hi_not_max = sub(mul(iv, sub(0xFFFFFFFFull, hi)), 1);
                EMIT(k, mul_nc(hi_not_max, lo)); k++;
                EMIT(k, sub(add(mul(hi, (u64)1 << 32), lo), add(mul(m0, m1), ad))); k++;
                if constexpr (!HEAD_ONLY) {
                    u64 cl = 0, chh = 0;
                    const u64 *limbs = W + (size_t)(6 * nops + 32 * i) * N;
                    LIMBS4_DESC(limbs, 32, 16, k + (31 - _j), cl, chh);
                    EMIT(k + 32, sub(cl, lo));
                    EMIT(k + 33, sub(chh, hi));
                }
                k += 34;
            }
            break;
        }
        case GLP_GATE_U32_ADD_MANY: {
            u32 k = 0; const u32 na = g.p0, nops = g.p1, wd = na + 3;
            for (u32 i = 0; i < nops; i++) {
                // addends + carry in as a 96-bit integer sum (three carry instructions per term against a modular addition's eight), folded once
                u64 slo = W[(size_t)(wd * i + na) * N];
                u32 shi = 0;
                for (u32 j = 0; j < na; j += 8) {          // eight loads in flight (na is a run-time value: no unrolling otherwise)
                    u64 t[8];
                    _Pragma("unroll") for (u32 e = 0; e < 8; e++) t[e] = j + e < na ? W[(size_t)(wd * i + j + e) * N] : 0;
                    _Pragma("unroll") for (u32 e = 0; e < 8; e++) { slo += t[e]; shi += slo < t[e] ? 1u : 0u; }
                }
                const u64 sum = canon(fold96_nc(slo, shi));
                const u64 res = W[(size_t)(wd * i + na + 1) * N], car = W[(size_t)(wd * i + na + 2) * N];
                EMIT(k, sub(add(mul(car, (u64)1 << 32), res), sum)); k++;
                if constexpr (!HEAD_ONLY) {
                    u64 cr = 0, cc = 0;
                    const u64 *limbs = W + (size_t)(wd * nops + 18 * i) * N;
                    LIMBS4_DESC(limbs, 18, 16, k + (17 - _j), cr, cc);
                    EMIT(k + 18, sub(cr, res));
                    EMIT(k + 19, sub(cc, car));
                }
                k += 20;
            }
            break;
        }
        case GLP_GATE_U32_SUBTRACTION: {
            u32 k = 0; const u32 nops = g.p0;
            for (u32 i = 0; i < nops; i++) {
                const u64 xx = W[(size_t)(5 * i) * N], yy = W[(size_t)(5 * i + 1) * N], bi = W[(size_t)(5 * i + 2) * N];
                const u64 res = W[(size_t)(5 * i + 3) * N], bo = W[(size_t)(5 * i + 4) * N];
                EMIT(k, sub(res, add(sub(sub(xx, yy), bi), mul(bo, (u64)1 << 32)))); k++;
                if constexpr (!HEAD_ONLY) {
                    u64 cl = 0, unused_hi = 0;
                    const u64 *limbs = W + (size_t)(5 * nops + 16 * i) * N;
                    LIMBS4_DESC(limbs, 16, 16, k + (15 - _j), cl, unused_hi);
                    (void)unused_hi;
                    EMIT(k + 16, sub(cl, res));
                }
                k += 17;
                EMIT(k, mul_nc(bo, sub(1, bo))); k++;
            }
            break;
        }
        case GLP_GATE_U32_RANGE_CHECK: {
            u32 k = 0; const u32 nin = g.p0;
            if constexpr (!HEAD_ONLY) {
                for (u32 i = 0; i < nin; i++) {
                    const u64 *aux = W + (size_t)(nin + 16 * i) * N;
                    u64 sum = 0, unused_hi = 0;
                    LIMBS4_DESC(aux, 16, 16, k + 1 + _j, sum, unused_hi);
                    (void)unused_hi;
                    EMIT(k, sub(sum, W[(size_t)i * N]));
                    k += 17;
                }
            }
            break;
        }
        case GLP_GATE_COMPARISON: {
            u32 k = 0; const u32 nb = g.p0, ncx = g.p1, cb = (nb + ncx - 1) / ncx, cs = 1u << cb;
            const u64 *ca = W + (size_t)4 * N, *cbp = ca + (size_t)ncx * N, *ed = cbp + (size_t)ncx * N;
            const u64 *ceq = ed + (size_t)ncx * N, *iv = ceq + (size_t)ncx * N, *mb = iv + (size_t)ncx * N;
            u64 fa = 0, fb = 0;
            for (int i = (int)ncx - 1; i >= 0; i--) { fa = add(mul(fa, cs), ca[(size_t)i * N]); fb = add(mul(fb, cs), cbp[(size_t)i * N]); }
            EMIT(k, sub(fa, W[0])); k++;
            EMIT(k, sub(fb, W[N])); k++;
            u64 msd = 0;
            for (u32 i0 = 0; i0 < ncx; i0 += 4) {     // 20 loads in flight per batch of four chunks
                u64 la[4], lb[4], le[4], li[4], ld[4];
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (i0 + t < ncx) {
                        const size_t o = (size_t)(i0 + t) * N;
                        la[t] = ca[o]; lb[t] = cbp[o]; le[t] = ceq[o]; li[t] = iv[o]; ld[t] = ed[o];
                    }
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (i0 + t < ncx) {
                        EMIT(k, range_product(la[t], cs)); k++;
                        EMIT(k, range_product(lb[t], cs)); k++;
                        const u64 diff = sub(lb[t], la[t]);
                        EMIT(k, sub(mul(diff, ld[t]), sub(1, le[t]))); k++;
                        EMIT(k, mul_nc(le[t], diff)); k++;
                        EMIT(k, sub(li[t], mul(le[t], msd))); k++;
                        msd = add(li[t], mul(sub(1, le[t]), diff));
                    }
            }
            const u64 msdw = W[(size_t)3 * N];
            EMIT(k, sub(msdw, msd)); k++;
            u64 bc = 0;
            for (u32 j = 0; j <= cb; j++) { const u64 bit = mb[(size_t)j * N]; EMIT(k, mul_nc(bit, sub(1, bit))); k++; }
            for (int j = (int)cb; j >= 0; j--) bc = add(dbl(bc), mb[(size_t)j * N]);
            EMIT(k, sub(add((u64)cs, msdw), bc)); k++;
            EMIT(k, sub(W[(size_t)2 * N], mb[(size_t)cb * N])); k++;
            break;
        }
        case GLP_GATE_BASE_SUM: {
            u32 k = 0; const u32 nl = g.p0, Bb = g.p1;
            u64 sum = 0;
            for (int j = (int)nl - 1; j >= 0; j--) sum = add(mul(sum, Bb), W[(size_t)(1 + j) * N]);
            EMIT(k, sub(sum, W[0])); k++;
            for (u32 j = 0; j < nl; j++) { EMIT(k, range_product(W[(size_t)(1 + j) * N], Bb)); k++; }
            break;
        }
        case GLP_GATE_RANDOM_ACCESS: {
            u32 k = 0; const u32 bits = g.p0, copies = g.p1 & 0xFFFF, nextra = g.p1 >> 16, vs = 1u << bits;
            const u32 routed = (2 + vs) * copies + nextra;
            for (u32 cpy = 0; cpy < copies; cpy++) {
                const u64 *bse = W + (size_t)((2 + vs) * cpy) * N, *bw = W + (size_t)(routed + bits * cpy) * N;
                u64 idx = 0;
                u64 sel;
                if (bits == 4) {           // the width the reference uses; folded in registers, every wire loaded once and the loads batched
                    const u64 b0 = bw[0], b1 = bw[N], b2 = bw[2 * N], b3 = bw[3 * N], claimed_idx = bse[0];
                    EMIT(k, mul_nc(b0, sub(b0, 1))); EMIT(k + 1, mul_nc(b1, sub(b1, 1))); EMIT(k + 2, mul_nc(b2, sub(b2, 1))); EMIT(k + 3, mul_nc(b3, sub(b3, 1)));
                    k += 4;
                    idx = add(dbl(add(dbl(add(dbl(b3), b2)), b1)), b0);
                    EMIT(k, sub(idx, claimed_idx)); k++;
                    u64 l2[4];
#pragma unroll
                    for (int q4 = 0; q4 < 4; q4++) {
                        const u64 *it = bse + (size_t)(2 + 4 * q4) * N;
                        const u64 i0 = it[0], i1 = it[N], i2 = it[2 * N], i3 = it[3 * N];
                        const u64 f0 = add(i0, mul(b0, sub(i1, i0))), f1 = add(i2, mul(b0, sub(i3, i2)));
                        l2[q4] = add(f0, mul(b1, sub(f1, f0)));
                    }
                    const u64 g0 = add(l2[0], mul(b2, sub(l2[1], l2[0]))), g1 = add(l2[2], mul(b2, sub(l2[3], l2[2])));
                    sel = add(g0, mul(b3, sub(g1, g0)));
                } else {                   // generic width: select by recursion over the index bits (no local array)
                    for (u32 b = 0; b < bits; b++) { const u64 bit = bw[(size_t)b * N]; EMIT(k, mul_nc(bit, sub(bit, 1))); k++; }
                    for (int b = (int)bits - 1; b >= 0; b--) idx = add(dbl(idx), bw[(size_t)b * N]);
                    EMIT(k, sub(idx, bse[0])); k++;
                    sel = 0;
                    for (u32 j = 0; j < vs; j++) {
                        u64 ind = 1;       // product over bits of (bit or 1 - bit): Lagrange indicator of slot j
                        for (u32 b = 0; b < bits; b++) { const u64 bit = bw[(size_t)b * N]; ind = mul(ind, ((j >> b) & 1) ? bit : sub(1, bit)); }
                        sel = add(sel, mul(ind, bse[(size_t)(2 + j) * N]));
                    }
                }
                EMIT(k, sub(sel, bse[N])); k++;
            }
            for (u32 e = 0; e < nextra; e++) { EMIT(k, sub(GC[(size_t)e * N], W[(size_t)((2 + vs) * copies + e) * N])); k++; }
            break;
        }
        // plonky2's extension-field gates (D = 2; recalled, unpinned: DESIGN.md).  On the LDE coset every wire is a base-field
        // value, so an ext value at wires [a, a+1] is the F_p^2 element W[a] + W[a+1] X; the two constraints of an op are the
        // two components of one difference.  Each op's wire planes are loaded before any of them is used.
        case GLP_GATE_ARITHMETIC_EXTENSION: {        // output - (c0 m0 m1 + c1 addend), wires [8i, 8i+8)
            const u64 c0 = GC[0], c1 = GC[N];
            for (u32 i = 0; i < g.p0; i++) {
                const u64 *o = W + (size_t)(8 * i) * N;
                const u64 w0 = o[0], w1 = o[N], w2 = o[2 * N], w3 = o[3 * N], w4 = o[4 * N], w5 = o[5 * N], w6 = o[6 * N], w7 = o[7 * N];
                const ext2 t = e_add(e_scale(e_mul(e_make(w0, w1), e_make(w2, w3)), c0), e_scale(e_make(w4, w5), c1));
                EMIT(2 * i, sub(w6, t.a)); EMIT(2 * i + 1, sub(w7, t.b));
            }
            break;
        }
        case GLP_GATE_MUL_EXTENSION: {               // output - c0 m0 m1, wires [6i, 6i+6)
            const u64 c0 = GC[0];
            for (u32 i = 0; i < g.p0; i++) {
                const u64 *o = W + (size_t)(6 * i) * N;
                const u64 w0 = o[0], w1 = o[N], w2 = o[2 * N], w3 = o[3 * N], w4 = o[4 * N], w5 = o[5 * N];
                const ext2 t = e_scale(e_mul(e_make(w0, w1), e_make(w2, w3)), c0);
                EMIT(2 * i, sub(w4, t.a)); EMIT(2 * i + 1, sub(w5, t.b));
            }
            break;
        }
        case GLP_GATE_REDUCING:                      // acc_{i-1} alpha + coeff_i - acc_i; output [0,2), alpha [2,4), old_acc [4,6)
        case GLP_GATE_REDUCING_EXTENSION: {          // coeffs from 6 (1 or 2 wires each), then acc_0 .. acc_{N-2}; acc_{N-1} = output
            const u32 nco = g.p0, cw = TYPE == GLP_GATE_REDUCING ? 1u : TYPE == GLP_GATE_REDUCING_EXTENSION ? 2u : (g.type == GLP_GATE_REDUCING ? 1u : 2u);
            const u32 accs = 6 + cw * nco;
            const ext2 alpha = e_make(W[2 * N], W[3 * N]);
            ext2 acc = e_make(W[4 * N], W[5 * N]);
            for (u32 i = 0; i < nco; i++) {
                const u64 *co = W + (size_t)(6 + cw * i) * N, *ac = W + (size_t)(i + 1 < nco ? accs + 2 * i : 0) * N;
                const u64 k0v = co[0], k1v = cw == 2 ? co[N] : 0, a0 = ac[0], a1 = ac[N];
                const ext2 t = e_add(e_mul(acc, alpha), e_make(k0v, k1v));
                EMIT(2 * i, sub(t.a, a0)); EMIT(2 * i + 1, sub(t.b, a1));
                acc = e_make(a0, a1);
            }
            break;
        }
        // The rest of the recursive verifier's gate set (D = 2).  Exponentiation and CosetInterpolation are recalled, unpinned
        // (DESIGN.md); PoseidonMds is pinned through the Poseidon MDS constants.
        case GLP_GATE_EXPONENTIATION: {              // base 0, bits 1..n (little-endian), output n+1, intermediates n+2..2n+1
            // constraint i: prev (bit base + 1 - bit) - intermediate_i, prev = 1 resp. intermediate_{i-1}^2, bit = bits[n-1-i]
            const u32 nb = g.p0;
            const u64 bm1 = sub(W[0], 1);            // bit base + 1 - bit = bit (base - 1) + 1
            u64 last = 0;
            for (u32 i0 = 0; i0 < nb; i0 += 8) {     // eight bit planes and eight intermediate planes in flight
                u64 bt[8], im[8];
                _Pragma("unroll") for (u32 t = 0; t < 8; t++) if (i0 + t < nb) { bt[t] = W[(size_t)(nb - (i0 + t)) * N]; im[t] = W[(size_t)(nb + 2 + i0 + t) * N]; }
                _Pragma("unroll") for (u32 t = 0; t < 8; t++) if (i0 + t < nb) {
                    const u64 f = add(mul(bt[t], bm1), 1);
                    EMIT(i0 + t, sub(i0 + t == 0 ? f : mul(mul(last, last), f), im[t]));
                    last = im[t];
                }
            }
            EMIT(nb, sub(W[(size_t)(nb + 1) * N], last));
            break;
        }
        case GLP_GATE_COSET_INTERPOLATION: {
            // shift 0, values from 1 (N pairs), evaluation point, evaluation value, I intermediate evals, I intermediate prods,
            // shifted point x.  Barycentric chain over the unshifted subgroup {x_i} with weights w_i = x_i / N (coset_table):
            // (eval, prod) <- (eval (x - x_i) + w_i value_i prod, prod (x - x_i)), checkpointed into the intermediates after the
            // first d points and then after every d - 1.
            const u32 np = 1u << g.p0, d = g.p1, ni = (np - 2) / (d - 1);
            const u32 o_pt = 1 + 2 * np, o_ie = o_pt + 4, o_ip = o_ie + 2 * ni, o_sp = o_ip + 2 * ni;
            const u64 *tab = coset_table(a.gates, a.num_gates, g.p0);
            const u64 shift = W[0];
            const ext2 x = e_make(W[(size_t)o_sp * N], W[(size_t)(o_sp + 1) * N]);
            EMIT(0, sub(mul(x.a, shift), W[(size_t)o_pt * N])); EMIT(1, sub(mul(x.b, shift), W[(size_t)(o_pt + 1) * N]));
            ext2 ev = e_from(0), pr = e_from(1);
            u32 start = 0;
            for (u32 c = 0; c <= ni; c++) {
                const u32 end = min(np, d + c * (d - 1));
                for (u32 j0 = start; j0 < end; j0 += 8) {      // a chunk's value planes (eight points at a time) before their use
                    u64 va[8], vb[8];
                    _Pragma("unroll") for (u32 t = 0; t < 8; t++) if (j0 + t < end) { va[t] = W[(size_t)(1 + 2 * (j0 + t)) * N]; vb[t] = W[(size_t)(2 + 2 * (j0 + t)) * N]; }
                    _Pragma("unroll") for (u32 t = 0; t < 8; t++) if (j0 + t < end) {
                        const ext2 dx = e_make(sub(x.a, tab[2 * (j0 + t)]), x.b);
                        ev = e_add(e_mul(ev, dx), e_scale(e_mul(e_make(va[t], vb[t]), pr), tab[2 * (j0 + t) + 1]));
                        pr = e_mul(pr, dx);
                    }
                }
                start = end;
                if (c < ni) {
                    const u64 *ie = W + (size_t)(o_ie + 2 * c) * N, *ip = W + (size_t)(o_ip + 2 * c) * N;
                    const u64 e0 = ie[0], e1 = ie[N], q0 = ip[0], q1 = ip[N];
                    EMIT(2 + 4 * c, sub(e0, ev.a)); EMIT(3 + 4 * c, sub(e1, ev.b)); EMIT(4 + 4 * c, sub(q0, pr.a)); EMIT(5 + 4 * c, sub(q1, pr.b));
                    ev = e_make(e0, e1); pr = e_make(q0, q1);
                }
            }
            EMIT(2 + 4 * ni, sub(W[(size_t)(o_pt + 2) * N], ev.a)); EMIT(3 + 4 * ni, sub(W[(size_t)(o_pt + 3) * N], ev.b));
            break;
        }
        case GLP_GATE_POSEIDON_MDS: {                // input i at [2i, 2i+2), output i at [24+2i, 24+2i+2): out - MDS in, per component
#if defined(__HIP_DEVICE_COMPILE__)
            for (u32 cmp = 0; cmp < 2; cmp++) {      // one component at a time: 12 input planes, the unreduced limb rows of poseidon.h
                u64 st[12], ov[12];
                _Pragma("unroll") for (u32 i = 0; i < 12; i++) { st[i] = W[(size_t)(2 * i + cmp) * N]; ov[i] = W[(size_t)(24 + 2 * i + cmp) * N]; }
                pos::mds_add_nc(st, pos::RC_ZERO);
                _Pragma("unroll") for (u32 i = 0; i < 12; i++) EMIT(2 * i + cmp, sub(ov[i], canon(st[i])));
            }
#endif
            break;
        }
        default: break;   // NOOP
        }
#undef LIMBS4_DESC
#undef EMIT
    }
}
// Contribution of ONE gate at one point: filter(selector) * sum_k constraint_k * alpha_c^(k0 + k), added into acc[c].
// TYPE >= 0 compiles a single gate body (per-gate kernels: small register footprint, high occupancy); TYPE = -1
// keeps the run-time switch (monolithic fallback).
template <int NCH, int TYPE>
__device__ __forceinline__ void gate_contrib(const QArgs &a, const QProof &p, const DevGate &g, size_t N, size_t slot, u32 k0, u64 (&acc)[MAXCH]) {
    const u64 filter = gate_filter(a, g, N, slot);
    AccHL ga[MAXCH];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) acc3_zero(ga[c]);
    gate_terms<NCH, TYPE, false>(a, p, g, N, slot, k0, ga);
    _Pragma("unroll") for (int c = 0; c < NCH; c++) acc[c] = add(acc[c], mul(filter, acc3_reduce(ga[c])));
}

// Gates that ride along with another launch (indices into the gate table)
// arith_ops != 0: gate arith_gi is an ArithmeticGate whose first arith_ops operations read only routed wires; k_quotient
// evaluates them from the wire values its permutation loop has in registers anyway (no second read of those planes).
struct LightArgs { u32 count; u32 gi[8]; u32 arith_gi, arith_ops; };
// The HBM-bound gate types (Constant, PublicInput, Arithmetic, BaseSum, RandomAccess), evaluated one after the other
template <int NCH>
__device__ __forceinline__ void light_gates(const QArgs &a, const QProof &p, const LightArgs &la, size_t N, size_t slot, u32 k0, u64 (&acc)[MAXCH]) {
    for (u32 t = 0; t < la.count; t++) {
        const DevGate g = a.gates[la.gi[t]];
        switch (g.type) {                      // uniform: every lane runs the same gate
        case GLP_GATE_CONSTANT: gate_contrib<NCH, GLP_GATE_CONSTANT>(a, p, g, N, slot, k0, acc); break;
        case GLP_GATE_PUBLIC_INPUT: gate_contrib<NCH, GLP_GATE_PUBLIC_INPUT>(a, p, g, N, slot, k0, acc); break;
        case GLP_GATE_ARITHMETIC: gate_contrib<NCH, GLP_GATE_ARITHMETIC>(a, p, g, N, slot, k0, acc); break;
        case GLP_GATE_BASE_SUM: gate_contrib<NCH, GLP_GATE_BASE_SUM>(a, p, g, N, slot, k0, acc); break;
        case GLP_GATE_RANDOM_ACCESS: gate_contrib<NCH, GLP_GATE_RANDOM_ACCESS>(a, p, g, N, slot, k0, acc); break;
        default: break;
        }
    }
}
// K6: vanishing polynomial / Z_H on the planes r = 0, step, 2 step, ... of the coset-major LDE domain.
//   terms: [L_0 (Z_c - 1)]_c, [prev*num - next*den]_{c,chunk}, gate constraints; res_c = sum_k term_k alpha_c^k
// GATES: 0 = permutation terms only; 1 = every gate (monolithic, run-time switch); 2 = the light gates of `la`: the
// permutation terms are VALU-bound and the light gates HBM-bound, so in one launch the waves in one phase fill the other
// phase's idle unit (separately: 3.3 + 2.75 ms at the headline size)
template <int NCH, int GATES>
__global__ __launch_bounds__(256, GATES == 1 ? 3 : 4) void k_quotient(QArgs a, QProof p0, QBatch qb, LightArgs la) {
    const QProof p = q_proof(p0, qb);
    const size_t n = (size_t)1 << a.lg, N = n << a.rb;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const u32 rq = blockIdx.y, r = rq * a.step;
    const size_t slot = (size_t)r * n + q, slot_next = (size_t)r * n + ((q + 1) & (n - 1));
    const u64 x = mul(a.shift_r[rq], dpow(a.w_n, q));
    constexpr u32 nch = NCH; const u32 nchunks = a.npp + 1, nt = a.nterms;
    u64 acc[MAXCH], zx[MAXCH], zg[MAXCH];
    Acc160 pa[MAXCH];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) { acc_zero(pa[c]); zx[c] = p.zl[(size_t)c * N + slot]; zg[c] = p.zl[(size_t)c * N + slot_next]; }
    const u64 l0 = a.l0[(size_t)rq * n + q];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) {
        const u64 t = mul(l0, sub(zx[c], 1));
        _Pragma("unroll") for (int c2 = 0; c2 < NCH; c2++) acc_fma(pa[c2], t, p.apow[c2 * nt + c]);
    }
    // NOTE: the chunk loop below exists a second time, in k_perm_quotient (perm_seam.inc), over the seam's operands: a change to the
    // chain belongs in both.  One shared body was tried and measured slower here (profiles/r22_seam_one_body.txt).
    u64 bkx[MAXCH];                                    // beta_c k_j x for the next wire j (k_ratio path)
    _Pragma("unroll") for (int c = 0; c < NCH; c++) bkx[c] = mul_nc(p.betas[c], x);
    const u32 k0 = nch + nch * nchunks;
    // ArithmeticGate riding on the permutation loop's wire loads (GATES == 2 only)
    const u32 ar_ops = GATES == 2 ? la.arith_ops : 0;
    AccHL gar[MAXCH];
    u64 ar_c0 = 0, ar_c1 = 0;
    if (GATES == 2) {
        _Pragma("unroll") for (int c = 0; c < NCH; c++) acc3_zero(gar[c]);
        if (ar_ops) { ar_c0 = a.cs[(size_t)a.nsel * N + slot]; ar_c1 = a.cs[(size_t)(a.nsel + 1) * N + slot]; }
    }
    for (u32 chunk = 0; chunk < nchunks; chunk++) {
        u64 num[MAXCH], den[MAXCH];
        _Pragma("unroll") for (int c = 0; c < NCH; c++) { num[c] = 1; den[c] = 1; }
        const u32 j0 = chunk * a.qdf, j1 = min((chunk + 1) * a.qdf, a.nr);
        for (u32 jb = j0; jb < j1; jb += 8) {          // eight wire + eight sigma loads in flight
            u64 w8[8], s8[8];
#pragma unroll
            for (int t = 0; t < 8; t++)
                if (jb + t < j1) { w8[t] = p.wl[(size_t)(jb + t) * N + slot]; s8[t] = a.cs[(size_t)(a.nc + jb + t) * N + slot]; }
            if (GATES == 2 && ar_ops) {                // jb is a multiple of 4 here (the host checks qdf % 4 == 0)
#pragma unroll
                for (int t = 0; t < 8; t += 4)
                    if (jb + t + 3 < j1 && (jb + t) / 4 < ar_ops) {
                        const u32 i = (jb + t) / 4;
                        const u64 v = sub(w8[t + 3], add(mul(mul(w8[t], w8[t + 1]), ar_c0), mul(w8[t + 2], ar_c1)));
                        _Pragma("unroll") for (int c2 = 0; c2 < NCH; c2++) acc3_fma(gar[c2], v, p.apl + APL_WORDS * ((size_t)c2 * nt + k0 + i));
                    }
            }
#pragma unroll
            for (int t = 0; t < 8; t++)
                if (jb + t < j1) {
                    // lazy chain: the running products and the beta terms stay non-canonical u64 (mul_nc takes any
                    // u64); only w + gamma is a canonical addition, shared by numerator and denominator
                    // beta k_j x: with k_j = g^j (g < 2^32, how plonky2 picks the coset shifts) it is the previous
                    // wire's value times g -- two multiply-adds and a fold instead of two full multiplications
                    u64 kx = 0;
                    if (!a.k_ratio) kx = mul_nc(a.k_is[jb + t], x);
                    _Pragma("unroll") for (int c = 0; c < NCH; c++) {
                        const u64 wg = add(w8[t], p.gammas[c]);
                        const u64 bk = a.k_ratio ? bkx[c] : mul_nc(p.betas[c], kx);
                        num[c] = mul_nc_cc(num[c], add_cnc(wg, bk));
                        den[c] = mul_nc_cc(den[c], add_cnc(wg, mul_nc_cc(p.betas[c], s8[t])));
                        if (a.k_ratio) bkx[c] = mul_small_nc(bkx[c], a.k_ratio);
                    }
                }
        }
        _Pragma("unroll") for (int c = 0; c < NCH; c++) {
            const u64 prev = chunk == 0 ? zx[c] : p.zl[(size_t)(nch + c * a.npp + chunk - 1) * N + slot];
            const u64 next = chunk == nchunks - 1 ? zg[c] : p.zl[(size_t)(nch + c * a.npp + chunk) * N + slot];
            const u64 t = sub(mul(prev, num[c]), mul(next, den[c]));
            const u32 k = nch + c * nchunks + chunk;
            _Pragma("unroll") for (int c2 = 0; c2 < NCH; c2++) acc_fma(pa[c2], t, p.apow[c2 * nt + k]);
        }
    }
    _Pragma("unroll") for (int c = 0; c < NCH; c++) acc[c] = acc_reduce(pa[c]);
    if (GATES == 2 && ar_ops) {
        const u64 filter = gate_filter(a, a.gates[la.arith_gi], N, slot);
        _Pragma("unroll") for (int c = 0; c < NCH; c++) acc[c] = add(acc[c], mul(filter, acc3_reduce(gar[c])));
    }
    if constexpr (GATES == 1) {                        // monolithic: every gate here
        for (u32 gi = 0; gi < a.num_gates; gi++) {
            const DevGate g = a.gates[gi];
            gate_contrib<NCH, -1>(a, p, g, N, slot, k0, acc);
        }
    }
    if constexpr (GATES == 2) light_gates<NCH>(a, p, la, N, slot, k0, acc);
    const size_t Rq = (size_t)gridDim.y;
    _Pragma("unroll") for (int c = 0; c < NCH; c++) p.out[((size_t)c * Rq + rq) * n + q] = mul(acc[c], a.zh_inv[rq]);
}

// One gate type per launch (gate_mode = 1): out[c][plane][q] += zh_inv * filter * sum_k constraint_k alpha_c^(k0 + k)
template <int NCH, int TYPE>
__global__ __launch_bounds__(256) void k_quotient_gate(QArgs a, QProof p0, QBatch qb, u32 gi) {
    const QProof p = q_proof(p0, qb);
    const size_t n = (size_t)1 << a.lg, N = n << a.rb;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const u32 rq = blockIdx.y, r = rq * a.step;
    const size_t slot = (size_t)r * n + q;
    u64 acc[MAXCH];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) acc[c] = 0;
    const DevGate g = a.gates[gi];
    gate_contrib<NCH, TYPE>(a, p, g, N, slot, (u32)NCH + (u32)NCH * (a.npp + 1), acc);
    const size_t Rq = (size_t)gridDim.y;
    _Pragma("unroll") for (int c = 0; c < NCH; c++) {
        u64 *o = p.out + ((size_t)c * Rq + rq) * n + q;
        *o = add(*o, mul(acc[c], a.zh_inv[rq]));
    }
}

// The base-4 limb gates of plonky2_u32 (U32Arithmetic, U32AddMany, U32Subtraction, U32RangeCheck) in ONE launch.  Their
// limb columns overlap almost completely (wires 30..113 are limbs of all four in the secp256k1 circuit): every wire plane
// is read once, range_product(w_j, 4) is computed once per column and multiplied into each gate's own carry-free
// accumulators (the selector filters are applied after the reduction, as in the per-gate kernels).  The per-column work
// is driven by a table built at circuit creation (uniform control flow, scalar loads):
//   desc[j][s] for wire column j and fused gate slot s:
//     bit 0        the column is a base-4 limb of this gate
//     bits 1..4    position of the limb in its base-4 sum (weight 4^pos)
//     bit 5        this limb closes the sum: emit  (sum - W[ref])  at alpha index kf, then reset the sum
//     bits 6..15   alpha index of the limb's range-check constraint
//     bits 16..25  kf        bits 26..33  ref (wire column the sum must equal)
// The constraints that are not limb work (two per U32Arithmetic op, one per AddMany op, two per Subtraction op) come from
// gate_terms<.., HEAD_ONLY = true>.
// `extra`: HBM-bound gates without limb work of their own kind (ComparisonGate) evaluated in the same launch, for the same
// reason as the light gates in k_quotient: their loads overlap the limb gates' arithmetic.
// More limb gates than slots (the real secp256k1 circuit has ten: U32Arithmetic, seven U32AddMany parameter sets, U32RangeCheck,
// U32Subtraction) go through the same launch in GROUPS of LIMB_SLOTS (five: 123 VGPRs, four waves per SIMD; six cost a wave and
// measured slower): the accumulators are reused; the wire planes are read again per group (PMC: from HBM, the last-level cache does
// not hold them in between).
constexpr int LIMB_SLOTS = 5, LIMB_GROUPS = 4;
struct LimbArgs { const u64 *desc; u32 groups, num_wires; u32 count[LIMB_GROUPS], jlo[LIMB_GROUPS], jhi[LIMB_GROUPS]; u32 gi[LIMB_GROUPS][LIMB_SLOTS]; u32 extra_count, extra_gi[4]; };
inline void limb_args(const glp_circuit *cc, LimbArgs &la) {
    la.desc = cc->dev_limb_desc; la.groups = cc->limb_groups; la.num_wires = cc->d.num_wires;
    for (int g = 0; g < LIMB_GROUPS; g++) {
        la.count[g] = cc->limb_gcount[g]; la.jlo[g] = cc->limb_jlo[g]; la.jhi[g] = cc->limb_jhi[g];
        for (int i = 0; i < LIMB_SLOTS; i++) la.gi[g][i] = cc->limb_gi[g * LIMB_SLOTS + i];
    }
}
template <int NCH>
__global__ __launch_bounds__(256, 2) void k_quotient_limbs(QArgs a, QProof p0, QBatch qb, LimbArgs la) {
    const QProof p = q_proof(p0, qb);
    const size_t n = (size_t)1 << a.lg, N = n << a.rb;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const u32 rq = blockIdx.y, r = rq * a.step;
    const size_t slot = (size_t)r * n + q;
    const u32 k0 = (u32)NCH + (u32)NCH * (a.npp + 1), nt = a.nterms;
    const u64 *W = p.wl + slot;
    const u64 *ap = p.apl + APL_WORDS * (size_t)k0;
    u64 acc[MAXCH];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) acc[c] = 0;
#define LIMB_EMIT(S, K, V)                                                                                     \
    do {                                                                                                       \
        const u64 _v = (V);                                                                                    \
        _Pragma("unroll") for (int c2 = 0; c2 < NCH; c2++) acc3_fma(ga[S][c2], _v, ap + APL_WORDS * ((size_t)c2 * nt + (K)));   \
    } while (0)
#pragma unroll 1
    for (u32 grp = 0; grp < la.groups; grp++) {
        const u32 gcount = la.count[grp], jlo = la.jlo[grp], jhi = la.jhi[grp];
        const u64 *desc = la.desc + (size_t)grp * la.num_wires * LIMB_SLOTS;
        AccHL ga[LIMB_SLOTS][MAXCH];
        Base4Sum bs[LIMB_SLOTS];
        _Pragma("unroll") for (int s = 0; s < LIMB_SLOTS; s++) {
            b4_zero(bs[s]);
            _Pragma("unroll") for (int c = 0; c < NCH; c++) acc3_zero(ga[s][c]);
        }
        // heads
        _Pragma("unroll") for (int s = 0; s < LIMB_SLOTS; s++) {
            if ((u32)s < gcount) {
                const DevGate g = a.gates[la.gi[grp][s]];
                switch (g.type) {
                case GLP_GATE_U32_ARITHMETIC: gate_terms<NCH, GLP_GATE_U32_ARITHMETIC, true>(a, p, g, N, slot, k0, ga[s]); break;
                case GLP_GATE_U32_ADD_MANY: gate_terms<NCH, GLP_GATE_U32_ADD_MANY, true>(a, p, g, N, slot, k0, ga[s]); break;
                case GLP_GATE_U32_SUBTRACTION: gate_terms<NCH, GLP_GATE_U32_SUBTRACTION, true>(a, p, g, N, slot, k0, ga[s]); break;
                default: break;                    // U32RangeCheck: limb work only
                }
            }
        }
        for (u32 j0 = jlo; j0 <= jhi; j0 += 8) {
            u64 lv[8];
            _Pragma("unroll") for (int t = 0; t < 8; t++) if (j0 + t <= jhi) lv[t] = W[(size_t)(j0 + t) * N];
            _Pragma("unroll") for (int t = 0; t < 8; t++) if (j0 + t <= jhi) {
                const u64 v = lv[t];
                const u64 *dj = desc + (size_t)(j0 + t) * LIMB_SLOTS;
                const u64 rp = range_product(v, 4);
                _Pragma("unroll") for (int s = 0; s < LIMB_SLOTS; s++) {
                    const u64 d = dj[s];
                    if (d & 1) {
                        const u32 kl = (u32)(d >> 6) & 0x3FFu;
                        _Pragma("unroll") for (int c2 = 0; c2 < NCH; c2++) acc3_fma(ga[s][c2], rp, ap + APL_WORDS * ((size_t)c2 * nt + kl));
                        b4_add(bs[s], v, (u32)(d >> 1) & 15u);
                        if (d & 32) {
                            const u32 kf = (u32)(d >> 16) & 0x3FFu, ref = (u32)(d >> 26) & 0xFFu;
                            LIMB_EMIT(s, kf, sub(b4_value(bs[s]), W[(size_t)ref * N]));
                            b4_zero(bs[s]);
                        }
                    }
                }
            }
        }
        _Pragma("unroll") for (int s = 0; s < LIMB_SLOTS; s++) {
            if ((u32)s < gcount) {
                const u64 filter = gate_filter(a, a.gates[la.gi[grp][s]], N, slot);
                _Pragma("unroll") for (int c = 0; c < NCH; c++) acc[c] = add(acc[c], mul(filter, acc3_reduce(ga[s][c])));
            }
        }
    }
#undef LIMB_EMIT
    for (u32 t = 0; t < la.extra_count; t++) {             // after the limb accumulators are dead (register budget)
        const DevGate g = a.gates[la.extra_gi[t]];
        if (g.type == GLP_GATE_COMPARISON) gate_contrib<NCH, GLP_GATE_COMPARISON>(a, p, g, N, slot, k0, acc);
    }
    const size_t Rq = (size_t)gridDim.y;
    _Pragma("unroll") for (int c = 0; c < NCH; c++) {
        u64 *o = p.out + ((size_t)c * Rq + rq) * n + q;
        *o = add(*o, mul(acc[c], a.zh_inv[rq]));
    }
}

// K6b: after the per-plane inverse NTT: undo the plane twist, inverse DFT across planes, undo the coset shift.
//   V [nch][Rq][n] (bit-reversed k')  ->  chunk coefficients [nch*Rq][n] (bit-reversed), chunk c = X^(c n) block
struct QCArgs { const u64 *V; u64 *out; u64 wM_inv, wR_inv, g_inv, rq_inv; u64 gn_inv_pow[MAXR]; u32 lg, Rq; };
__global__ __launch_bounds__(256) void k_quotient_combine(QCArgs a) {
    const size_t n = (size_t)1 << a.lg;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const u32 ch = blockIdx.y, Rq = a.Rq;
    const u32 kp = bitrev32((u32)p, a.lg);
    const u64 tw = dpow(a.wM_inv, kp);            // w_M^-k'
    const u64 gk = mul(dpow(a.g_inv, kp), a.rq_inv);
    u64 y[MAXR];
    u64 t = 1;
    for (u32 r = 0; r < Rq; r++) { y[r] = mul(a.V[((size_t)ch * Rq + r) * n + p], t); t = mul(t, tw); }
    u64 wc = 1;                                    // w_Rq^-c
    for (u32 c = 0; c < Rq; c++) {
        u64 s = 0, w = 1;
        for (u32 r = 0; r < Rq; r++) { s = add(s, mul(y[r], w)); w = mul(w, wc); }
        a.out[((size_t)ch * Rq + c) * n + p] = mul(s, mul(gk, a.gn_inv_pow[c]));
        wc = mul(wc, a.wR_inv);
    }
}
