// acc.h -- the unreduced accumulators of the gate bodies and of the FRI / opening sums: range_product, Base4Sum, Acc160 (five 32-bit
// words with carries), AccLimb and AccHL (carry-free 64-bit registers with a term bound) and the host side of AccHL's multiplier table.
// Needs glf.h only; included by quotient_kernels.inc, and by tests/device/field_probe.hip, which runs every function here on its own.
#pragma once
#include "glf.h"
using namespace glf;

// prod_{x < bound} (v - x), v canonical -> NON-canonical u64 (it only ever feeds acc_fma, which takes any u64)
__device__ __forceinline__ u64 range_product(u64 v, u32 bound) {
    if (bound == 4) {                       // v(v-3) * (v-1)(v-2) = u (u + 2): two multiplications instead of three
        // (mul_nc, not mul_nc_cc: in k_quotient_limbs the carry-chain form measured 7.33 -> 7.83 ms, in the permutation loop 5.85 -> 5.66)
        const u64 u = mul_nc(v, add_cnc(v, P - 3));       // v - 3 as v + (p - 3), left non-canonical; u any u64
        return mul_nc(u, add_cnc(2, u));
    }
    u64 p = v;
    for (u32 x = 1; x + 1 < bound; x++) p = mul(p, sub(v, (u64)x));
    return bound > 1 ? mul_nc(p, sub(v, (u64)(bound - 1))) : p;
}
// sum_j 4^j limb_j over up to 16 canonical limbs without a modular operation per limb: the 32-bit halves are
// accumulated separately (each sum < 2^32 (4^16 - 1) / 3 < 2^64 / 3) and folded once.
struct Base4Sum { u64 lo, hi; };
__device__ __forceinline__ void b4_zero(Base4Sum &b) { b.lo = 0; b.hi = 0; }
__device__ __forceinline__ void b4_add(Base4Sum &b, u64 limb, u32 j /* < 16 */) {
    const u32 w = 1u << (2 * j);
    b.lo += (u64)(u32)limb * w;
    b.hi += (u64)(u32)(limb >> 32) * w;
}
__device__ __forceinline__ u64 b4_value(const Base4Sum &b) {       // canonical
    const u64 l = b.lo + (b.hi << 32);
    const u32 h = (u32)(b.hi >> 32) + (l < b.lo ? 1u : 0u);
    return canon(fold96_nc(l, h));
}
// Unreduced accumulator for sum_k c_k * alpha^k: 128-bit products are added into five 32-bit words and folded
// once per gate instead of once per constraint (a modular multiply-add costs ~40 issue slots, this ~19).
struct Acc160 { u32 w0, w1, w2, w3, w4; };
__device__ __forceinline__ void acc_zero(Acc160 &a) { a.w0 = a.w1 = a.w2 = a.w3 = a.w4 = 0; }
__device__ __forceinline__ void acc_fma(Acc160 &a, u64 v, u64 m) {
    const u32 v0 = (u32)v, v1 = (u32)(v >> 32), m0 = (u32)m, m1 = (u32)(m >> 32);
    const u64 p00 = (u64)v0 * m0;
    const u64 p01 = (u64)v0 * m1 + (p00 >> 32);
    const u64 p10 = (u64)v1 * m0 + (u32)p01;
    const u64 p11 = (u64)v1 * m1 + (p01 >> 32) + (p10 >> 32);
    u32 c;
    a.w0 = __builtin_addc(a.w0, (u32)p00, 0u, &c);
    a.w1 = __builtin_addc(a.w1, (u32)p10, c, &c);
    a.w2 = __builtin_addc(a.w2, (u32)p11, c, &c);
    a.w3 = __builtin_addc(a.w3, (u32)(p11 >> 32), c, &c);
    a.w4 += c;
}
__device__ __forceinline__ u64 acc_reduce(const Acc160 &a) {      // canonical
    const u64 h = fold96_nc(((u64)a.w3 << 32) | a.w2, a.w4);       // (w2 + w3 2^32 + w4 2^64) mod p
    return canon(fold128_nc(a.w0, a.w1, (u32)h, (u32)(h >> 32)));
}

// Gate constraints: sum_k v_k alpha^k with NO carries per term.  v is cut into 22-bit limbs and alpha^k into 32-bit
// halves; each of the six limb products (< 2^54) is accumulated in its own 64-bit register by one v_mad_u64_u32, so up
// to 1024 terms fit before anything can overflow (glp_circuit_create rejects gates with more constraints).  6 issue
// slots per term against 14 for the 160-bit carry chain above; the limbs of v are shared by all challenges.
constexpr u32 ACC_MAX_TERMS = 1024;
struct AccLimb { u64 a00, a01, a10, a11, a20, a21; };     // a[i][j]: limb i of v (bits 22 i ..) times half j of m
__device__ __forceinline__ void acc2_zero(AccLimb &a) { a.a00 = a.a01 = a.a10 = a.a11 = a.a20 = a.a21 = 0; }
__device__ __forceinline__ void acc2_fma(AccLimb &a, u32 v0, u32 v1, u32 v2, u64 m) {
    const u32 m0 = (u32)m, m1 = (u32)(m >> 32);
    a.a00 += (u64)v0 * m0; a.a01 += (u64)v0 * m1;
    a.a10 += (u64)v1 * m0; a.a11 += (u64)v1 * m1;
    a.a20 += (u64)v2 * m0; a.a21 += (u64)v2 * m1;
}
template <int E> __device__ __forceinline__ void acc_add_shifted(Acc160 &w, u64 x) {   // w += x << E
    constexpr int idx = E / 32, sh = E % 32;
    const u64 lo = x << sh;
    const u32 t0 = (u32)lo, t1 = (u32)(lo >> 32);
    u32 t2 = 0;
    if constexpr (sh != 0) t2 = (u32)(x >> (64 - sh));
    u32 *W[5] = {&w.w0, &w.w1, &w.w2, &w.w3, &w.w4};
    u32 c;
    *W[idx] = __builtin_addc(*W[idx], t0, 0u, &c);
    *W[idx + 1] = __builtin_addc(*W[idx + 1], t1, c, &c);
    *W[idx + 2] = __builtin_addc(*W[idx + 2], t2, c, &c);
    if constexpr (idx + 3 < 5) *W[idx + 3] = __builtin_addc(*W[idx + 3], 0u, c, &c);
    if constexpr (idx + 4 < 5) *W[idx + 4] = __builtin_addc(*W[idx + 4], 0u, c, &c);
}
__device__ __forceinline__ u64 acc2_reduce(const AccLimb &a) {    // canonical
    Acc160 w;
    acc_zero(w);
    acc_add_shifted<0>(w, a.a00); acc_add_shifted<22>(w, a.a10); acc_add_shifted<32>(w, a.a01);
    acc_add_shifted<44>(w, a.a20); acc_add_shifted<54>(w, a.a11); acc_add_shifted<76>(w, a.a21);
    return acc_reduce(w);
}

// The same carry-free scheme with the roles swapped, for the quotient: the multiplier alpha^k comes from a table the host
// cuts into 22-bit limbs once per proof, so a constraint value enters as its two 32-bit halves -- the registers it already
// lives in -- instead of being cut into three limbs per term (5 shift / mask slots per constraint, 620 constraints per point).
// m enters TWICE, as m and as m' = m 2^32 mod p: then  v m = vlo m + vhi m'  and both products sit at the same limb weights, so
// three accumulators per sum are enough (six if the 2^32 is left to the weights).  Half the registers per gate in the quotient
// kernels -- what bounds how many gates share one pass over the wire planes -- for twice the (scalar) table loads.
struct AccHL { u64 c0, c1, c2; };                         // c[j]: limb j of m (bits 22 j ..) times vlo + limb j of m' times vhi
constexpr u32 ACC3_MAX_TERMS = 512;                       // 2 products < 2^54 per term and accumulator
inline void apl_words(u64 m, u64 out[4]) {                // host side of the table
    const u64 mp = glf::mul(m, 1ull << 32);
    out[0] = (m & 0x3FFFFFull) | (((m >> 22) & 0x3FFFFFull) << 32); out[1] = m >> 44;
    out[2] = (mp & 0x3FFFFFull) | (((mp >> 22) & 0x3FFFFFull) << 32); out[3] = mp >> 44;
}
__device__ __forceinline__ void acc3_zero(AccHL &a) { a.c0 = a.c1 = a.c2 = 0; }
__device__ __forceinline__ void acc3_fma(AccHL &a, u64 v, const u64 *ml) {
    const u32 vlo = (u32)v, vhi = (u32)(v >> 32);
    const u64 w0 = ml[0], w1 = ml[1], w2 = ml[2], w3 = ml[3];
    a.c0 += (u64)vlo * (u32)w0; a.c1 += (u64)vlo * (u32)(w0 >> 32); a.c2 += (u64)vlo * (u32)w1;
    a.c0 += (u64)vhi * (u32)w2; a.c1 += (u64)vhi * (u32)(w2 >> 32); a.c2 += (u64)vhi * (u32)w3;
}
__device__ __forceinline__ u64 acc3_reduce(const AccHL &a) {      // canonical
    Acc160 w;
    acc_zero(w);
    acc_add_shifted<0>(w, a.c0); acc_add_shifted<22>(w, a.c1); acc_add_shifted<44>(w, a.c2);
    return acc_reduce(w);
}
