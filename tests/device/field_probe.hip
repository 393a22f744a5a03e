// field_probe.hip -- runs every primitive of csrc/glf.h, csrc/acc.h and the non-canonical Poseidon layers of csrc/poseidon.h on its
// own, one case per thread, over operands a test chooses.  It holds no expected value: tests/field_model.py writes the operands,
// computes the reference with Python integers and compares (tests/test_field_probe.py on the CPU, tests/test_gpu_field_probe.py on
// the GPU).
//
//     field_probe host|device <dir>
//
// For each operation of the table at the end it reads <dir>/<op>.in, applies the operation to every row and writes <dir>/<op>.out;
// both are raw little-endian u64, NIN words in and NOUT words out per case.  An operation whose .in file is absent is skipped.
//   device  one kernel per operation, 256 threads per block, one case per thread, each primitive called the way the library
//           calls it.  Every HIP return code is checked: the first failure ends the program with status 1 and HIP's error text.
//   host    the GLF_HD functions through their host bodies (and the host-only apl_words and host schedule of poseidon.h); no HIP
//           runtime call is made, so it runs on a machine without a GPU.  Device-only operations are left out.
//
// What a green run proves: the arithmetic of each primitive as hipcc compiles it HERE, with the library's flags.  It does not pin
// every inlined copy inside the library's kernels, where the surrounding schedule (and so the distance between an inline-assembly
// block that writes a carry and the one that reads it) differs.  Two chained operations narrow that gap, with one block's result
// feeding the next and nothing in between: sbox7_nc (four mul_nc_cc back to back) and mul_nc_chain = mul_nc(mul_nc(x, y), y).
//
// Of csrc/poseidon.h, layer by layer, each over ANY u64 the layer before may hand it (a whole-permutation test controls only the state
// that enters round 0, which passes an S-box layer before the first sum sees it):
//   sbox7_nc, sbox_layer_nc (twelve carry chains under the scheduling barriers), mds_add_nc, mds_add_wave (the int8 matrix pipe),
//   full_round_nc / full_round_wave = the S-box layer and a linear layer with nothing in between (the shape permute_body and k_quotient
//   inline), the six partial-round blocks plain and with a hook that replaces the S-box input (k_quotient's wire_in), permute_tail7,
//   pow_round0_consts, permute (host schedule and permute_body<false>) and permute_wave; on the host pos::host::fold, the six
//   pos::host::partial_block and pos::host::mds_add.
//   NOT run here: permute_coop and permute_quad.  They take canonical words and S-box them before any sum, so their unreduced rows
//   cannot be driven from outside; the Merkle tests cover them against the oracle.
// The operations that call a matrix instruction (mds_add_wave, full_round_wave, permute_wave) run under k_probe_wave: the instruction
// acts on all 64 lanes whatever the execution mask, so every lane computes (lanes past the end on row 0) and only the store is masked.
//
// Accumulator loops: a row is  N, (flags), then TERMS operand groups; the kernel runs N (clamped to TERMS) terms.  The *_flush
// forms reduce, add and zero every ACC_MAX_TERMS (ACC3_MAX_TERMS) terms, the pattern of k_open_dot.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>
#include "glf.h"
#include "acc.h"
#include "poseidon.h"

// row capacities of the accumulator loops (tests/field_model.py holds the same numbers)
constexpr u32 ACC_TERMS = 4096, ACC2_TERMS = 2 * ACC_MAX_TERMS + 3, ACC3_TERMS = 2 * ACC3_MAX_TERMS + 3;

#define PROBE_D __device__ __forceinline__
// NAME, words in, words out, callable on the host, body over (const u64 *x, u64 *y)
#define OP(NAME, NIN_, NOUT_, HOST_, QUAL, ...)                                                     \
    struct op_##NAME {                                                                              \
        static constexpr u32 NIN = NIN_, NOUT = NOUT_;                                              \
        static constexpr bool HOST = HOST_, APL = false;                                            \
        static const char *name() { return #NAME; }                                                 \
        static QUAL void run(const u64 *x, u64 *y) { __VA_ARGS__ }                                  \
    };
#define OP_HD(NAME, NIN_, NOUT_, ...) OP(NAME, NIN_, NOUT_, true, GLF_HD, __VA_ARGS__)
#define OP_D(NAME, NIN_, NOUT_, ...) OP(NAME, NIN_, NOUT_, false, PROBE_D, __VA_ARGS__)

PROBE_D void put(u64 *y, ext2 e) { y[0] = e.a; y[1] = e.b; }
static inline void put_h(u64 *y, ext2 e) { y[0] = e.a; y[1] = e.b; }
#if defined(__HIP_DEVICE_COMPILE__)
#define PUT put
#else
#define PUT put_h
#endif

// ---- canonical -> canonical -----------------------------------------------------------------------------------------------
OP_HD(add, 2, 1, y[0] = add(x[0], x[1]);)
OP_HD(sub, 2, 1, y[0] = sub(x[0], x[1]);)
OP_HD(neg, 1, 1, y[0] = neg(x[0]);)
OP_HD(dbl, 1, 1, y[0] = dbl(x[0]);)
OP_HD(pow, 2, 1, y[0] = pow(x[0], x[1]);)
OP_HD(inv, 1, 1, y[0] = inv(x[0]);)
OP_HD(e_add, 4, 2, PUT(y, e_add(e_make(x[0], x[1]), e_make(x[2], x[3])));)
OP_HD(e_sub, 4, 2, PUT(y, e_sub(e_make(x[0], x[1]), e_make(x[2], x[3])));)
OP_HD(e_neg, 2, 2, PUT(y, e_neg(e_make(x[0], x[1])));)
OP_HD(e_mul, 4, 2, PUT(y, e_mul(e_make(x[0], x[1]), e_make(x[2], x[3])));)
OP_HD(e_sqr, 2, 2, PUT(y, e_sqr(e_make(x[0], x[1])));)
OP_HD(e_scale, 3, 2, PUT(y, e_scale(e_make(x[0], x[1]), x[2]));)
OP_HD(e_inv, 2, 2, PUT(y, e_inv(e_make(x[0], x[1])));)
OP_HD(e_pow, 3, 2, PUT(y, e_pow(e_make(x[0], x[1]), x[2]));)
// ---- any u64 -> canonical -------------------------------------------------------------------------------------------------
OP_HD(canon, 1, 1, y[0] = canon(x[0]);)
OP_HD(mul, 2, 1, y[0] = mul(x[0], x[1]);)
OP_HD(sqr, 1, 1, y[0] = sqr(x[0]);)
OP_HD(reduce128, 2, 1, y[0] = reduce128(x[0], x[1]);)
OP_HD(reduce96, 2, 1, y[0] = reduce96(x[0], (u32)x[1]);)
OP_HD(mul_2exp, 2, 1, y[0] = mul_2exp(x[0], (u32)x[1]);)
OP_D(mul_c, 2, 1, y[0] = mul_c(x[0], x[1]);)

template <int... I>
PROBE_D u64 mul_pow2_any(u64 v, u32 e, std::integer_sequence<int, I...>) {      // e = 1..95 -> mul_pow2_c<e>(v)
    u64 r = 0;
    (void)((e == (u32)(I + 1) ? (r = mul_pow2_c<I + 1>(v), true) : false) || ...);
    return r;
}
OP_D(mul_pow2_c, 2, 1, y[0] = mul_pow2_any(x[0], (u32)x[1], std::make_integer_sequence<int, 95>());)
OP_D(b4_value, 16, 1,
     Base4Sum b; b4_zero(b);
     for (u32 j = 0; j < 16; j++) b4_add(b, x[j], j);
     y[0] = b4_value(b);)
OP_D(acc_reduce, 5, 1,
     Acc160 a; a.w0 = (u32)x[0]; a.w1 = (u32)x[1]; a.w2 = (u32)x[2]; a.w3 = (u32)x[3]; a.w4 = (u32)x[4];
     y[0] = acc_reduce(a);)
OP_D(acc2_reduce, 6, 1,
     AccLimb a; a.a00 = x[0]; a.a01 = x[1]; a.a10 = x[2]; a.a11 = x[3]; a.a20 = x[4]; a.a21 = x[5];
     y[0] = acc2_reduce(a);)
OP_D(acc3_reduce, 3, 1,
     AccHL a; a.c0 = x[0]; a.c1 = x[1]; a.c2 = x[2];
     y[0] = acc3_reduce(a);)
// ---- any u64 -> some u64 congruent mod p (device only) --------------------------------------------------------------------
OP_D(mul_nc, 2, 1, y[0] = mul_nc(x[0], x[1]);)
OP_D(mul_nc_cc, 2, 1, y[0] = mul_nc_cc(x[0], x[1]);)
OP_D(mul_nc_chain, 2, 1, y[0] = mul_nc(mul_nc(x[0], x[1]), x[1]);)
OP_D(fold96_nc, 2, 1, y[0] = fold96_nc(x[0], (u32)x[1]);)
OP_D(fold96_c, 2, 1, y[0] = fold96_c(x[0], (u32)x[1]);)
OP_D(fold128_nc, 2, 1, y[0] = fold128_nc((u32)x[0], (u32)(x[0] >> 32), (u32)x[1], (u32)(x[1] >> 32));)
OP_D(fold128_mad_nc, 2, 1, y[0] = fold128_mad_nc(x[0], x[1]);)
OP_D(mul_small_nc, 2, 1, y[0] = mul_small_nc(x[0], (u32)x[1]);)
OP_D(add_cnc, 2, 1, y[0] = add_cnc(x[0], x[1]);)
OP_D(range_product, 2, 1, y[0] = range_product(x[0], (u32)x[1]);)
OP_D(sbox7_nc, 1, 1, y[0] = pos::sbox7_nc(x[0]);)
OP_D(mds_add_nc, 24, 12,
     u64 s[12];
     for (int i = 0; i < 12; i++) s[i] = x[i];
#if defined(__HIP_DEVICE_COMPILE__)
     pos::mds_add_nc(s, x + 12);
#endif
     for (int i = 0; i < 12; i++) y[i] = s[i];)
// ---- the layers of csrc/poseidon.h (device schedule; the host pass of hipcc does not declare these names) --------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define PROBE_DEV(...) __VA_ARGS__
#define PROBE_HOST(...)
#else
#define PROBE_DEV(...)
#define PROBE_HOST(...) __VA_ARGS__
#endif
#define LOAD12 u64 s[12]; for (int i = 0; i < 12; i++) s[i] = x[i];
#define STORE12 for (int i = 0; i < 12; i++) y[i] = s[i];
// an operation that calls a matrix instruction: run by k_probe_wave, y is the lane's own array, mo = pos::mds_operands()
#define OP_W(NAME, NIN_, NOUT_, ...)                                                                \
    struct op_##NAME {                                                                              \
        static constexpr u32 NIN = NIN_, NOUT = NOUT_;                                              \
        static constexpr bool HOST = false, APL = false, WAVE = true;                               \
        static const char *name() { return #NAME; }                                                 \
        static PROBE_D void run(const u64 *x, u64 *y, const pos::MdsOperands &mo) { PROBE_DEV(__VA_ARGS__) }  \
    };
OP_W(mds_add_wave, 24, 12, LOAD12 pos::mds_add_wave(s, x + 12, mo); STORE12)
OP_D(sbox_layer_nc, 12, 12, LOAD12 PROBE_DEV(pos::sbox_layer_nc(s);) STORE12)
OP_D(full_round_nc, 24, 12, LOAD12 PROBE_DEV(pos::sbox_layer_nc(s); pos::mds_add_nc(s, x + 12);) STORE12)
OP_W(full_round_wave, 24, 12, LOAD12 pos::sbox_layer_nc(s); pos::mds_add_wave(s, x + 12, mo); STORE12)
// K partial rounds as one block: rounds 3 (linear layer) + 4..6, 7..10, 11..14, 15..18, 19..22, 23..25
#define PBLOCK_OP(NAME, K, MERGED, KC)                                                              \
    OP_D(NAME, 12, 12, LOAD12 PROBE_DEV(pos::partial_block_nc<K, MERGED>(s, KC);) STORE12)          \
    /* row: the state, then the word the hook returns in place of z_j (k_quotient's wire_in); out: the state, then each z_j */  \
    OP_D(NAME##_hook, 12 + K, 12 + K, LOAD12                                                        \
         PROBE_DEV(pos::partial_block_nc<K, MERGED>(s, KC, [&](int j, u64 z) { y[12 + j] = z; return x[12 + j]; });) STORE12)
PBLOCK_OP(pblock_m3, 3, true, pos::PBM[0])
PBLOCK_OP(pblock_4a, 4, false, pos::PB4[0])
PBLOCK_OP(pblock_4b, 4, false, pos::PB4[1])
PBLOCK_OP(pblock_4c, 4, false, pos::PB4[2])
PBLOCK_OP(pblock_4d, 4, false, pos::PB4[3])
PBLOCK_OP(pblock_3, 3, false, pos::PB3[0])
// ---- canonical out (device only) ------------------------------------------------------------------------------------------
OP_D(tail7, 12, 1, LOAD12 PROBE_DEV(y[0] = pos::permute_tail7(s);))
OP_D(pow_round0_consts, 13, 12, PROBE_DEV(u64 s[12]; pos::pow_round0_consts(x, (u32)x[12], s); STORE12))
OP_W(permute_wave, 12, 12, LOAD12 pos::permute_wave(s, mo); STORE12)
// host: the host schedule of poseidon.h; device: permute_body<false>
OP_HD(permute, 12, 12, LOAD12 PROBE_DEV(pos::permute_body<false>(s, pos::MdsOperands{});) PROBE_HOST(pos::permute(s);) STORE12)
// ---- exact ----------------------------------------------------------------------------------------------------------------
template <int E> PROBE_D void add_shifted(Acc160 &w, u64 v, u32 e) { if (e == (u32)E) acc_add_shifted<E>(w, v); }
OP_D(acc_add_shifted, 7, 5,           // w0..w4, v, E -> w + (v << E) mod 2^160 for the E of acc2_reduce and acc3_reduce
     Acc160 a; a.w0 = (u32)x[0]; a.w1 = (u32)x[1]; a.w2 = (u32)x[2]; a.w3 = (u32)x[3]; a.w4 = (u32)x[4];
     const u32 e = (u32)x[6];
     add_shifted<0>(a, x[5], e); add_shifted<22>(a, x[5], e); add_shifted<32>(a, x[5], e);
     add_shifted<44>(a, x[5], e); add_shifted<54>(a, x[5], e); add_shifted<76>(a, x[5], e);
     y[0] = a.w0; y[1] = a.w1; y[2] = a.w2; y[3] = a.w3; y[4] = a.w4;)
OP_HD(root_of_unity, 1, 1, y[0] = root_of_unity((int)x[0]);)
OP_HD(bitrev32, 2, 1, y[0] = bitrev32((u32)x[0], (int)x[1]);)
// ---- accumulator loops ----------------------------------------------------------------------------------------------------
PROBE_D u32 clamp_terms(u64 n, u32 cap) { return n < cap ? (u32)n : cap; }
// row: N, then (v, m) per term
OP_D(acc_loop, 1 + 2 * ACC_TERMS, 1,
     Acc160 a; acc_zero(a);
     const u32 n = clamp_terms(x[0], ACC_TERMS);
     for (u32 k = 0; k < n; k++) acc_fma(a, x[1 + 2 * k], x[2 + 2 * k]);
     y[0] = acc_reduce(a);)
OP_D(acc_flush, 1 + 2 * ACC_TERMS, 1,
     Acc160 a; acc_zero(a);
     u64 s = 0; u32 terms = 0;
     const u32 n = clamp_terms(x[0], ACC_TERMS);
     for (u32 k = 0; k < n; k++) {
         acc_fma(a, x[1 + 2 * k], x[2 + 2 * k]);
         if (++terms == ACC_MAX_TERMS) { s = add(s, acc_reduce(a)); acc_zero(a); terms = 0; }
     }
     y[0] = add(s, acc_reduce(a));)
// row: N, then (c, m) per term; c is cut into 22-bit limbs the way k_open_dot cuts a coefficient
OP_D(acc2_loop, 1 + 2 * ACC2_TERMS, 1,
     AccLimb a; acc2_zero(a);
     const u32 n = clamp_terms(x[0], ACC2_TERMS);
     for (u32 k = 0; k < n; k++) {
         const u64 c = x[1 + 2 * k];
         acc2_fma(a, (u32)c & 0x3FFFFFu, (u32)(c >> 22) & 0x3FFFFFu, (u32)(c >> 44), x[2 + 2 * k]);
     }
     y[0] = acc2_reduce(a);)
OP_D(acc2_flush, 1 + 2 * ACC2_TERMS, 1,
     AccLimb a; acc2_zero(a);
     u64 s = 0; u32 terms = 0;
     const u32 n = clamp_terms(x[0], ACC2_TERMS);
     for (u32 k = 0; k < n; k++) {
         const u64 c = x[1 + 2 * k];
         acc2_fma(a, (u32)c & 0x3FFFFFu, (u32)(c >> 22) & 0x3FFFFFu, (u32)(c >> 44), x[2 + 2 * k]);
         if (++terms == ACC_MAX_TERMS) { s = add(s, acc2_reduce(a)); acc2_zero(a); terms = 0; }
     }
     y[0] = add(s, acc2_reduce(a));)
// row: N, from_m, then (v, w0, w1, w2, w3) per term: the table words of one multiplier.  from_m != 0: w0 holds the multiplier m
// itself and the HOST side of this program fills w0..w3 with apl_words(m) before the upload, as the prover fills its table.
#define ACC3_OP(NAME, ...)                                                                          \
    struct op_##NAME {                                                                              \
        static constexpr u32 NIN = 2 + 5 * ACC3_TERMS, NOUT = 1;                                    \
        static constexpr bool HOST = false, APL = true;                                             \
        static const char *name() { return #NAME; }                                                 \
        static PROBE_D void run(const u64 *x, u64 *y) { __VA_ARGS__ }                               \
    };
ACC3_OP(acc3_loop,
        AccHL a; acc3_zero(a);
        const u32 n = clamp_terms(x[0], ACC3_TERMS);
        for (u32 k = 0; k < n; k++) acc3_fma(a, x[2 + 5 * k], x + 3 + 5 * k);
        y[0] = acc3_reduce(a);)
ACC3_OP(acc3_flush,
        AccHL a; acc3_zero(a);
        u64 s = 0; u32 terms = 0;
        const u32 n = clamp_terms(x[0], ACC3_TERMS);
        for (u32 k = 0; k < n; k++) {
            acc3_fma(a, x[2 + 5 * k], x + 3 + 5 * k);
            if (++terms == ACC3_MAX_TERMS) { s = add(s, acc3_reduce(a)); acc3_zero(a); terms = 0; }
        }
        y[0] = add(s, acc3_reduce(a));)
static void fill_apl_rows(std::vector<u64> &in) {
    const size_t nin = 2 + 5 * (size_t)ACC3_TERMS;
    for (size_t r = 0; r + nin <= in.size(); r += nin) {
        if (!in[r + 1]) continue;
        const size_t n = in[r] < ACC3_TERMS ? (size_t)in[r] : ACC3_TERMS;
        for (size_t k = 0; k < n; k++) apl_words(in[r + 3 + 5 * k], &in[r + 3 + 5 * k]);
    }
}
// host only: m -> the four table words
struct op_apl_words {
    static constexpr u32 NIN = 1, NOUT = 4;
    static constexpr bool HOST = true, APL = false, DEVICE = false;
    static const char *name() { return "apl_words"; }
    static void run(const u64 *x, u64 *y) { apl_words(x[0], y); }
};
// host only: the host schedule's fold (al, ah, k), its six blocks (any u64 in) and its full-round linear layer (canonical in and out)
#define OP_H(NAME, NIN_, NOUT_, ...)                                                                \
    struct op_##NAME {                                                                              \
        static constexpr u32 NIN = NIN_, NOUT = NOUT_;                                              \
        static constexpr bool HOST = true, APL = false, DEVICE = false;                             \
        static const char *name() { return #NAME; }                                                 \
        static void run(const u64 *x, u64 *y) { PROBE_HOST(__VA_ARGS__) }                           \
    };
OP_H(host_fold, 3, 1, y[0] = pos::host::fold(x[0], x[1], x[2]);)
OP_H(host_pblock_m3, 12, 12, LOAD12 pos::host::partial_block<3, true>(s, pos::host::HPBM); STORE12)
OP_H(host_pblock_4a, 12, 12, LOAD12 pos::host::partial_block<4, false>(s, pos::host::HPB4[0]); STORE12)
OP_H(host_pblock_4b, 12, 12, LOAD12 pos::host::partial_block<4, false>(s, pos::host::HPB4[1]); STORE12)
OP_H(host_pblock_4c, 12, 12, LOAD12 pos::host::partial_block<4, false>(s, pos::host::HPB4[2]); STORE12)
OP_H(host_pblock_4d, 12, 12, LOAD12 pos::host::partial_block<4, false>(s, pos::host::HPB4[3]); STORE12)
OP_H(host_pblock_3, 12, 12, LOAD12 pos::host::partial_block<3, false>(s, pos::host::HPB3); STORE12)
OP_H(host_mds_add, 24, 12, LOAD12 pos::host::mds_add(s, x + 12); STORE12)

// ---- driver ---------------------------------------------------------------------------------------------------------------
template <class Op>
__global__ __launch_bounds__(256) void k_probe(const u64 *in, u64 *out, u64 n) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Op::run(in + i * Op::NIN, out + i * Op::NOUT);
}

template <class Op, class = void> struct is_wave { static constexpr bool value = false; };
template <class Op> struct is_wave<Op, std::enable_if_t<Op::WAVE>> { static constexpr bool value = true; };
// the same for an operation that calls a matrix instruction: control flow is wave-uniform up to the call, every lane computes (the
// lanes past the end on row 0, as the kernels of merkle.hip do) and only the store is masked
template <class Op>
__global__ __launch_bounds__(256) void k_probe_wave(const u64 *in, u64 *out, u64 n) {
    const u64 i0 = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool live = i0 < n;
    const u64 i = live ? i0 : 0;
    const pos::MdsOperands mo = pos::mds_operands();
    u64 y[Op::NOUT];
    Op::run(in + i * Op::NIN, y, mo);
    if (live)
        for (u32 k = 0; k < Op::NOUT; k++) out[i * Op::NOUT + k] = y[k];
}

#define HIP_OK(call)                                                                                \
    do {                                                                                            \
        const hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "field_probe: %s: %s: %s\n", op, #call, hipGetErrorString(e_));         \
            exit(1);                                                                                \
        }                                                                                           \
    } while (0)

static bool read_words(const std::string &path, std::vector<u64> &v) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % 8) { fprintf(stderr, "field_probe: %s: not a whole number of words\n", path.c_str()); exit(1); }
    v.resize((size_t)bytes / 8);
    if (!v.empty() && fread(v.data(), 8, v.size(), f) != v.size()) { fprintf(stderr, "field_probe: %s: short read\n", path.c_str()); exit(1); }
    fclose(f);
    return true;
}
static void write_words(const std::string &path, const std::vector<u64> &v) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && fwrite(v.data(), 8, v.size(), f) != v.size()) || fclose(f)) {
        fprintf(stderr, "field_probe: cannot write %s\n", path.c_str());
        exit(1);
    }
}

template <class Op, class = void> struct on_device { static constexpr bool value = true; };
template <class Op> struct on_device<Op, std::enable_if_t<!Op::DEVICE>> { static constexpr bool value = false; };

template <class Op>
static void run_device(const char *op, const std::vector<u64> &in, std::vector<u64> &out, size_t n) {
    if constexpr (on_device<Op>::value) {
        u64 *d_in = nullptr, *d_out = nullptr;
        HIP_OK(hipMalloc(&d_in, in.size() * 8));
        HIP_OK(hipMalloc(&d_out, out.size() * 8));
        HIP_OK(hipMemcpy(d_in, in.data(), in.size() * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0xA5, out.size() * 8));
        if constexpr (is_wave<Op>::value) hipLaunchKernelGGL(k_probe_wave<Op>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, (u64)n);
        else hipLaunchKernelGGL(k_probe<Op>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, (u64)n);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_in));
        HIP_OK(hipFree(d_out));
    }
}
template <class Op>
static void run_host(const std::vector<u64> &in, std::vector<u64> &out, size_t n) {
    if constexpr (Op::HOST)
        for (size_t i = 0; i < n; i++) Op::run(in.data() + i * Op::NIN, out.data() + i * Op::NOUT);
}

template <class Op>
static void run_op(bool device, const std::string &dir, unsigned &done) {
    if (device ? !on_device<Op>::value : !Op::HOST) return;
    std::vector<u64> in;
    if (!read_words(dir + "/" + Op::name() + ".in", in)) return;
    if (in.empty() || in.size() % Op::NIN) {
        fprintf(stderr, "field_probe: %s.in: %zu words is not a whole number of %u-word rows\n", Op::name(), in.size(), Op::NIN);
        exit(1);
    }
    const size_t n = in.size() / Op::NIN;
    if constexpr (Op::APL) fill_apl_rows(in);
    std::vector<u64> out(n * Op::NOUT);
    if (device) run_device<Op>(Op::name(), in, out, n);
    else run_host<Op>(in, out, n);
    write_words(dir + "/" + Op::name() + ".out", out);
    done++;
}
template <class... Ops>
static unsigned run_all(bool device, const std::string &dir) {
    unsigned done = 0;
    (run_op<Ops>(device, dir, done), ...);
    return done;
}

int main(int argc, char **argv) {
    if (argc != 3 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) {
        fprintf(stderr, "usage: field_probe host|device <dir>\n");
        return 2;
    }
    const bool device = !strcmp(argv[1], "device");
    const unsigned done = run_all<
        op_add, op_sub, op_neg, op_dbl, op_pow, op_inv, op_e_add, op_e_sub, op_e_neg, op_e_mul, op_e_sqr, op_e_scale, op_e_inv, op_e_pow,
        op_canon, op_mul, op_sqr, op_reduce128, op_reduce96, op_mul_2exp, op_mul_c, op_mul_pow2_c, op_b4_value, op_acc_reduce,
        op_acc2_reduce, op_acc3_reduce, op_mul_nc, op_mul_nc_cc, op_mul_nc_chain, op_fold96_nc, op_fold96_c, op_fold128_nc,
        op_fold128_mad_nc, op_mul_small_nc, op_add_cnc, op_range_product, op_sbox7_nc, op_mds_add_nc, op_mds_add_wave, op_sbox_layer_nc,
        op_full_round_nc, op_full_round_wave, op_pblock_m3, op_pblock_m3_hook, op_pblock_4a, op_pblock_4a_hook, op_pblock_4b, op_pblock_4b_hook,
        op_pblock_4c, op_pblock_4c_hook, op_pblock_4d, op_pblock_4d_hook, op_pblock_3, op_pblock_3_hook, op_tail7, op_pow_round0_consts,
        op_permute_wave, op_permute, op_acc_add_shifted,
        op_root_of_unity, op_bitrev32, op_acc_loop, op_acc_flush, op_acc2_loop, op_acc2_flush, op_acc3_loop, op_acc3_flush,
        op_apl_words, op_host_fold, op_host_pblock_m3, op_host_pblock_4a, op_host_pblock_4b, op_host_pblock_4c, op_host_pblock_4d,
        op_host_pblock_3, op_host_mds_add>(device, argv[2]);
    printf("field_probe %s: %u operations\n", argv[1], done);
    return 0;
}
