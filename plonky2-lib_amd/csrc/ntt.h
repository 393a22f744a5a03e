// ntt.h -- batched Goldilocks NTT / iNTT / low-degree extension over column-major device arrays.
//
// Device layouts (chosen for coalescing on gfx950, not plonky2's host layouts):
//   trace values   [ncols][n]            natural order (row i = w^i)
//   coefficients   [ncols][n]            BIT-REVERSED order: slot p holds the coefficient of X^bitrev(p)
//   LDE values     [ncols][R][n]         "coset-major": slot (r, q) holds p(shift * W^(q*R + r)),
//                                        R = 2^rate_bits, W = primitive_root_of_unity(log_n + rate_bits)
// An inverse transform is decimation-in-frequency (natural -> bit-reversed), a forward one
// decimation-in-time (bit-reversed -> natural), so no permutation pass ever touches HBM.
// Kernels by size (ntt.hip; forward = k_lde_*, inverse = k_intt_*):
//   n <= 2^4          k_lde_small / k_intt_small: one thread per (column, coset), the transform on registers
//   n = 2^5 .. 2^8    k_lde_mid (all cosets of a column in one LDS tile); inverse: k_intt_contig
//   n = 2^9 .. 2^11   k_lde_contig / k_intt_contig: one tile of n elements, radix-2 stages in LDS
//   n = 2^12 .. 2^22  two passes, n = A * 4096: k_lde_contig16 / k_intt_contig16 over B = 4096 contiguous elements (three
//                     16-point steps) and a strided pass over A rows (128-byte row segments), chosen by strided_pass():
//                       A = 2 .. 16      k_outer<.., TW = false>  A-point register transform, no LDS
//                       A = 32 .. 128    k_strided16e             16-point step, LDS exchange, A/16-point tail
//                       A = 256          k_strided16              two 16-point steps
//                       A = 512, 1024    k_strided32              32-point step, A/32-point step; tiles of 64-128 KB in the
//                                                                 160 KB LDS of gfx950
//   n = 2^23, 2^24    three passes: the two above per 2^20 block, then k_outer with twiddles over the n / 2^20 blocks
// Every transform on a thread's registers (16 / 32 points and the shorter tails) is dft_reg_dit / dft_reg_dif: the 64th
// roots of unity are powers of two, so those butterflies are shifts.
#pragma once
#include "common.h"

namespace glp {

constexpr int NTT_2PASS_LG = 22;    // two-pass limit: B <= 2^12 (contiguous), A <= 2^10 (strided; 2^9 and 2^10 in k_strided32).
                                    // glp_ctx::two_pass_lg (GLP_NTT_2PASS_LG in the environment: 20..22) lowers it per context
constexpr int NTT_INNER_LG = 20;    // above the two-pass limit: per 2^20 block the two-pass transform, then an outer strided pass
constexpr int NTT_MAX_LG = 24;      //   over A' = n / 2^20 <= 16 blocks (three passes)
constexpr int NTT_LGB_MAX = 12;
constexpr int NTT_STRIDED_W = 16;   // columns per strided tile (16 x 8 B = one 128-B line per row)
// What one launch carries in grid.y (columns, coset planes, outer blocks, channels) or grid.z.  hipDeviceProp_t::maxGridSize is
// {2^31 - 1, 65536, 65536} on the MI355X; ROCm 7 was seen to run grids past that in y (profiles/r20_wide_columns_tests.txt), but only
// the reported limit is a promise, and 65535 is inside it on every HIP platform.  Every function whose column count is the caller's
// walks the columns in ranges of at most this many and offsets its pointers by the range's first column.
constexpr u32 GRID_YZ_MAX = 65535;

struct NttPlan {
    int lg, lgA, lgB;
    u64 *tw_B = nullptr, *itw_B = nullptr;   // w_B^j / w_B^-j, j < B/2
    u64 *tw4096 = nullptr, *itw4096 = nullptr;  // w_4096^(+-j), j < 4096: inter-step twiddles of the register kernels
    u64 w_n, w_n_inv, n_inv;
    // three-pass plans only (lg above the context's two-pass limit): n = A' * 2^20
    int lgAo = 0;
    const NttPlan *inner = nullptr;          // the 2^20 plan
    u64 *it0 = nullptr, *it1 = nullptr;      // inverse outer twiddle: (w_n^-k1o)^q = it1[pbo][q >> 10] * it0[pbo][q & 1023], it1 carries 1/A'
    NttPlan() = default;
    NttPlan(const NttPlan &) = delete;
    NttPlan &operator=(const NttPlan &) = delete;
    ~NttPlan() {                             // tables belong to the plan: an error path that drops a half-built plan frees them
        for (u64 *t : {tw_B, itw_B, tw4096, itw4096, it0, it1}) if (t) (void)hipFree(t);
    }
};

struct LdePlan {
    const NttPlan *ntt;
    int rate_bits;
    u64 shift;
    u64 *pre = nullptr;      // [R][B]: (s_r^A)^bitrev_B(pl),  s_r = shift * W^r
    u64 *s_r = nullptr;      // [R]
    // three-pass plans only
    const LdePlan *inner = nullptr;          // (2^20, rate_bits, shift^A')
    u64 *t0 = nullptr, *t1 = nullptr;        // outer twiddle s_r^k1o (w_n^k1o)^q = t1[r][pbo][q >> 10] * t0[pbo][q & 1023]
    u64 last_use = 0;                        // LRU stamp (glp_ctx::lde_clock); plans other LdePlans point at are pinned
    int pins = 0;
    LdePlan() = default;
    LdePlan(const LdePlan &) = delete;
    LdePlan &operator=(const LdePlan &) = delete;
    ~LdePlan() { for (u64 *t : {pre, s_r, t0, t1}) if (t) (void)hipFree(t); }
};
constexpr size_t LDE_PLAN_CACHE_MAX = 48;    // distinct (log_n, rate_bits, shift) tables kept per context

int get_ntt_plan(glp_ctx *c, int lg, NttPlan **out);
int get_lde_plan(glp_ctx *c, int lg, int rate_bits, u64 shift, LdePlan **out);
void free_plans(glp_ctx *c);
// once per context, device bound: raises the dynamic-LDS limit of the k_strided32 instantiations (tiles above 64 KB)
int ntt_init_device(glp_ctx *c);

// values [ncols][n] natural  ->  coefficients [ncols][n] bit-reversed   (PolynomialValues::ifft)
int intt_values_to_coeffs(glp_ctx *c, const u64 *dev_values, u64 *dev_coeffs, u32 ncols, int lg);
// coefficients bit-reversed -> values natural (PolynomialCoeffs::fft), in place allowed (out == in)
int ntt_coeffs_to_values(glp_ctx *c, const u64 *dev_coeffs, u64 *dev_values, u32 ncols, int lg);
// coefficients [ncols][n] bit-reversed -> LDE [ncols][R][n] coset-major   (lde + coset_fft(shift))
int lde_coeffs(glp_ctx *c, const u64 *dev_coeffs, u64 *dev_lde, u32 ncols, int lg, int rate_bits, u64 shift);
// out[c][bitrev(p)] = in[c][p]  (layout conversion for accessors; not on the prove path)
int bitrev_copy(glp_ctx *c, const u64 *dev_in, u64 *dev_out, u32 ncols, int lg);
// coset-major [ncols][R][n] -> natural [ncols][N]  (accessor only)
int lde_to_natural(glp_ctx *c, const u64 *dev_lde, u64 *dev_out, u32 ncols, int lg, int rate_bits);
// The sub-coset shift * <W_M>, M = n << sub_bits, sub_bits <= rate_bits, read out of K coset-major members [ncols][R][n] that lie
// member_stride words apart: rows [row_begin, row_begin + num_rows) of columns [0, num_cols) of dev_lde, row i = q S + r being slot q
// of plane r * 2^(rate_bits - sub_bits).  row_major: out [K][num_rows][num_cols] (an LDS-tiled transpose), else [K][num_cols][num_rows].
int lde_sub_coset_rows(glp_ctx *c, const u64 *dev_lde, size_t member_stride, u32 K, u32 num_cols, int lg, int rate_bits, int sub_bits,
                       u64 row_begin, u64 num_rows, bool row_major, u64 *dev_out);
// natural order on such a coset [ncols][M] -> its S = 2^sub_bits planes [ncols][S][n]: index q S + r to plane r, slot q (sub_bits 1..4)
int coset_values_to_planes(glp_ctx *c, const u64 *dev_in, u64 *dev_out, size_t ncols, int lg, int sub_bits);

}  // namespace glp
