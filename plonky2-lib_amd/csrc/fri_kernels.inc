// fri_kernels.inc -- K7-K10: openings at zeta, the FRI batch polynomial, commit-phase leaves, folding, query gathers and the
// proof-of-work search.  Included by prover.hip; launched by the stage functions of prover_stages.inc, pow_search and pow_batch_launch.
// zt[p] = z^bitrev(p)  (extension), from z^(2^b), b < lg
// batch (zeta_b != nullptr, blockIdx.y = proof): the point comes from zeta_b[proof][2] and its squarings are made here
struct ZTArgs { u64 *zt; ext2 zp2[24]; u32 lg; const u64 *zeta_b; size_t zeta_stride; };
template <bool BATCH>
__global__ __launch_bounds__(256) void k_zeta_table(ZTArgs a) {
    const size_t n = (size_t)1 << a.lg;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const u32 k = bitrev32((u32)p, a.lg);
    ext2 acc = e_from(1);
    if constexpr (BATCH) {
        const u64 *z = a.zeta_b + (size_t)blockIdx.y * a.zeta_stride;
        ext2 sq = e_make(z[0], z[1]);
        for (u32 b = 0; b < a.lg; b++) { if ((k >> b) & 1) acc = e_mul(acc, sq); sq = e_sqr(sq); }
        a.zt += (size_t)blockIdx.y * 2 * n;
    } else {
        for (u32 b = 0; b < a.lg; b++) if ((k >> b) & 1) acc = e_mul(acc, a.zp2[b]);
    }
    a.zt[2 * p] = acc.a; a.zt[2 * p + 1] = acc.b;
}
// K7: partial sums of  sum_p coeffs[col][p] * zt[p]   grid = (OPEN_BLOCKS, ncols)
constexpr int OPEN_BLOCKS = 32;      // at most; open_blocks(n) picks fewer for short polynomials (the stride is gridDim.x)
inline u32 open_blocks(size_t n) { return (u32)std::max<size_t>(1, std::min<size_t>(OPEN_BLOCKS, n / 256)); }
// blockIdx.z = proof of a batch: coefficients / table / partial sums advance by the given strides (0 = shared by all proofs)
__global__ __launch_bounds__(256) void k_open_dot(const u64 *coeffs, const u64 *zt, u64 *partial, u32 lg, size_t coeffs_bstride,
                                                  size_t zt_bstride, size_t partial_bstride) {
    __shared__ u64 sa[256], sb[256];
    coeffs += (size_t)blockIdx.z * coeffs_bstride; zt += (size_t)blockIdx.z * zt_bstride; partial += (size_t)blockIdx.z * partial_bstride;
    const size_t n = (size_t)1 << lg;
    const u32 col = blockIdx.y, t = threadIdx.x;
    // n / (OPEN_BLOCKS * 256) <= 2^11 terms per thread, flushed every ACC_MAX_TERMS: carry-free limb accumulators
    // (one reduction per flush instead of a modular multiply-add per coefficient)
    u64 a = 0, b = 0;
    AccLimb xa, xb;
    acc2_zero(xa); acc2_zero(xb);
    u32 terms = 0;
    for (size_t p = (size_t)blockIdx.x * 256 + t; p < n; p += (size_t)gridDim.x * 256) {
        const u64 c = coeffs[(size_t)col * n + p];
        const u32 c0 = (u32)c & 0x3FFFFFu, c1 = (u32)(c >> 22) & 0x3FFFFFu, c2 = (u32)(c >> 44);
        acc2_fma(xa, c0, c1, c2, zt[2 * p]);
        acc2_fma(xb, c0, c1, c2, zt[2 * p + 1]);
        if (++terms == ACC_MAX_TERMS) {
            a = add(a, acc2_reduce(xa)); b = add(b, acc2_reduce(xb));
            acc2_zero(xa); acc2_zero(xb); terms = 0;
        }
    }
    a = add(a, acc2_reduce(xa)); b = add(b, acc2_reduce(xb));
    sa[t] = a; sb[t] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (t < s) { sa[t] = add(sa[t], sa[t + s]); sb[t] = add(sb[t], sb[t + s]); } __syncthreads(); }
    if (t == 0) { partial[2 * ((size_t)col * gridDim.x + blockIdx.x)] = sa[0]; partial[2 * ((size_t)col * gridDim.x + blockIdx.x) + 1] = sb[0]; }
}

// K8: values of the FRI batch polynomial on the coset plane 0 (x_q = g w_n^q):
//   F(x) = alpha^nch * (sum_j alpha^j f_j(x) - red0)/(x - zeta) + (sum_{j<nch} alpha^j Z_j(x) - red1)/(x - g zeta)
struct FVArgs {
    const u64 *lde[4]; u32 ncols[4];
    const u64 *apow;            // ext alpha^j, j < total columns
    u64 *out;                   // [2][n]
    ext2 red0, red1, zeta, zeta_next, shift_acc;   // shift_acc = alpha^nch
    u64 w_n, g;
    u32 lg, rb, nch;
    // many-proofs batch (blockIdx.y = proof): pp[proof][10] = red0, red1, zeta, zeta_next, shift_acc; strides per proof
    const u64 *pp;
    size_t lde_stride[4], apow_stride, out_stride;
};
__global__ __launch_bounds__(256) void k_final_values(FVArgs a) {
    const size_t n = (size_t)1 << a.lg, N = n << a.rb;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    if (a.pp) {
        const size_t pk = blockIdx.y;
        const u64 *v = a.pp + pk * 10;
        a.red0 = e_make(v[0], v[1]); a.red1 = e_make(v[2], v[3]); a.zeta = e_make(v[4], v[5]); a.zeta_next = e_make(v[6], v[7]);
        a.shift_acc = e_make(v[8], v[9]);
        _Pragma("unroll") for (int k = 0; k < 4; k++) a.lde[k] += pk * a.lde_stride[k];
        a.apow += pk * a.apow_stride; a.out += pk * a.out_stride;
    }
    // sum_j alpha^j f_j(x): the base-field value is cut into 22-bit limbs once and multiplied into carry-free
    // accumulators for the two extension coordinates (flushed every ACC_MAX_TERMS columns)
    ext2 acc0 = e_from(0), acc1 = e_from(0);
    AccLimb xa, xb;
    acc2_zero(xa); acc2_zero(xb);
    u32 j = 0, terms = 0;
    for (int k = 0; k < 4; k++) {
        const u64 *l = a.lde[k] + q;
        for (u32 c = 0; c < a.ncols[k]; c++, j++) {
            const u64 v = l[(size_t)c * N];
            const u32 v0 = (u32)v & 0x3FFFFFu, v1 = (u32)(v >> 22) & 0x3FFFFFu, v2 = (u32)(v >> 44);
            acc2_fma(xa, v0, v1, v2, a.apow[2 * j]);
            acc2_fma(xb, v0, v1, v2, a.apow[2 * j + 1]);
            if (++terms == ACC_MAX_TERMS) {
                acc0 = e_add(acc0, e_make(acc2_reduce(xa), acc2_reduce(xb)));
                acc2_zero(xa); acc2_zero(xb); terms = 0;
            }
            if (k == 2 && c < a.nch) {
                const ext2 ap1 = e_make(a.apow[2 * c], a.apow[2 * c + 1]);
                acc1 = e_add(acc1, e_scale(ap1, v));
            }
        }
    }
    acc0 = e_add(acc0, e_make(acc2_reduce(xa), acc2_reduce(xb)));
    const u64 x = mul(a.g, dpow(a.w_n, q));
    const ext2 d0 = e_inv(e_sub(e_from(x), a.zeta)), d1 = e_inv(e_sub(e_from(x), a.zeta_next));
    ext2 f = e_mul(e_mul(e_sub(acc0, a.red0), d0), a.shift_acc);
    f = e_add(f, e_mul(e_sub(acc1, a.red1), d1));
    a.out[q] = f.a; a.out[n + q] = f.b;
}

// The same for at most 128 points per proof (a batch of small proofs: blockIdx.y = proof, one workgroup per proof): 256 / n lanes share a point, each
// takes every (256 / n)-th column of the four oracles, an xor-butterfly adds the partial sums up, and lanes 0 and 1 of the group invert the two
// denominators side by side.  k_final_values walks ~250 columns and two extension inversions per lane with 8 lanes live: 105 us per 256 zkdsa proofs.
__global__ __launch_bounds__(256) void k_final_values_small(FVArgs a) {
    const u32 n = 1u << a.lg, lpp = 256u >> a.lg;            // lanes per point: 2 .. 64
    const size_t N = (size_t)n << a.rb;
    const u32 q = threadIdx.x / lpp, t = threadIdx.x % lpp;
    if (a.pp) {
        const size_t pk = blockIdx.y;
        const u64 *v = a.pp + pk * 10;
        a.red0 = e_make(v[0], v[1]); a.red1 = e_make(v[2], v[3]); a.zeta = e_make(v[4], v[5]); a.zeta_next = e_make(v[6], v[7]);
        a.shift_acc = e_make(v[8], v[9]);
        _Pragma("unroll") for (int k = 0; k < 4; k++) a.lde[k] += pk * a.lde_stride[k];
        a.apow += pk * a.apow_stride; a.out += pk * a.out_stride;
    }
    ext2 acc0 = e_from(0), acc1 = e_from(0);
    AccLimb xa, xb;
    acc2_zero(xa); acc2_zero(xb);
    u32 base = 0;
    for (int k = 0; k < 4; k++) {
        const u64 *l = a.lde[k] + q;
        for (u32 c = t; c < a.ncols[k]; c += lpp) {          // at most ACC_MAX_TERMS terms per lane (final_values_small_fits): no flush
            const u32 j = base + c;
            const u64 v = l[(size_t)c * N];
            const u32 v0 = (u32)v & 0x3FFFFFu, v1 = (u32)(v >> 22) & 0x3FFFFFu, v2 = (u32)(v >> 44);
            acc2_fma(xa, v0, v1, v2, a.apow[2 * j]);
            acc2_fma(xb, v0, v1, v2, a.apow[2 * j + 1]);
            if (k == 2 && c < a.nch) acc1 = e_add(acc1, e_scale(e_make(a.apow[2 * c], a.apow[2 * c + 1]), v));
        }
        base += a.ncols[k];
    }
    acc0 = e_make(acc2_reduce(xa), acc2_reduce(xb));
    for (u32 m = lpp >> 1; m >= 1; m >>= 1) {                // lpp <= 64 here (n >= 4): the group lies inside one wavefront
        acc0 = e_add(acc0, e_make(pos::shfl_xor64(acc0.a, (int)m), pos::shfl_xor64(acc0.b, (int)m)));
        acc1 = e_add(acc1, e_make(pos::shfl_xor64(acc1.a, (int)m), pos::shfl_xor64(acc1.b, (int)m)));
    }
    const u64 x = mul(a.g, dpow(a.w_n, q));
    const ext2 dmine = e_inv(e_sub(e_from(x), t == 1 ? a.zeta_next : a.zeta));       // lane 0: 1 / (x - zeta), lane 1: 1 / (x - zeta_next)
    const int lane1 = (int)((threadIdx.x & 63u) - t + 1);
    const ext2 d1 = e_make(pos::shfl64(dmine.a, lane1), pos::shfl64(dmine.b, lane1));
    if (t == 0) {
        ext2 f = e_mul(e_mul(e_sub(acc0, a.red0), dmine), a.shift_acc);
        f = e_add(f, e_mul(e_sub(acc1, a.red1), d1));
        a.out[q] = f.a; a.out[n + q] = f.b;
    }
}
// K8 for any FRI instance (fri_openings.inc), K proofs of it in lock step (blockIdx.y = proof; glp_fri_begin makes K = 1): up to
// GLP_FRI_MAX_POINTS opening points, each naming its own list of columns:
//   F <- alpha^(len_b) F + (sum_j alpha^j p_{b,j}(x) - red_b) / (x - z_b)     for b = 0 .. npoints - 1, F = 0 before the first
// One pass over the union of the named columns: prog[e] is one column (its plane 0) and, per point, where that column's alpha
// power sits in the table (FC_ABSENT: the point does not name it), so a column several points name is loaded once.  The column
// program is shared by all proofs; a column's plane advances by `stride` words per proof (0: an oracle all proofs share, else
// (ncols + salt) N of its oracle).  Alpha, red_b, z_b and shift_b = alpha^(len_b) are each proof's own and come from device tables
// that k_fri_table fills: apow [K][nopen] ext, pp [K][FCM_PP_WORDS] = red[NP], z[NP], shift[NP] (ext each).  Every table address
// is made of kernel arguments and blockIdx.y only, so the reads stay scalar.
constexpr u32 FC_ABSENT = 0xFFFFFFFFu;
struct FCColM { const u64 *plane; size_t stride; u32 ap[GLP_FRI_MAX_POINTS]; };
constexpr u32 FCM_PP_WORDS = 6 * GLP_FRI_MAX_POINTS;
struct FCMArgs {
    const FCColM *prog; u32 nprog, npoints;
    const u64 *apow;            // [K][nopen] ext alpha powers of proof k, indexed by FCColM::ap
    const u64 *pp;              // [K][FCM_PP_WORDS]
    u64 *out;                   // [K][2][n]
    size_t nopen;
    u64 w_n, g;
    u32 lg;
};
// pp of one proof: part 0 = red_b, 1 = z_b, 2 = shift_b
__device__ __forceinline__ ext2 fcm_pp(const u64 *pp, int part, int b) {
    return e_make(pp[2 * (part * GLP_FRI_MAX_POINTS + b)], pp[2 * (part * GLP_FRI_MAX_POINTS + b) + 1]);
}
// 2^8 points per proof and more: one lane per point.  The program and the powers are read uniformly (scalar loads, uniform branches),
// as coset_table is; one carry-free accumulator pair per opening point, all flushed every ACC_MAX_TERMS columns.  Columns are loaded
// four at a time to keep four loads in flight.
__global__ __launch_bounds__(256) void k_fri_combine_many(FCMArgs a) {
    constexpr int NP = GLP_FRI_MAX_POINTS;
    const size_t n = (size_t)1 << a.lg, pk = blockIdx.y;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const u64 *apow = a.apow + pk * 2 * a.nopen, *pp = a.pp + pk * FCM_PP_WORDS;
    ext2 sum[NP];
    AccLimb xa[NP], xb[NP];
#pragma unroll
    for (int b = 0; b < NP; b++) { sum[b] = e_from(0); acc2_zero(xa[b]); acc2_zero(xb[b]); }
    u32 terms = 0;
    for (u32 e0 = 0; e0 < a.nprog; e0 += 4) {
        u64 v[4];
#pragma unroll
        for (u32 i = 0; i < 4; i++) v[i] = e0 + i < a.nprog ? a.prog[e0 + i].plane[pk * a.prog[e0 + i].stride + q] : 0;
#pragma unroll
        for (u32 i = 0; i < 4; i++) {
            if (e0 + i >= a.nprog) break;
            const u32 v0 = (u32)v[i] & 0x3FFFFFu, v1 = (u32)(v[i] >> 22) & 0x3FFFFFu, v2 = (u32)(v[i] >> 44);
#pragma unroll
            for (int b = 0; b < NP; b++) {
                const u32 j = a.prog[e0 + i].ap[b];
                if (j != FC_ABSENT) { acc2_fma(xa[b], v0, v1, v2, apow[2 * (size_t)j]); acc2_fma(xb[b], v0, v1, v2, apow[2 * (size_t)j + 1]); }
            }
        }
        if ((terms += 4) == ACC_MAX_TERMS) {
#pragma unroll
            for (int b = 0; b < NP; b++) {
                sum[b] = e_add(sum[b], e_make(acc2_reduce(xa[b]), acc2_reduce(xb[b])));
                acc2_zero(xa[b]); acc2_zero(xb[b]);
            }
            terms = 0;
        }
    }
    const ext2 x = e_from(mul(a.g, dpow(a.w_n, q)));
    ext2 f = e_from(0);
#pragma unroll
    for (int b = 0; b < NP; b++) {
        if ((u32)b >= a.npoints) break;
        const ext2 s = e_add(sum[b], e_make(acc2_reduce(xa[b]), acc2_reduce(xb[b])));
        f = e_add(e_mul(f, fcm_pp(pp, 2, b)), e_mul(e_sub(s, fcm_pp(pp, 0, b)), e_inv(e_sub(x, fcm_pp(pp, 1, b)))));
    }
    u64 *out = a.out + pk * 2 * n;
    out[q] = f.a; out[n + q] = f.b;
}
// 4 .. 128 points per proof (where batches of small proofs live): one workgroup per proof, lpp = 256 / n lanes share a point.  Lane t
// of a point takes the program entries t, t + lpp, ..; an xor-butterfly inside the group (lpp <= 64: one wavefront) adds the partial
// sums of every point up, lane b % lpp of the group inverts x - z_b, and lane 0 finishes.  A lane's slice of the program is its own,
// so the program and the powers are vector loads here; the per-proof table stays scalar.  Unlike k_final_values_small a lane
// flushes its carry-free accumulators every ACC_MAX_TERMS entries: an instance may name any number of columns.
__global__ __launch_bounds__(256) void k_fri_combine_many_small(FCMArgs a) {
    constexpr int NP = GLP_FRI_MAX_POINTS;
    const u32 n = 1u << a.lg, lpp = 256u >> a.lg;            // lanes per point: 2 .. 64
    const size_t pk = blockIdx.y;
    const u32 q = threadIdx.x / lpp, t = threadIdx.x % lpp;
    const u64 *apow = a.apow + pk * 2 * a.nopen, *pp = a.pp + pk * FCM_PP_WORDS;
    ext2 sum[NP];
    AccLimb xa[NP], xb[NP];
#pragma unroll
    for (int b = 0; b < NP; b++) { sum[b] = e_from(0); acc2_zero(xa[b]); acc2_zero(xb[b]); }
    u32 terms = 0;
    for (u32 e = t; e < a.nprog; e += lpp) {
        const FCColM col = a.prog[e];
        const u64 v = col.plane[pk * col.stride + q];
        const u32 v0 = (u32)v & 0x3FFFFFu, v1 = (u32)(v >> 22) & 0x3FFFFFu, v2 = (u32)(v >> 44);
#pragma unroll
        for (int b = 0; b < NP; b++) {
            const u32 j = col.ap[b];
            if (j != FC_ABSENT) { acc2_fma(xa[b], v0, v1, v2, apow[2 * (size_t)j]); acc2_fma(xb[b], v0, v1, v2, apow[2 * (size_t)j + 1]); }
        }
        if (++terms == ACC_MAX_TERMS) {
#pragma unroll
            for (int b = 0; b < NP; b++) {
                sum[b] = e_add(sum[b], e_make(acc2_reduce(xa[b]), acc2_reduce(xb[b])));
                acc2_zero(xa[b]); acc2_zero(xb[b]);
            }
            terms = 0;
        }
    }
#pragma unroll
    for (int b = 0; b < NP; b++) {
        sum[b] = e_add(sum[b], e_make(acc2_reduce(xa[b]), acc2_reduce(xb[b])));
        for (u32 m = lpp >> 1; m >= 1; m >>= 1)
            sum[b] = e_add(sum[b], e_make(pos::shfl_xor64(sum[b].a, (int)m), pos::shfl_xor64(sum[b].b, (int)m)));
    }
    // 1 / (x - z_b) on lane b % lpp, slot b / lpp (two slots only when two lanes share a point: n = 128)
    const ext2 x = e_from(mul(a.g, dpow(a.w_n, q)));
    ext2 dinv[2];
#pragma unroll
    for (u32 s = 0; s < 2; s++) {
        const u32 b = t + s * lpp;
        dinv[s] = b < a.npoints ? e_inv(e_sub(x, e_make(pp[2 * (NP + b)], pp[2 * (NP + b) + 1]))) : e_from(0);
    }
    const int lane0 = (int)((threadIdx.x & 63u) - t);
    ext2 f = e_from(0);
#pragma unroll
    for (int b = 0; b < NP; b++) {
        if ((u32)b >= a.npoints) break;
        const ext2 mine = (u32)b / lpp ? dinv[1] : dinv[0];
        const int src = lane0 + (int)((u32)b % lpp);
        const ext2 d = e_make(pos::shfl64(mine.a, src), pos::shfl64(mine.b, src));
        f = e_add(e_mul(f, fcm_pp(pp, 2, b)), e_mul(e_sub(sum[b], fcm_pp(pp, 0, b)), d));
    }
    if (t == 0) {
        u64 *out = a.out + pk * 2 * n;
        out[q] = f.a; out[n + q] = f.b;
    }
}
// the openings of all proofs from k_open_dot's partial sums (open_batch_finish on the device): partial [count][nob] ext -> open [count] ext
__global__ __launch_bounds__(256) void k_fri_open_finish(const u64 *partial, u64 *open, size_t count, u32 nob) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    u64 sa = 0, sb = 0;
    for (u32 k = 0; k < nob; k++) { sa = add(sa, partial[2 * (i * nob + k)]); sb = add(sb, partial[2 * (i * nob + k) + 1]); }
    open[2 * i] = sa; open[2 * i + 1] = sb;
}
// the per-proof tables of k_fri_combine_many*: workgroup (b, k) walks the
// len_b polynomials of point b for proof k, 256 lanes a chunk each from alpha_k^(chunk start): apow[k][first_b + j] = alpha_k^j,
// red_b = sum_j alpha_k^j open[k][first_b + j], shift_b = alpha_k^(len_b), z_b copied next to them.
struct FTArgs {
    const u64 *alpha;           // [K] ext
    const u64 *open;            // [K][nopen] ext
    const u64 *z;               // [K][npoints] ext
    u64 *apow, *pp;             // [K][nopen] ext, [K][FCM_PP_WORDS]
    size_t nopen;
    u32 first[GLP_FRI_MAX_POINTS], len[GLP_FRI_MAX_POINTS];
};
__global__ __launch_bounds__(256) void k_fri_table(FTArgs a) {
    constexpr int NP = GLP_FRI_MAX_POINTS;
    __shared__ u64 sa[256], sb[256];
    const u32 b = blockIdx.x, t = threadIdx.x, npoints = gridDim.x;
    const size_t pk = blockIdx.y;
    const ext2 alpha = e_make(a.alpha[2 * pk], a.alpha[2 * pk + 1]);
    const u32 first = a.first[b], len = a.len[b], chunk = (len + 255) / 256;
    const u64 *open = a.open + 2 * (pk * a.nopen + first);
    u64 *apow = a.apow + 2 * (pk * a.nopen + first);
    const u32 j0 = t * chunk < len ? t * chunk : len, j1 = j0 + chunk < len ? j0 + chunk : len;
    ext2 x = e_pow(alpha, j0), red = e_from(0);
    for (u32 j = j0; j < j1; j++) {
        apow[2 * j] = x.a; apow[2 * j + 1] = x.b;
        red = e_add(red, e_mul(x, e_make(open[2 * j], open[2 * j + 1])));
        x = e_mul(x, alpha);
    }
    sa[t] = red.a; sb[t] = red.b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if ((int)t < s) { sa[t] = add(sa[t], sa[t + s]); sb[t] = add(sb[t], sb[t + s]); } __syncthreads(); }
    if (t == 0) {
        u64 *pp = a.pp + pk * FCM_PP_WORDS;
        const ext2 shift = e_pow(alpha, len);
        pp[2 * b] = sa[0]; pp[2 * b + 1] = sb[0];
        pp[2 * (NP + b)] = a.z[2 * (pk * npoints + b)]; pp[2 * (NP + b) + 1] = a.z[2 * (pk * npoints + b) + 1];
        pp[2 * (2 * NP + b)] = shift.a; pp[2 * (2 * NP + b) + 1] = shift.b;
    }
}
// data[c][p] *= base^bitrev(p)
__global__ __launch_bounds__(256) void k_scale_bitrev_pow(u64 *data, u64 base, u32 lg) {
    const size_t n = (size_t)1 << lg;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const u64 f = dpow(base, bitrev32((u32)p, lg));
    data[(size_t)blockIdx.y * n + p] = mul(data[(size_t)blockIdx.y * n + p], f);
}

// K9a: FRI commit-phase leaves.  vals = coset-major LDE [2][R][ncur] of the current polynomial (L = R*ncur
// points); leaf m = the `arity` extension values at natural indices bitrev_L(m*arity + t).  Lane = M' = bitrev(m).
__global__ __launch_bounds__(256, 4) void k_fri_leaf_hash(const u64 *vals, u64 *digests, u32 lgL, u32 rb, u32 ab, size_t vals_bstride,
                                                       size_t dig_bstride) {
    vals += (size_t)blockIdx.y * vals_bstride; digests += (size_t)blockIdx.y * dig_bstride;     // blockIdx.y = proof of a batch
    const size_t L = (size_t)1 << lgL, ncur = L >> rb, nleaves = L >> ab;
    const size_t Mp = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (Mp >= nleaves) return;
    const size_t m = bitrev32((u32)Mp, lgL - ab);
    const u32 arity = 1u << ab;
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = 0;
    const u64 *re = vals, *im = vals + L;
    u32 fill = 0;
    for (u32 t = 0; t < arity; t++) {
        const size_t i = (size_t)bitrev32(t, ab) * nleaves + Mp;
        const size_t pos = (i & (((size_t)1 << rb) - 1)) * ncur + (i >> rb);
        s[fill++] = re[pos];
        s[fill++] = im[pos];
        if (fill == 8) { if (2 * arity > 4) pos::permute(s); fill = 0; }
    }
    if (fill && 2 * arity > 4) pos::permute(s);
    ulonglong2 d0, d1;
    d0.x = s[0]; d0.y = s[1]; d1.x = s[2]; d1.y = s[3];
    reinterpret_cast<ulonglong2 *>(digests + 4 * m)[0] = d0;
    reinterpret_cast<ulonglong2 *>(digests + 4 * m)[1] = d1;
}
// K9a, latency form for small layers: one leaf per 16-lane group, sponge state on 12 lanes.
__global__ __launch_bounds__(256) void k_fri_leaf_hash_coop(const u64 *vals, u64 *digests, u32 lgL, u32 rb, u32 ab, size_t vals_bstride,
                                                            size_t dig_bstride) {
    vals += (size_t)blockIdx.y * vals_bstride; digests += (size_t)blockIdx.y * dig_bstride;
    const size_t L = (size_t)1 << lgL, ncur = L >> rb, nleaves = L >> ab;
    const int tid = threadIdx.x, l = tid & 15, lane = tid & 63, group_base = lane & ~15;
    const size_t Mp0 = (size_t)blockIdx.x * 16 + (tid >> 4);
    const bool live = Mp0 < nleaves;
    const size_t Mp = live ? Mp0 : 0;
    const size_t m = bitrev32((u32)Mp, lgL - ab);
    const u32 len = 2u << ab;                       // base-field elements per leaf
    u64 x = 0;
    for (u32 c = 0; c < len; c += 8) {
        if (l < 8 && c + l < len) {
            const u32 e = c + l, t = e >> 1;
            const size_t i = (size_t)bitrev32(t, ab) * nleaves + Mp;
            const size_t pos = (i & (((size_t)1 << rb) - 1)) * ncur + (i >> rb);
            x = vals[(e & 1 ? L : 0) + pos];
        }
        if (len > 4) x = pos::permute_coop(x, l, group_base);
    }
    if (live && l < 4) digests[4 * m + l] = x;
}
// K9a with KeccakHash<25>: hash_or_noop of the leaf's 2^(ab+1) elements (arity 2 already exceeds the 3 elements that are copied)
// one leaf per quad of lanes (pos::permute_quad): layers of 2^12..2^15 leaves, as for the initial trees (merkle.hip)
__global__ __launch_bounds__(256) void k_fri_leaf_hash_quad(const u64 *vals, u64 *digests, u32 lgL, u32 rb, u32 ab, size_t vals_bstride,
                                                            size_t dig_bstride) {
    vals += (size_t)blockIdx.y * vals_bstride; digests += (size_t)blockIdx.y * dig_bstride;
    const size_t L = (size_t)1 << lgL, ncur = L >> rb, nleaves = L >> ab;
    const int tid = threadIdx.x, q = tid & 3;
    const size_t Mp0 = (size_t)blockIdx.x * 64 + (tid >> 2);
    const bool live = Mp0 < nleaves;
    const size_t Mp = live ? Mp0 : 0;
    const size_t m = bitrev32((u32)Mp, lgL - ab);
    const u32 len = 2u << ab;                       // base-field elements per leaf
    u64 x[3] = {0, 0, 0};
    for (u32 c = 0; c < len; c += 8) {
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const u32 e8 = 3 * q + s, e = c + e8;
            if (e8 < 8 && e < len) {
                const u32 t = e >> 1;
                const size_t i = (size_t)bitrev32(t, ab) * nleaves + Mp;
                const size_t pos = (i & (((size_t)1 << rb) - 1)) * ncur + (i >> rb);
                x[s] = vals[(e & 1 ? L : 0) + pos];
            }
        }
        if (len > 4) pos::permute_quad(x, q);
    }
    if (live) {
        if (q == 0) { digests[4 * m] = x[0]; digests[4 * m + 1] = x[1]; digests[4 * m + 2] = x[2]; }
        if (q == 1) digests[4 * m + 3] = x[0];
    }
}
__global__ __launch_bounds__(256) void k_fri_leaf_hash_keccak(const u64 *vals, u64 *digests, u32 lgL, u32 rb, u32 ab, size_t vals_bstride,
                                                              size_t dig_bstride) {
    vals += (size_t)blockIdx.y * vals_bstride; digests += (size_t)blockIdx.y * dig_bstride;
    const size_t L = (size_t)1 << lgL, ncur = L >> rb, nleaves = L >> ab;
    const size_t Mp = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (Mp >= nleaves) return;
    const size_t m = bitrev32((u32)Mp, lgL - ab);
    const u32 arity = 1u << ab;
    kec::Sponge s;
    kec::sponge_init(s);
    for (u32 t = 0; t < arity; t++) {
        const size_t i = (size_t)bitrev32(t, ab) * nleaves + Mp;
        const size_t pos = (i & (((size_t)1 << rb) - 1)) * ncur + (i >> rb);
        kec::sponge_absorb(s, vals[pos]);
        kec::sponge_absorb(s, vals[L + pos]);
    }
    kec::sponge_finish(s);
    u64 d[4];
    kec::sponge_digest25(s, d);
    ulonglong2 d0, d1;
    d0.x = d[0]; d0.y = d[1]; d1.x = d[2]; d1.y = d[3];
    reinterpret_cast<ulonglong2 *>(digests + 4 * m)[0] = d0;
    reinterpret_cast<ulonglong2 *>(digests + 4 * m)[1] = d1;
}
// K9b: fold coefficients (bit-reversed layout): new[p'] = sum_t beta^t old[bitrev(t) * nnew + p']
// batch (beta_b != nullptr, blockIdx.y = proof): beta from beta_b[proof][2]; coefficient arrays [proof][2][n]
__global__ __launch_bounds__(256) void k_fri_fold(const u64 *oldc, u64 *newc, ext2 beta, u32 lg_old, u32 ab, const u64 *beta_b) {
    const size_t nold = (size_t)1 << lg_old, nnew = nold >> ab;
    if (beta_b) {
        beta = e_make(beta_b[2 * blockIdx.y], beta_b[2 * blockIdx.y + 1]);
        oldc += (size_t)blockIdx.y * 2 * nold; newc += (size_t)blockIdx.y * 2 * nnew;
    }
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nnew) return;
    ext2 acc = e_from(0);
    for (u32 t = 1u << ab; t-- > 0;) {
        const size_t o = (size_t)bitrev32(t, ab) * nnew + p;
        acc = e_add(e_mul(acc, beta), e_make(oldc[o], oldc[nold + o]));
    }
    newc[p] = acc.a; newc[nnew + p] = acc.b;
}
// leaf evals for the query phase: out[k][2*t..] = the arity values of leaf idx[k]
__global__ void k_fri_gather_leaf(const u64 *vals, u32 lgL, u32 rb, u32 ab, const u64 *idx, u32 idx_shift, u32 count, u64 *out,
                                  size_t out_stride, size_t vals_bstride, size_t out_bstride) {
    vals += (size_t)blockIdx.y * vals_bstride; idx += (size_t)blockIdx.y * count; out += (size_t)blockIdx.y * out_bstride;
    const size_t L = (size_t)1 << lgL, ncur = L >> rb, nleaves = L >> ab;
    const u32 arity = 1u << ab;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (size_t)count * arity) return;
    const u32 k = (u32)(gid / arity), t = (u32)(gid % arity);
    const size_t m = idx[k] >> idx_shift;
    const size_t Mp = bitrev32((u32)m, lgL - ab);
    const size_t i = (size_t)bitrev32(t, ab) * nleaves + Mp;
    const size_t pos = (i & (((size_t)1 << rb) - 1)) * ncur + (i >> rb);
    out[(size_t)k * out_stride + 2 * t] = vals[pos];
    out[(size_t)k * out_stride + 2 * t + 1] = vals[L + pos];
}

// K10: proof-of-work grinding; smallest candidate in [base, base + count) whose response has `bits` leading zeros
struct PowArgs { u64 st[12]; u32 pos, bits; u64 base; unsigned long long *best; };
template <int HASHER>
__global__ __launch_bounds__(256) void k_pow(PowArgs a) {
    const u64 cand = a.base + (u64)blockIdx.x * 256 + threadIdx.x;
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = a.st[i];
#pragma unroll
    for (int i = 0; i < 8; i++) if ((u32)i == a.pos) s[i] = cand;        // cand < 2^40 + 2^20 < p: a canonical word, as permute() takes
    if constexpr (HASHER == GLP_HASH_KECCAK25) kec::permute(s); else pos::permute(s);
    if (a.bits == 0 || (s[7] >> (64 - a.bits)) == 0) atomicMin(a.best, (unsigned long long)cand);
}

// K10 for a batch of K proofs, each with its own sponge state st_b[proof][12] and input position pos_b[proof].  Workgroups
// are persistent: a workgroup takes the next 256 candidates of a proof from that proof's counter (next[proof], handed out
// in increasing order), tests them, and records the smallest hit in best[proof]; it leaves a proof once a hit below its next
// chunk is known and moves on to the next unfinished proof, so the long tail of one unlucky search is shared by the whole
// GPU instead of idling it.  Every chunk below the final best[proof] was handed out and completed before the kernel ends,
// hence the result is the smallest witness regardless of scheduling.  Termination: a proof is finished once best <= next
// (a witness exists below 2^40 with overwhelming probability; the hand-out stops there in any case), and a workgroup exits
// after one full pass over the proofs finds none unfinished.
template <int HASHER>
__global__ __launch_bounds__(256) void k_pow_batch(const u64 *st_b, const u32 *pos_b, u32 bits, unsigned long long *best,
                                                   unsigned long long *next, u32 K) {
    __shared__ unsigned long long sh_base;
    u32 pk = blockIdx.x % K, idle = 0;
    while (idle < K) {
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long b = ~0ull;
            const unsigned long long cur = *(volatile unsigned long long *)(best + pk);
            if (*(volatile unsigned long long *)(next + pk) < cur) {
                b = atomicAdd(next + pk, 256ull);
                if (b >= cur || b >= (1ull << 40)) b = ~0ull;       // nothing below the known witness (or the cap) is left
            }
            sh_base = b;
        }
        __syncthreads();
        const unsigned long long base = sh_base;
        if (base == ~0ull) { pk = pk + 1 == K ? 0 : pk + 1; idle++; continue; }
        idle = 0;
        u64 s[12];
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = st_b[(size_t)pk * 12 + i];
        const u32 pos = pos_b[pk];
        const u64 cand = base + threadIdx.x;
        for (u32 i = 0; i < 8; i++) if (i == pos) s[i] = cand;      // cand < 2^40 + 256 < p: a canonical word, as permute() takes
        if constexpr (HASHER == GLP_HASH_KECCAK25) kec::permute(s); else pos::permute(s);
        if (bits == 0 || (s[7] >> (64 - bits)) == 0) atomicMin(best + pk, (unsigned long long)cand);
    }
}

// The same search for PoseidonGoldilocksConfig, restructured (round 3):
//  * round 0 and the last linear layer collapse per candidate (poseidon.h permute_tail7; k_pow_prepare computes the twelve
//    per-proof constants once);
//  * work is dealt round robin over the UNFINISHED proofs: a workgroup draws a ticket (one global counter) and takes its next
//    chunk of 256 candidates from the (ticket mod U)-th of the U proofs still open -- every thread looks at the proofs
//    t, t + 256, ..., a wavefront scan ranks them.  What a finished search wastes is the chunks of that proof still in flight
//    beyond the witness, so the chunks in flight must be spread evenly: workgroups that stay on "their" proof and move to the
//    next open one when it finishes (the first form of this kernel) pile up behind runs of finished proofs, and 20 % of the
//    candidates hashed lay beyond a witness (profiles/r03_sq_pow_batch2.txt); dealt evenly it is the ~9 % that 2^18 lanes in
//    flight over U open proofs cost in any order;
//  * workgroups are NOT persistent: each takes at most `chunks` chunks of 256 candidates and leaves, so the launch drains as the
//    work runs out and the small latency-bound kernels of another sub-batch (own context and stream) find free slots between
//    them.  The grid is sized for several times the expected work; the last `tail_from`.. workgroups stay until every proof is
//    finished, so the search completes however unlucky it is.
// k_b[K][12] per-proof constants, then one word: the ticket counter (k_pow_prepare zeroes it)
__global__ __launch_bounds__(64) void k_pow_prepare(const u64 *st_b, const u32 *pos_b, u64 *k_b, u32 K) {
    const u32 k = blockIdx.x * 64 + threadIdx.x;
    if (k == 0) k_b[(size_t)K * 12] = 0;
    if (k >= K) return;
    u64 st[12], out[12];
    for (int i = 0; i < 12; i++) st[i] = st_b[(size_t)k * 12 + i];
    pos::pow_round0_consts(st, pos_b[k], out);
    for (int i = 0; i < 12; i++) k_b[(size_t)k * 12 + i] = out[i];
}
__device__ __forceinline__ bool pow_open(const unsigned long long *best, const unsigned long long *next, u32 q) {
    const unsigned long long b = *(volatile const unsigned long long *)(best + q), nx = *(volatile const unsigned long long *)(next + q);
    return nx < b && nx < (1ull << 40);
}
__global__ __launch_bounds__(256, 4) void k_pow_batch2(u64 *k_b, const u32 *pos_b, u32 bits, unsigned long long *best,
                                                        unsigned long long *next, u32 K, u32 chunks, u32 tail_from) {
    __shared__ unsigned long long sh_base, sh_ticket;
    __shared__ u32 sh_pick, sh_wsum[4];
    const u32 t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool persistent = blockIdx.x >= tail_from;
    unsigned long long *ticket = (unsigned long long *)(k_b + (size_t)K * 12);
    for (u32 done = 0; persistent || done < chunks; done++) {
        // rank the open proofs: thread t owns proofs t, t + 256, ...
        u32 mine = 0;
        for (u32 q = t; q < K; q += 256) mine += pow_open(best, next, q) ? 1u : 0u;
        u32 incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u32 v = (u32)__shfl_up((int)incl, d, 64); if ((int)lane >= d) incl += v; }
        __syncthreads();                                            // the previous round's readers of sh_* are done
        if (lane == 63) sh_wsum[wave] = incl;
        if (t == 0) { sh_ticket = atomicAdd(ticket, 1ull); sh_pick = ~0u; }
        __syncthreads();
        u32 before = 0, open = 0;
#pragma unroll
        for (u32 w = 0; w < 4; w++) { if (w < wave) before += sh_wsum[w]; open += sh_wsum[w]; }
        if (open == 0) return;                                      // every proof has its witness (or its search is exhausted)
        const u32 want = (u32)sh_ticket % open, first = before + incl - mine;
        if (want >= first && want < first + mine) {                 // exactly one thread; proofs may have closed since the count
            u32 r = want - first;
            for (u32 q = t; q < K; q += 256)
                if (pow_open(best, next, q)) { if (r == 0) { sh_pick = q; break; } r--; }
        }
        __syncthreads();
        const u32 pk = sh_pick;
        if (pk == ~0u) continue;                                    // it closed in between: draw again
        if (t == 0) {
            unsigned long long b = atomicAdd(next + pk, 256ull);
            if (b >= *(volatile unsigned long long *)(best + pk) || b >= (1ull << 40)) b = ~0ull;       // taken by someone else in the meantime
            sh_base = b;
        }
        __syncthreads();
        const unsigned long long base = sh_base;
        if (base == ~0ull) continue;
        const u32 pos_ = pos_b[pk];
        const u64 cand = base + t;
        // a plain add, no reduction: cand < 2^40 + 256 and pos_ < 8, and RC[0..7] < 2^64 - 2^41 (static_assert at pblk::RC_CE,
        // poseidon.h), so the sum stays a u64; it may pass p, which sbox7_nc takes
        const u64 sp = pos::sbox7_nc(cand + pos::RC[pos_]);
        u64 s[12];
#pragma unroll
        for (int r = 0; r < 12; r++) s[r] = add_cnc(k_b[(size_t)pk * 12 + r], mul_small_nc(sp, pos::mds_entry(r, (int)pos_)));
        // a witness below this whole chunk may turn up while it is being hashed: then the rest of the permutation is wasted work
        const unsigned long long *bp = best + pk;
        const u64 e7 = pos::permute_tail7(s, [bp, base] { return *(volatile const unsigned long long *)bp < base; });
        if (bits == 0 || (e7 >> (64 - bits)) == 0) atomicMin(best + pk, (unsigned long long)cand);
    }
}
