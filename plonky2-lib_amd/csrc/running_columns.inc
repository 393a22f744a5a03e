// running_columns.inc -- glp_running_columns: the helper columns h_t = num_t / den_t and the running column Z of a caller-defined
// lookup, logUp, cross-table or grand-product argument (include/glp.h, "caller-defined running arguments at the commitment seam").
// Included by prover.hip behind trace_program.inc, whose output is this file's input.
//
// Element (proof k, argument a, term t, row i) of nums and dens sits at k * in_stride + (a T + t) n + i; out is [K][A][T + 1][n], the
// T helper columns of an argument and then its Z.  With op = + (GLP_RUN_SUM, identity 0) or * (GLP_RUN_PRODUCT, identity 1):
//     c[i] = op_t h_t[i]          Z[0] = identity, Z[i + 1] = Z[i] op c[i]          total = Z[n - 1] op c[n - 1]
//
// run_row: one lane owns one row of one argument and inverts its T denominators with ONE Fermat inversion (Montgomery's trick, the
// walk of k_pp_rows): pass 1 writes the prefix products of the denominators into the helper columns, pass 2 walks back down with
// 1 / PD_t = (1 / PD_{t+1}) den_{t+1} and replaces them by h_t.  Lanes are consecutive rows, so every load and store is coalesced along
// i.  A zero denominator must not poison its neighbours silently: it enters the chain as 1 (in both passes) and its flat index
// ((k A + a) T + t) n + i goes into res[0] by a 64-bit atomicMin, so the host names the first one in (k, a, t, i) order.
// The scan is the three-step scheme of pp_kernels.inc K5b-d and no workgroup ever waits on another:
//   k_run_terms      run_row, c[i] into the Z column for now, and the block's total of 256 c[i] (K5b, fused: the values are at hand)
//   k_run_scan_tot   exclusive scan of the block totals, one workgroup per (proof, argument); the grand total goes to res (K5c)
//   k_run_apply      Z[i] = prefix(block) op the in-block exclusive scan (K5d)
//   k_run_small      n <= 256: the whole column is one workgroup's, all of it in one launch, blockIdx = (argument, proof) -- K small
//                    proofs in lock step are the seam's main customer (k_pp_rows_small)
// A device input word is reduced mod p once as it is loaded.
struct RunArgs {
    const u64 *nums, *dens;               // nums == nullptr: every numerator is 1
    u64 *out;                             // [K][A][T + 1][n]
    u64 *tot;                             // [K][A][nblocks]: block totals, then their exclusive scan
    unsigned long long *res;              // res[0]: the smallest flat index of a zero denominator, ~0 if none; res[1 + k A + a]: totals
    size_t in_stride;
    u32 lg, A, T, nblocks;
};
template <int KIND> __device__ __forceinline__ u64 run_op(u64 a, u64 b) { return KIND == (int)GLP_RUN_SUM ? add(a, b) : mul(a, b); }
template <int KIND> __device__ __forceinline__ u64 run_identity() { return KIND == (int)GLP_RUN_SUM ? 0 : 1; }

// the T helper values of row i of argument `arg` of proof k, written; returns c[i]
template <int KIND>
__device__ __forceinline__ u64 run_row(const RunArgs &a, size_t k, u32 arg, size_t i) {
    const size_t n = (size_t)1 << a.lg;
    const u32 T = a.T;
    const size_t in0 = k * a.in_stride + (size_t)arg * T * n + i;
    const u64 *dn = a.dens + in0, *nm = a.nums ? a.nums + in0 : nullptr;
    u64 *h = a.out + (k * a.A + arg) * (size_t)(T + 1) * n + i;
    u64 pd = 1;
    for (u32 t = 0; t < T; t++) {
        u64 d = canon(dn[(size_t)t * n]);
        if (d == 0) {
            d = 1;
            atomicMin(a.res, (unsigned long long)(((k * a.A + arg) * T + t) * n + i));
        }
        pd = mul(pd, d);
        h[(size_t)t * n] = pd;
    }
    u64 ipd = inv(pd);
    u64 c = run_identity<KIND>();
    for (u32 t = T; t-- > 0;) {
        u64 d = canon(dn[(size_t)t * n]);
        if (d == 0) d = 1;
        u64 v = t ? mul(ipd, h[(size_t)(t - 1) * n]) : ipd;        // 1 / den_t
        if (nm) v = mul(v, nm[(size_t)t * n]);                      // mul takes any u64: the numerator is reduced here
        h[(size_t)t * n] = v;
        ipd = mul(ipd, d);
        c = run_op<KIND>(c, v);
    }
    return c;
}
// n >= 512, a power of two: every block is full
template <int KIND>
__global__ __launch_bounds__(256) void k_run_terms(RunArgs a) {
    __shared__ u64 sh[256];
    const size_t n = (size_t)1 << a.lg, k = blockIdx.z;
    const u32 arg = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const size_t i = (size_t)b * 256 + t;
    const u64 c = run_row<KIND>(a, k, arg, i);
    a.out[((k * a.A + arg) * (size_t)(a.T + 1) + a.T) * n + i] = c;                  // the Z column holds c[i] for now
    sh[t] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (t < (u32)s) sh[t] = run_op<KIND>(sh[t], sh[t + s]); __syncthreads(); }
    if (t == 0) a.tot[(k * a.A + arg) * a.nblocks + b] = sh[0];
}
// exclusive scan of the block totals of one (proof, argument): blockIdx.x = k A + a
template <int KIND>
__global__ __launch_bounds__(256) void k_run_scan_tot(RunArgs a) {
    __shared__ u64 sh[256];
    const u32 t = threadIdx.x, nblocks = a.nblocks;
    u64 *v = a.tot + (size_t)blockIdx.x * nblocks;
    const u32 m = (nblocks + 255) / 256;
    const u32 k0 = min(t * m, nblocks), k1 = min((t + 1) * m, nblocks);
    u64 loc = run_identity<KIND>();
    for (u32 j = k0; j < k1; j++) loc = run_op<KIND>(loc, v[j]);
    sh[t] = loc;
    __syncthreads();
    if (t == 0) {
        u64 acc = run_identity<KIND>();
        for (int j = 0; j < 256; j++) { const u64 x = sh[j]; sh[j] = acc; acc = run_op<KIND>(acc, x); }
        a.res[1 + blockIdx.x] = acc;
    }
    __syncthreads();
    u64 acc = sh[t];
    for (u32 j = k0; j < k1; j++) { const u64 x = v[j]; v[j] = acc; acc = run_op<KIND>(acc, x); }
}
// exclusive scan of 256 values through LDS (Hillis-Steele over `width` lanes, width a power of two <= 256 = blockDim.x); returns
// lane t's exclusive prefix, *all = the combination of all of them
template <int KIND>
__device__ __forceinline__ u64 run_block_scan(u64 (*sh)[256], u32 t, u32 width, u64 mine, u64 *all) {
    int cur = 0;
    sh[0][t] = mine;
    __syncthreads();
    for (u32 off = 1; off < width; off <<= 1) {
        u64 v = sh[cur][t];
        if (t >= off) v = run_op<KIND>(sh[cur][t - off], v);
        sh[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    *all = sh[cur][width - 1];
    return t ? sh[cur][t - 1] : run_identity<KIND>();
}
template <int KIND>
__global__ __launch_bounds__(256) void k_run_apply(RunArgs a) {
    __shared__ u64 sh[2][256];
    const size_t n = (size_t)1 << a.lg, k = blockIdx.z;
    const u32 arg = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    u64 *z = a.out + ((k * a.A + arg) * (size_t)(a.T + 1) + a.T) * n + (size_t)b * 256 + t;
    u64 all;
    const u64 excl = run_block_scan<KIND>(sh, t, 256, *z, &all);
    *z = run_op<KIND>(a.tot[(k * a.A + arg) * a.nblocks + b], excl);
}
// n <= 256: blockDim.x = max(64, n) lanes, lane t is row t
template <int KIND>
__global__ __launch_bounds__(256) void k_run_small(RunArgs a) {
    __shared__ u64 sh[2][256];
    const size_t n = (size_t)1 << a.lg, k = blockIdx.y;
    const u32 arg = blockIdx.x, t = threadIdx.x;
    const u64 c = t < n ? run_row<KIND>(a, k, arg, t) : run_identity<KIND>();
    u64 all;
    const u64 excl = run_block_scan<KIND>(sh, t, blockDim.x, c, &all);
    if (t < n) a.out[((k * a.A + arg) * (size_t)(a.T + 1) + a.T) * n + t] = excl;
    if (t == 0) a.res[1 + k * a.A + arg] = all;
}

namespace {
// nums or dens in host memory: the A T n words in use of every proof, canonical or refused naming the array, the proof and the word
int run_words_check(const char *fn, const char *name, const u64 *v, u32 K, size_t stride, size_t per_proof) {
    for (u32 k = 0; k < K; k++) {
        const size_t bad = first_noncanonical(v + k * stride, per_proof);
        GLP_REQUIRE(bad == per_proof, "%s: %s: proof %u, word %zu = 0x%016llx is not a canonical field element (>= p)", fn, name, k, bad,
                    (unsigned long long)v[k * stride + (bad == per_proof ? 0 : bad)]);
    }
    return GLP_OK;
}
// host nums or dens -> HBM, the words in use packed [K][A T n]
int run_input(glp_ctx *c, Scratch &tmp, const u64 *host, u32 K, size_t stride, size_t per_proof, const u64 **dev) {
    if (K == 1 || stride == per_proof) return tmp.input(host, 0, (size_t)K * per_proof, dev);
    u64 *d;
    GLP_TRY(tmp.words(&d, (size_t)K * per_proof));
    GLP_HIP(hipMemcpy2DAsync(d, per_proof * 8, host, stride * 8, per_proof * 8, K, hipMemcpyHostToDevice, c->stream));
    *dev = d;
    return GLP_OK;
}
template <int KIND>
int run_launch(glp_ctx *c, const RunArgs &a, u32 K, bool with_nums) {
    const size_t n = (size_t)1 << a.lg;
    const double cells = (double)n * K * a.A;
    if (n <= 256) {             // one launch; the scan is inside it
        StageScope st(c, "running.terms", 8.0 * cells * ((with_nums ? 2.0 : 1.0) * a.T + a.T + 1));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_run_small<KIND>), dim3(a.A, K), dim3((unsigned)std::max<size_t>(64, n)), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
        return GLP_OK;
    }
    {
        StageScope st(c, "running.terms", 8.0 * cells * ((with_nums ? 2.0 : 1.0) * a.T + a.T + 1));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_run_terms<KIND>), dim3(a.nblocks, a.A, K), dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
    }
    {
        StageScope st(c, "running.scan", 8.0 * cells * 2);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_run_scan_tot<KIND>), dim3(a.A * K), dim3(256), 0, c->stream, a);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_run_apply<KIND>), dim3(a.nblocks, a.A, K), dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
    }
    return GLP_OK;
}
}  // namespace

extern "C" {

int glp_running_columns(glp_ctx *c, uint32_t kind, uint32_t num_proofs, uint32_t num_args, uint32_t num_terms, uint32_t log_n, const uint64_t *nums,
                        const uint64_t *dens, size_t in_proof_stride, int inputs_on_device, uint64_t *out, int out_on_device, uint64_t *totals_out) {
    static const char *fn = "glp_running_columns";
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    GLP_REQUIRE(dens, "%s: dens is null", fn);
    GLP_REQUIRE(out, "%s: out is null", fn);
    GLP_REQUIRE(totals_out, "%s: totals_out is null", fn);
    GLP_REQUIRE(kind == GLP_RUN_SUM || kind == GLP_RUN_PRODUCT, "%s: kind = %u is not one of GLP_RUN_*", fn, kind);
    const u32 K = num_proofs, A = num_args, T = num_terms, lg = log_n;
    GLP_TRY(seam_num_proofs_check(fn, K));
    GLP_REQUIRE(A >= 1 && A <= 16, "%s: num_args = %u outside 1..16", fn, A);
    GLP_REQUIRE(T >= 1 && T <= 64, "%s: num_terms = %u outside 1..64", fn, T);
    GLP_REQUIRE(lg <= (u32)NTT_MAX_LG, "%s: log_n = %u is more than %d", fn, lg, NTT_MAX_LG);
    const size_t n = (size_t)1 << lg, per_proof = (size_t)A * T * n;
    GLP_REQUIRE((size_t)K * A * (T + 1) <= BATCH_MAX_BYTES / (8 * n), "%s: out too large (num_proofs * num_args * (num_terms + 1) * 2^log_n words)", fn);
    GLP_REQUIRE(in_proof_stride >= per_proof, "%s: in_proof_stride = %zu is less than num_args * num_terms * 2^log_n = %zu", fn, in_proof_stride, per_proof);
    GLP_REQUIRE(in_proof_stride <= BATCH_MAX_BYTES / 8, "%s: in_proof_stride = %zu is more than 2^33", fn, in_proof_stride);
    if (!inputs_on_device) {
        GLP_TRY(run_words_check(fn, "dens", dens, K, in_proof_stride, per_proof));
        if (nums) GLP_TRY(run_words_check(fn, "nums", nums, K, in_proof_stride, per_proof));
    }
    GLP_TRY(bind(c));
    Scratch tmp(c);
    RunArgs a;
    memset(&a, 0, sizeof(a));
    a.nums = nums; a.dens = dens; a.in_stride = in_proof_stride;
    if (!inputs_on_device) {
        GLP_TRY(run_input(c, tmp, dens, K, in_proof_stride, per_proof, &a.dens));
        if (nums) GLP_TRY(run_input(c, tmp, nums, K, in_proof_stride, per_proof, &a.nums));
        a.in_stride = per_proof;
    }
    const size_t words = (size_t)K * A * (T + 1) * n;
    a.out = out;
    if (!out_on_device) GLP_TRY(tmp.words(&a.out, words));
    a.lg = lg; a.A = A; a.T = T; a.nblocks = nblk(n);
    if (n > 256) GLP_TRY(tmp.words(&a.tot, (size_t)K * A * a.nblocks));
    const size_t nres = 1 + (size_t)K * A;
    GLP_TRY(tmp.array(&a.res, nres));
    GLP_HIP(hipMemsetAsync(a.res, 0xFF, 8, c->stream));
    if (kind == GLP_RUN_SUM) GLP_TRY(run_launch<(int)GLP_RUN_SUM>(c, a, K, nums != nullptr));
    else GLP_TRY(run_launch<(int)GLP_RUN_PRODUCT>(c, a, K, nums != nullptr));
    std::vector<unsigned long long> res(nres);
    GLP_TRY(d2h(c, res.data(), a.res, nres * 8));
    if (res[0] != ~0ull) {
        const size_t f = (size_t)res[0];
        return set_error(GLP_ERR_PROVE, "%s: zero denominator at proof %zu, argument %zu, term %zu, row %zu", fn, f / per_proof, f / ((size_t)T * n) % A,
                         f / n % T, f % n);
    }
    for (size_t j = 0; j + 1 < nres; j++) totals_out[j] = res[1 + j];
    if (!out_on_device) GLP_TRY(d2h(c, out, a.out, words * 8));
    return GLP_OK;
}

}  // extern "C"
