// pp_kernels.inc -- K5: the partial products of the permutation argument and Z.  Included by prover.hip; launched by
// stage_partial_products (prover_stages.inc).
struct PPArgs {
    const u64 *wires, *sigmas, *k_is;
    u64 *zp, *dens;      // dens: scratch [nch][npp + 1][n]
    u64 betas[MAXCH], gammas[MAXCH];
    u64 w_n;
    u32 lg, nr, nch, npp, qdf;
    // many-proofs batch (blockIdx.y = proof): challenges from chal[proof][2 MAXCH] (betas, gammas), arrays strided per proof
    const u64 *chal;
    size_t wires_stride, zp_stride;
};
// K5a: per row, the running products of the quotient chunks  prod_{j in chunk} (w_j + beta k_j x + gamma)/(w_j + beta sigma_j + gamma)
template <int NCH>
__global__ __launch_bounds__(256) void k_pp_rows(PPArgs a) {
    const size_t n = (size_t)1 << a.lg;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u64 betas[MAXCH], gammas[MAXCH];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) { betas[c] = a.betas[c]; gammas[c] = a.gammas[c]; }
    if (a.chal) {
        const size_t pk = blockIdx.y;
        a.wires += pk * a.wires_stride; a.zp += pk * a.zp_stride; a.dens += pk * a.zp_stride;
        _Pragma("unroll") for (int c = 0; c < NCH; c++) { betas[c] = a.chal[pk * 2 * MAXCH + c]; gammas[c] = a.chal[pk * 2 * MAXCH + MAXCH + c]; }
    }
    const u64 x = dpow(a.w_n, i);
    // Pass 1: prefix products of the chunk numerators (into the output columns) and the chunk denominators
    // (into `dens`); pass 2 walks back down with ONE field inversion per challenge instead of one per chunk:
    // 1/PD_k = (1/PD_{k+1}) * den_{k+1}.
    u64 pn[MAXCH], pd[MAXCH];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) { pn[c] = 1; pd[c] = 1; }
    for (u32 chunk = 0; chunk <= a.npp; chunk++) {
        u64 num[MAXCH], den[MAXCH];
        _Pragma("unroll") for (int c = 0; c < NCH; c++) { num[c] = 1; den[c] = 1; }
        const u32 j1 = min((chunk + 1) * a.qdf, a.nr);
        for (u32 j = chunk * a.qdf; j < j1; j++) {
            const u64 w = canon(a.wires[(size_t)j * n + i]), s = canon(a.sigmas[(size_t)j * n + i]);   // a caller's device words: reduced as loaded
            const u64 kx = mul(a.k_is[j], x);
            _Pragma("unroll") for (int c = 0; c < NCH; c++) {
                num[c] = mul(num[c], add(add(w, mul(betas[c], kx)), gammas[c]));
                den[c] = mul(den[c], add(add(w, mul(betas[c], s)), gammas[c]));
            }
        }
        _Pragma("unroll") for (int c = 0; c < NCH; c++) {
            pn[c] = mul(pn[c], num[c]);
            pd[c] = mul(pd[c], den[c]);
            const u32 col = chunk < a.npp ? NCH + c * a.npp + chunk : c;   // Z column holds the row product for now
            a.zp[(size_t)col * n + i] = pn[c];
            a.dens[((size_t)c * (a.npp + 1) + chunk) * n + i] = den[c];
        }
    }
    u64 ipd[MAXCH];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) ipd[c] = inv(pd[c]);
    for (int chunk = (int)a.npp; chunk >= 0; chunk--) {
        _Pragma("unroll") for (int c = 0; c < NCH; c++) {
            const u32 col = (u32)chunk < a.npp ? NCH + c * a.npp + chunk : c;
            const size_t o = (size_t)col * n + i;
            a.zp[o] = mul(a.zp[o], ipd[c]);
            ipd[c] = mul(ipd[c], a.dens[((size_t)c * (a.npp + 1) + chunk) * n + i]);
        }
    }
}

// The same for traces of at most 128 rows (a batch of small proofs: blockIdx.y = proof, one workgroup per proof).  k_pp_rows gives a row to a lane, and a
// lane then walks ~1000 dependent multiplications (80 wires x two challenges, one inversion per challenge) while 56 lanes of its wave idle: 120 us per 256
// zkdsa proofs, all of it latency.  Here a lane takes one (row, chunk, challenge): the chunk products in parallel through LDS, then one lane per
// (row, challenge) for the prefix products, the inversion and the walk back -- ~170 dependent multiplications -- and, since the whole trace is in this
// workgroup, the running product over the rows as well (k_pp_block_tot / k_pp_scan_tot / k_pp_apply of the large path).  Same values in the same places.
__global__ __launch_bounds__(256) void k_pp_rows_small(PPArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 pp_lds[];
    const u32 n = 1u << a.lg, nchunks = a.npp + 1, nch = a.nch, units = n * nchunks * nch;
    u64 *snum = pp_lds, *sden = pp_lds + units;              // [c][chunk][i]
    u64 *rowp = pp_lds + 2 * (size_t)units, *zrow = rowp + (size_t)nch * n;      // [c][i]: row products, running products
    const size_t pk = blockIdx.y;
    if (a.chal) { a.wires += pk * a.wires_stride; a.zp += pk * a.zp_stride; }
    const u64 *ch = a.chal ? a.chal + pk * 2 * MAXCH : nullptr;
    for (u32 u = threadIdx.x; u < units; u += 256) {
        const u32 i = u % n, chunk = (u / n) % nchunks, c = u / (n * nchunks);
        const u64 beta = ch ? ch[c] : a.betas[c], gamma = ch ? ch[MAXCH + c] : a.gammas[c];
        const u64 x = dpow(a.w_n, i);
        u64 num = 1, den = 1;
        const u32 j1 = min((chunk + 1) * a.qdf, a.nr);
        for (u32 j = chunk * a.qdf; j < j1; j++) {
            const u64 w = canon(a.wires[(size_t)j * n + i]), sg = canon(a.sigmas[(size_t)j * n + i]);
            num = mul(num, add(add(w, mul(beta, mul(a.k_is[j], x))), gamma));
            den = mul(den, add(add(w, mul(beta, sg)), gamma));
        }
        snum[u] = num; sden[u] = den;
    }
    __syncthreads();
    for (u32 u = threadIdx.x; u < n * nch; u += 256) {
        const u32 i = u % n, c = u / n;
        const u64 *nm = snum + (size_t)c * nchunks * n + i, *dn = sden + (size_t)c * nchunks * n + i;
        u64 pn = 1, pd = 1;
        for (u32 chunk = 0; chunk < nchunks; chunk++) {
            pn = mul(pn, nm[(size_t)chunk * n]);
            pd = mul(pd, dn[(size_t)chunk * n]);
            const u32 col = chunk < a.npp ? nch + c * a.npp + chunk : c;   // Z column holds the row product for now
            a.zp[(size_t)col * n + i] = pn;
        }
        u64 ipd = inv(pd);
        for (int chunk = (int)a.npp; chunk >= 0; chunk--) {
            const u32 col = (u32)chunk < a.npp ? nch + c * a.npp + chunk : c;
            const size_t o = (size_t)col * n + i;
            const u64 v = mul(a.zp[o], ipd);
            a.zp[o] = v;
            if ((u32)chunk == a.npp) rowp[(size_t)c * n + i] = v;          // the row's whole product
            ipd = mul(ipd, dn[(size_t)chunk * n]);
        }
    }
    __syncthreads();
    // Z_i = product of the rows before i (one lane per challenge walks the <= 128 rows), then every partial product of row i times Z_i
    if (threadIdx.x < nch) {
        const u32 c = threadIdx.x;
        u64 acc = 1;
        for (u32 i = 0; i < n; i++) { const u64 r = rowp[(size_t)c * n + i]; zrow[(size_t)c * n + i] = acc; acc = mul(acc, r); }
    }
    __syncthreads();
    for (u32 u = threadIdx.x; u < units; u += 256) {
        const u32 i = u % n, k = (u / n) % nchunks, c = u / (n * nchunks);
        const u64 z = zrow[(size_t)c * n + i];
        if (k < a.npp) { const size_t o = (size_t)(nch + c * a.npp + k) * n + i; a.zp[o] = mul(a.zp[o], z); }
        else a.zp[(size_t)c * n + i] = z;
    }
}
// K5b: product of each block of 256 row products
__global__ __launch_bounds__(256) void k_pp_block_tot(const u64 *zp, u64 *tot, u32 lg, u32 nblocks, size_t zp_stride) {
    __shared__ u64 sh[256];
    zp += (size_t)blockIdx.z * zp_stride; tot += (size_t)blockIdx.z * gridDim.y * nblocks;
    const size_t n = (size_t)1 << lg;
    const u32 c = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const size_t i = (size_t)b * 256 + t;
    sh[t] = i < n ? zp[(size_t)c * n + i] : 1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (t < s) sh[t] = mul(sh[t], sh[t + s]); __syncthreads(); }
    if (t == 0) tot[(size_t)c * nblocks + b] = sh[0];
}
// K5c: exclusive prefix product of the block totals (one workgroup per challenge)
__global__ __launch_bounds__(256) void k_pp_scan_tot(u64 *tot, u32 nblocks) {
    __shared__ u64 sh[256];
    const u32 c = blockIdx.x, t = threadIdx.x;
    u64 *v = tot + ((size_t)blockIdx.y * gridDim.x + c) * nblocks;
    const u32 m = (nblocks + 255) / 256;
    u64 loc = 1;
    for (u32 k = t * m; k < min((t + 1) * m, nblocks); k++) loc = mul(loc, v[k]);
    sh[t] = loc;
    __syncthreads();
    if (t == 0) { u64 acc = 1; for (int k = 0; k < 256; k++) { u64 x = sh[k]; sh[k] = acc; acc = mul(acc, x); } }
    __syncthreads();
    u64 acc = sh[t];
    for (u32 k = t * m; k < min((t + 1) * m, nblocks); k++) { u64 x = v[k]; v[k] = acc; acc = mul(acc, x); }
}
// K5d: Z(x_i) = prefix(block) * in-block exclusive scan; partial products *= Z
__global__ __launch_bounds__(256) void k_pp_apply(u64 *zp, const u64 *tot, u32 lg, u32 nblocks, u32 nch, u32 npp, size_t zp_stride) {
    __shared__ u64 sh[2][256];
    zp += (size_t)blockIdx.z * zp_stride; tot += (size_t)blockIdx.z * gridDim.y * nblocks;
    const size_t n = (size_t)1 << lg;
    const u32 c = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const size_t i = (size_t)b * 256 + t;
    const u64 mine = i < n ? zp[(size_t)c * n + i] : 1;
    int cur = 0;
    sh[0][t] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {     // Hillis-Steele inclusive scan
        u64 v = sh[cur][t];
        if (t >= off) v = mul(sh[cur][t - off], v);
        sh[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    const u64 excl = t ? sh[cur][t - 1] : 1;
    if (i >= n) return;
    const u64 z = mul(tot[(size_t)c * nblocks + b], excl);
    zp[(size_t)c * n + i] = z;
    for (u32 k = 0; k < npp; k++) {
        const size_t o = (size_t)(nch + c * npp + k) * n + i;
        zp[o] = mul(zp[o], z);
    }
}
