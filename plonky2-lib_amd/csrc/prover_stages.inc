// prover_stages.inc -- the device stages of one prove call, each in ONE host function.  Included by prover.hip between the
// kernels and the three drivers that walk these stages: glp_session (one proof, challenges handed in as host values),
// prove_batch_impl (prover_batch.inc: K proofs, transcripts on host threads) and prove_batch_impl_dev (prover_batch_dev.inc:
// K proofs, transcripts on the device).
//
// A driver owns the transcript and the data movement: where a challenge comes from, where caps and openings go, every
// upload, copy back and synchronisation.  A stage function owns the launches: it fills the kernel's argument struct,
// chooses the kernel from the circuit's shape and checks hipGetLastError.  None of them synchronises or copies to the host.
// The kernels take the proof index in a grid dimension and a stride per proof; a device array of per-proof challenges
// (`chal`, `pp`, `zetas`, `betas`) that is null means ONE proof whose challenges ride in the kernel arguments, which is
// how the single-proof session calls the same functions with K = 1.
#include <stdlib.h>
#include <chrono>

namespace {

// what every stage needs of the circuit and the batch, computed once per prove call
struct ProveGeo {
    const glp_circuit *cc;                         // nullptr: no circuit (fri_openings.inc), only the FRI fields below are set
    int lg, rb, qdb, hasher, cap_height;           // qdb: log2 of the evaluated quotient planes
    size_t n, N;
    u32 nch, nr, nw, nc, qdf, npp, nzp, capn, Rq, step, nterms, K;
    const u32 *arity_bits;                         // FRI: reduction_arity_bits of the owner (circuit description or glp_fri)
    u32 nq;                                        // FRI: num_query_rounds
};
ProveGeo prove_geo(const glp_circuit *cc, u32 K) {
    const glp_circuit_desc &d = cc->d;
    ProveGeo g;
    g.cc = cc; g.K = K;
    g.lg = (int)d.degree_bits; g.rb = (int)d.rate_bits; g.hasher = (int)d.hasher; g.cap_height = (int)d.cap_height;
    g.n = (size_t)1 << g.lg; g.N = g.n << g.rb;
    g.nch = d.num_challenges; g.nr = d.num_routed_wires; g.nw = d.num_wires; g.nc = d.num_constants;
    g.qdf = d.quotient_degree_factor; g.npp = d.num_partial_products;
    g.nzp = g.nch * (1 + g.npp); g.capn = 1u << d.cap_height;
    g.qdb = 0;
    while ((1u << g.qdb) < g.qdf) g.qdb++;
    g.Rq = 1u << g.qdb; g.step = 1u << (g.rb - g.qdb);
    g.nterms = g.nch + g.nch * (g.npp + 1) + d.num_gate_constraints;
    g.arity_bits = d.reduction_arity_bits; g.nq = d.num_query_rounds;
    return g;
}
// the constants/sigmas oracle (oracle 0) is shared by all proofs of a batch, the other three advance per proof
inline size_t per_proof(int oracle, size_t words) { return oracle ? words : 0; }
inline size_t oracle_cols(const glp_batch *const ob[4]) { return (size_t)ob[0]->ncols + ob[1]->ncols + ob[2]->ncols + ob[3]->ncols; }

// a kernel template over the number of challenges, 1..MAXCH (checked by the caller), launched for a run-time nch
#define GLP_LAUNCH_NCH(kernel, nch, grid, block, lds, stream, ...)                                                  \
    switch (nch) {                                                                                                  \
    case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<1>), grid, block, lds, stream, __VA_ARGS__); break;           \
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<2>), grid, block, lds, stream, __VA_ARGS__); break;           \
    case 3: hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<3>), grid, block, lds, stream, __VA_ARGS__); break;           \
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(kernel<4>), grid, block, lds, stream, __VA_ARGS__); break;          \
    }
static_assert(MAXCH == 4, "GLP_LAUNCH_NCH instantiates 1..4");

// K5 without a circuit: what the kernels read of the permutation argument.  The library's own drivers fill it from the circuit
// (stage_partial_products below), the seam from the caller's description (perm_seam.inc).
struct PermGeo { int lg; u32 nw, nr, nch, npp, qdf, K; };
// g if k_is[j] = g^j for every j with g < 2^32 (plonky2's get_unique_coset_shifts: powers of the generator 7), else 0: then the
// quotient kernels chain beta k_j x by g instead of multiplying by k_j
inline u32 coset_shift_ratio(const u64 *k_is, size_t nr) {
    if (nr < 2 || k_is[0] != 1 || k_is[1] <= 1 || k_is[1] >= (1ull << 32)) return 0;
    const u32 g = (u32)k_is[1];
    for (size_t j = 1; j < nr; j++)
        if (k_is[j] != mul(k_is[j - 1], (u64)g)) return 0;
    return g;
}
// wires [K][nw][n], sigmas [nr][n] and k_is [nr] on the device.  chal == nullptr: one proof, challenges from betas / gammas; else
// chal[K][2 MAXCH] on the device.  zp, dens: [K][nch (npp + 1)][n]; tot: [K][nch][blocks of 256 rows].
int launch_partial_products(glp_ctx *c, const PermGeo &g, const u64 *wires, const u64 *sigmas, const u64 *k_is, const u64 *betas,
                            const u64 *gammas, const u64 *chal, u64 *zp, u64 *dens, u64 *tot) {
    const size_t n = (size_t)1 << g.lg;
    const u32 nch = g.nch, npp = g.npp, K = g.K, lg = (u32)g.lg, nblocks = nblk(n);
    PPArgs a;
    a.wires = wires; a.sigmas = sigmas; a.k_is = k_is; a.zp = zp; a.dens = dens;
    for (u32 i = 0; i < MAXCH; i++) { a.betas[i] = !chal && i < nch ? betas[i] : 0; a.gammas[i] = !chal && i < nch ? gammas[i] : 0; }
    a.w_n = root_of_unity(g.lg); a.lg = lg; a.nr = g.nr; a.nch = nch; a.npp = npp; a.qdf = g.qdf;
    a.chal = chal; a.wires_stride = (size_t)g.nw * n; a.zp_stride = (size_t)nch * (1 + npp) * n;
    const size_t small_lds = (size_t)2 * nch * (npp + 2) * n * sizeof(u64);       // k_pp_rows_small: chunk products, row products and running products of one proof in LDS
    if (g.lg <= 7 && small_lds <= 64 * 1024) {     // at most 128 rows: (row, chunk, challenge) per lane, one workgroup per proof; the running product too
        hipLaunchKernelGGL(k_pp_rows_small, dim3(1, K), dim3(256), small_lds, c->stream, a);
        GLP_HIP(hipGetLastError());
        return GLP_OK;
    }
    GLP_LAUNCH_NCH(k_pp_rows, nch, dim3(nblocks, K), dim3(256), 0, c->stream, a);
    GLP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pp_block_tot, dim3(nblocks, nch, K), dim3(256), 0, c->stream, zp, tot, lg, nblocks, a.zp_stride);
    hipLaunchKernelGGL(k_pp_scan_tot, dim3(nch, K), dim3(256), 0, c->stream, tot, nblocks);
    hipLaunchKernelGGL(k_pp_apply, dim3(nblocks, nch, K), dim3(256), 0, c->stream, zp, tot, lg, nblocks, nch, npp, a.zp_stride);
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}
// K5 of a circuit: partial products and Z from its sigmas and coset shifts
int stage_partial_products(glp_ctx *c, const ProveGeo &g, const u64 *wires, const u64 *betas, const u64 *gammas, const u64 *chal,
                           u64 *zp, u64 *dens, u64 *tot) {
    const PermGeo pg = {g.lg, g.nw, g.nr, g.nch, g.npp, g.qdf, g.K};
    return launch_partial_products(c, pg, wires, g.cc->dev_sigmas, g.cc->dev_k_is, betas, gammas, chal, zp, dens, tot);
}

// out[e] = alpha^e, e < count
void alpha_powers(u64 alpha, u32 count, u64 *out) {
    u64 x = 1;
    for (u32 e = 0; e < count; e++) { out[e] = x; x = mul(x, alpha); }
}
// alpha powers twice: whole (permutation terms) and as 22-bit limbs of m and m 2^32 (gate constraints, AccHL):
// whole[nch][nterms], limbs[nch][nterms][APL_WORDS]
void alpha_power_table(const u64 *alphas, u32 nch, u32 nterms, u64 *whole, u64 *limbs) {
    for (u32 i = 0; i < nch; i++) {
        alpha_powers(alphas[i], nterms, whole + (size_t)i * nterms);
        for (size_t e = (size_t)i * nterms; e < (size_t)(i + 1) * nterms; e++) apl_words(whole[e], limbs + APL_WORDS * e);
    }
}
// The evaluated planes of the coset g <W>, W of order 2^(lg + plane_bits): plane i of `planes` is LDE plane r = i step of 2^plane_bits.
// Fills what k_l0_table reads and zh_inv[i] = 1 / Z_H on that plane.
void coset_plane_tables(int lg, int plane_bits, u32 planes, u32 step, L0Args &la, u64 *zh_inv) {
    memset(&la, 0, sizeof(la));
    const u64 W = root_of_unity(lg + plane_bits), gn = pow(GEN, (u64)1 << lg), wR = root_of_unity(plane_bits);
    for (u32 i = 0; i < planes; i++) {
        const u32 r = i * step;
        la.shift_r[i] = mul(GEN, pow(W, (u64)r));
        la.zh[i] = sub(mul(gn, pow(wR, (u64)r)), 1);       // Z_H(g W^(q 2^plane_bits + r)) = g^n w_R^r - 1
        zh_inv[i] = inv(la.zh[i]);
    }
    la.w_n = root_of_unity(lg); la.n_field = ((u64)1 << lg) % P; la.lg = (u32)lg;
}
// the per-proof quotient arguments over the committed wires and Z oracles.  dev_apow: [K][nch * nterms] whole powers, the limb forms
// of all proofs after them.  dev_pp: [K][3 MAXCH] betas, gammas, public-input hash; nullptr: one proof, the caller writes them into qp.
void quotient_proof_args(const ProveGeo &g, const glp_batch *wb, const glp_batch *zb, u64 *qv, const u64 *dev_apow, const u64 *dev_pp,
                         QProof &qp, QBatch &qb) {
    memset(&qp, 0, sizeof(qp));
    qb.apow_stride = (size_t)g.nch * g.nterms;
    qp.wl = wb->lde; qp.zl = zb->lde; qp.out = qv; qp.apow = dev_apow; qp.apl = dev_apow + g.K * qb.apow_stride;
    qb.pp = dev_pp; qb.wl_stride = (size_t)(g.nw + wb->salt) * g.N; qb.zl_stride = (size_t)(g.nzp + zb->salt) * g.N;
    qb.out_stride = (size_t)g.nch * g.Rq * g.n;
}
// the gates of type GLP_GATE_PROGRAM, one k_quotient_gate_program launch each (circuit_program.inc)
int quotient_program_launches(glp_ctx *c, const glp_circuit *cc, u32 nch, dim3 grid, const QArgs &a, const QProof &qp, const QBatch &qbt);
// K6: the quotient's values on the Rq evaluated planes -> qp.out.  l0t: scratch [Rq][n].
int stage_quotient_eval(glp_ctx *c, const ProveGeo &g, const QProof &qp, const QBatch &qbt, u64 *l0t) {
    const glp_circuit *cc = g.cc;
    const glp_circuit_desc &d = cc->d;
    const u32 nch = g.nch;
    QArgs a;
    a.cs = cc->cs->lde; a.gates = cc->dev_gates; a.k_is = cc->dev_k_is; a.k_ratio = cc->k_ratio;
    L0Args la;
    coset_plane_tables(g.lg, g.rb, g.Rq, g.step, la, a.zh_inv);
    memcpy(a.shift_r, la.shift_r, sizeof(u64) * g.Rq); memcpy(a.zh, la.zh, sizeof(u64) * g.Rq);
    a.w_n = la.w_n; a.n_field = la.n_field;
    a.lg = (u32)g.lg; a.rb = (u32)g.rb; a.step = g.step; a.nc = g.nc; a.nsel = d.num_selectors; a.nr = g.nr; a.nw = g.nw;
    a.nch = nch; a.npp = g.npp; a.qdf = g.qdf; a.num_gates = d.num_gates; a.nterms = g.nterms;
    a.many_selectors = d.num_selectors > 1;
    // two challenges (every preset the reference uses): permutation terms in one launch, then one launch per
    // gate type compiled on its own; other challenge counts take the monolithic kernel
    a.gate_mode = nch == 2 ? 1 : 0;
    a.l0 = l0t;
    hipLaunchKernelGGL(k_l0_table, dim3(nblk(g.n)), dim3(256), 0, c->stream, la, l0t, g.Rq);
    GLP_HIP(hipGetLastError());
    LightArgs lg_;
    lg_.count = cc->light_count; lg_.arith_gi = cc->arith_gi; lg_.arith_ops = cc->arith_ops;
    for (u32 i = 0; i < 8; i++) lg_.gi[i] = cc->light_gi[i];
    const dim3 grid(nblk(g.n), g.Rq, g.K);
    switch (nch) {
    case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<1, 1>), grid, dim3(256), 0, c->stream, a, qp, qbt, lg_); break;
    case 2:
        if (cc->light_count || cc->arith_ops) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<2, 2>), grid, dim3(256), 0, c->stream, a, qp, qbt, lg_);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<2, 0>), grid, dim3(256), 0, c->stream, a, qp, qbt, lg_);
        break;
    case 3: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<3, 1>), grid, dim3(256), 0, c->stream, a, qp, qbt, lg_); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<4, 1>), grid, dim3(256), 0, c->stream, a, qp, qbt, lg_); break;
    }
    GLP_HIP(hipGetLastError());
    if (a.gate_mode != 1) return quotient_program_launches(c, cc, nch, grid, a, qp, qbt);      // the monolithic kernel skips type 23
    if (cc->limb_count) {
        LimbArgs la;
        limb_args(cc, la);
        la.extra_count = cc->limb_extra_count;
        for (int i = 0; i < 4; i++) la.extra_gi[i] = cc->limb_extra_gi[i];
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient_limbs<2>), grid, dim3(256), 0, c->stream, a, qp, qbt, la);
        GLP_HIP(hipGetLastError());
    }
    for (u32 gi : cc->single_gates) {
#define GLP_GATE_LAUNCH(T) case T: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient_gate<2, T>), grid, dim3(256), 0, c->stream, a, qp, qbt, gi); break;
        switch (cc->gates[gi].type) {
            GLP_CONSTRAINED_GATES(GLP_GATE_LAUNCH)      // gate_shapes.h: every type that has constraints
        default: break;   // NoopGate: no constraints
        }
#undef GLP_GATE_LAUNCH
        GLP_HIP(hipGetLastError());
    }
    return quotient_program_launches(c, cc, nch, grid, a, qp, qbt);
}
// values on the planes (qv) -> the quotient chunks' coefficients (qc, bit-reversed order); qV: scratch.  All [K][nch][Rq][n].
int stage_quotient_coeffs(glp_ctx *c, const ProveGeo &g, u64 *qv, u64 *qV, u64 *qc) {
    return coset_planes_to_chunk_coeffs(c, qv, qV, qc, g.K * g.nch, g.lg, g.qdb, GEN);
}

// K7.  Partial sums of one proof: the four oracles at zeta, then the Z columns at g zeta; poff[b] = where block b starts, poff[5] = words per proof
void open_offsets(const ProveGeo &g, const glp_batch *const ob[4], size_t poff[6]) {
    poff[0] = 0;
    for (int b = 0; b < 5; b++) poff[b + 1] = poff[b] + (size_t)(b < 4 ? ob[b]->ncols : g.nch) * open_blocks(g.n) * 2;
}
// every committed polynomial at zeta, Z at g zeta, queued back to back -> partial [K][poff[5]].  zeta_host == nullptr: the points come
// from dev_zetas[K][4] (zeta, g zeta); else one proof at zeta_host[0], zeta_host[1].  zt: scratch [K][2 n].
int stage_open(glp_ctx *c, const ProveGeo &g, const glp_batch *const ob[4], const ext2 *zeta_host, const u64 *dev_zetas, u64 *zt,
               u64 *partial, const size_t poff[6]) {
    const size_t n = g.n;
    for (int which = 0; which < 2; which++) {
        ZTArgs za;
        za.zt = zt; za.lg = (u32)g.lg;
        if (zeta_host) {
            za.zeta_b = nullptr; za.zeta_stride = 0;
            ext2 p = zeta_host[which];
            for (int b = 0; b < 24; b++) { za.zp2[b] = p; p = e_sqr(p); }
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_zeta_table<false>), dim3(nblk(n)), dim3(256), 0, c->stream, za);
        } else {
            za.zeta_b = dev_zetas + 2 * which; za.zeta_stride = 4;
            for (int b = 0; b < 24; b++) za.zp2[b] = e_from(0);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_zeta_table<true>), dim3(nblk(n), g.K), dim3(256), 0, c->stream, za);
        }
        GLP_HIP(hipGetLastError());
        for (int b = which ? 2 : 0; b < (which ? 3 : 4); b++) {        // at g zeta: only the Z columns of oracle 2
            hipLaunchKernelGGL(k_open_dot, dim3(open_blocks(n), which ? g.nch : ob[b]->ncols, g.K), dim3(256), 0, c->stream, ob[b]->coeffs, zt,
                               partial + poff[which ? 4 : b], (u32)g.lg, per_proof(b, ob[b]->ncols * n), (size_t)2 * n, poff[5]);
            GLP_HIP(hipGetLastError());
        }
    }
    return GLP_OK;
}
// host side of the same: fold the open_blocks partial sums of each column
void open_batch_finish(const u64 *h, u32 ncols, u32 nob, std::vector<ext2> &out) {
    out.resize(ncols);
    for (u32 col = 0; col < ncols; col++) {
        u64 a = 0, bb = 0;
        for (u32 k = 0; k < nob; k++) { a = add(a, h[2 * ((size_t)col * nob + k)]); bb = add(bb, h[2 * ((size_t)col * nob + k) + 1]); }
        out[col] = e_make(a, bb);
    }
}
// one proof's partial sums h -> open[4] (per oracle), zs_next, and the proof's openings op in OpeningSet order
void openings_to_proof(const ProveGeo &g, const glp_batch *const ob[4], const u64 *h, const size_t poff[6], std::vector<ext2> open[4],
                       std::vector<ext2> &zs_next, u64 *op) {
    const u32 nob = open_blocks(g.n), nch = g.nch;
    for (int b = 0; b < 4; b++) open_batch_finish(h + poff[b], ob[b]->ncols, nob, open[b]);
    open_batch_finish(h + poff[4], nch, nob, zs_next);
    size_t o = 0;
    auto put = [&](ext2 e) { op[o++] = e.a; op[o++] = e.b; };
    for (u32 k = 0; k < g.nc + g.nr; k++) put(open[0][k]);
    for (u32 k = 0; k < g.nw; k++) put(open[1][k]);
    for (u32 k = 0; k < nch; k++) put(open[2][k]);
    for (u32 k = 0; k < nch; k++) put(zs_next[k]);
    for (u32 k = 0; k < nch * g.npp; k++) put(open[2][nch + k]);
    for (u32 k = 0; k < nch * g.qdf; k++) put(open[3][k]);
}
// the order plonky2 observes an OpeningSet in: constants/sigmas, wires, zs, partial products, quotient, zs_next
void observe_openings(Challenger &ch, const ProveGeo &g, const u64 *op) {
    const u32 nch = g.nch;
    const u64 *p_cs = op, *p_w = op + 2 * (g.nc + g.nr), *p_zs = p_w + 2 * g.nw, *p_zn = p_zs + 2 * nch;
    const u64 *p_pp = p_zn + 2 * nch, *p_q = p_pp + 2 * nch * g.npp;
    ch.observe(p_cs, 2 * (g.nc + g.nr)); ch.observe(p_w, 2 * g.nw); ch.observe(p_zs, 2 * nch);
    ch.observe(p_pp, 2 * (size_t)nch * g.npp); ch.observe(p_q, 2 * (size_t)nch * g.qdf); ch.observe(p_zn, 2 * nch);
}
// FRI batch polynomial: ap[2 oracle_cols] = alpha powers over all columns; pt = the reduced openings at zeta and g zeta,
// the two points, alpha^nch (the order of FVArgs and of its device form pp[10])
void fri_alpha_powers(const ProveGeo &g, const glp_batch *const ob[4], const std::vector<ext2> open[4], const std::vector<ext2> &zs_next,
                      ext2 alpha, ext2 zeta, ext2 zeta_next, u64 *ap, ext2 pt[5]) {
    ext2 x = e_from(1), red0 = e_from(0), red1 = e_from(0);
    size_t j = 0;
    for (int b = 0; b < 4; b++)
        for (u32 col = 0; col < ob[b]->ncols; col++, j++) {
            ap[2 * j] = x.a; ap[2 * j + 1] = x.b;
            red0 = e_add(red0, e_mul(x, open[b][col]));
            x = e_mul(x, alpha);
        }
    x = e_from(1);
    for (u32 col = 0; col < g.nch; col++) { red1 = e_add(red1, e_mul(x, zs_next[col])); x = e_mul(x, alpha); }
    pt[0] = red0; pt[1] = red1; pt[2] = zeta; pt[3] = zeta_next; pt[4] = e_pow(alpha, g.nch);
}

// the FRI batch polynomial's values on coset plane 0 (fv [K][2][n]) -> its coefficients (fcoef, bit-reversed order)
int fri_values_to_coeffs(glp_ctx *c, const ProveGeo &g, const u64 *fv, u64 *fcoef) {
    GLP_TRY(intt_values_to_coeffs(c, fv, fcoef, 2 * g.K, g.lg));
    hipLaunchKernelGGL(k_scale_bitrev_pow, dim3(nblk(g.n), 2 * g.K), dim3(256), 0, c->stream, fcoef, inv(GEN), (u32)g.lg);
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}
// k_final_values_small never flushes its carry-free accumulators, so it serves 4..128 points only while no lane can pass
// ACC_MAX_TERMS terms: lane t of a point takes the columns t, t + lpp, .. of each oracle, lane 0 the most, sum_b ceil(ncols[b] / lpp).
// The bound is the worst case of acc.h, not what natural data needs.  Wider circuits go to k_final_values, which flushes.
inline bool final_values_small_fits(const ProveGeo &g, const glp_batch *const ob[4]) {
    if (g.lg < 2 || g.lg > 7) return false;
    const u32 lpp = 256u >> g.lg;
    size_t lane_terms = 0;
    for (int b = 0; b < 4; b++) lane_terms += (ob[b]->ncols + lpp - 1) / lpp;
    return lane_terms <= ACC_MAX_TERMS;
}
// K8: alpha-combination of all openings batches, quotient by (X - zeta) / (X - g zeta) -> fcoef [K][2][n], the FRI polynomial's
// coefficients; fv: scratch of the same size.  dev_ap [K][2 oracle_cols]; pt != nullptr: one proof with the values of
// fri_alpha_powers; else they come from dev_pp[K][10].
int stage_fri_values(glp_ctx *c, const ProveGeo &g, const glp_batch *const ob[4], const u64 *dev_ap, const ext2 *pt, const u64 *dev_pp,
                     u64 *fv, u64 *fcoef) {
    const ext2 zero = e_from(0);
    FVArgs a;
    for (int b = 0; b < 4; b++) { a.lde[b] = ob[b]->lde; a.ncols[b] = ob[b]->ncols; a.lde_stride[b] = per_proof(b, (ob[b]->ncols + ob[b]->salt) * g.N); }
    a.apow = dev_ap; a.out = fv;
    a.red0 = pt ? pt[0] : zero; a.red1 = pt ? pt[1] : zero; a.zeta = pt ? pt[2] : zero; a.zeta_next = pt ? pt[3] : zero; a.shift_acc = pt ? pt[4] : zero;
    a.w_n = root_of_unity(g.lg); a.g = GEN; a.lg = (u32)g.lg; a.rb = (u32)g.rb; a.nch = g.nch;
    a.pp = pt ? nullptr : dev_pp; a.apow_stride = 2 * oracle_cols(ob); a.out_stride = 2 * g.n;
    if (final_values_small_fits(g, ob)) hipLaunchKernelGGL(k_final_values_small, dim3(1, g.K), dim3(256), 0, c->stream, a);      // 4..128 points: 256 / n lanes per point
    else hipLaunchKernelGGL(k_final_values, dim3(nblk(g.n), g.K), dim3(256), 0, c->stream, a);            // any n (and lg < 2), one lane per point
    GLP_HIP(hipGetLastError());
    return fri_values_to_coeffs(c, g, fv, fcoef);
}

// K9: the commit phase.  One layer per reduction: values on the coset and the tree over arity-sized leaves, [K] of each.
struct FriLayer { u64 *vals, *dig; u32 lgL, ab; size_t ndig; };
struct FriState {
    std::vector<FriLayer> layers;
    u64 *cur = nullptr;        // [K][2][2^lgcur] coefficients of the polynomial being reduced
    int lgcur = 0;
    u64 shift = GEN;
    void start(u64 *fcoef, int lg) { cur = fcoef; lgcur = lg; shift = GEN; }
};
// first half: LDE of the current polynomial on its coset, Merkle tree over the leaves (buffers from tmp); the new layer is f.layers.back()
int stage_fri_commit(glp_ctx *c, const ProveGeo &g, Scratch &tmp, FriState &f) {
    const u32 K = g.K, rb = (u32)g.rb;
    FriLayer ly;
    ly.ab = g.arity_bits[f.layers.size()]; ly.lgL = (u32)(f.lgcur + g.rb);
    const u32 ab = ly.ab, lgL = ly.lgL;
    const size_t Lsz = (size_t)1 << lgL, nleaves = Lsz >> ab;
    ly.ndig = merkle_num_digests(nleaves, g.cap_height);
    GLP_TRY(tmp.words(&ly.vals, (size_t)K * 2 * Lsz));
    GLP_TRY(tmp.words(&ly.dig, (size_t)K * ly.ndig * 4));
    GLP_TRY(lde_coeffs(c, f.cur, ly.vals, 2 * K, f.lgcur, g.rb, f.shift));
    if (g.hasher == GLP_HASH_KECCAK25)
        hipLaunchKernelGGL(k_fri_leaf_hash_keccak, dim3(nblk(nleaves), K), dim3(256), 0, c->stream, ly.vals, ly.dig, lgL, rb, ab, 2 * Lsz, ly.ndig * 4);
    else if (nleaves * K <= c->merkle_coop_max)
        hipLaunchKernelGGL(k_fri_leaf_hash_coop, dim3((unsigned)((nleaves + 15) / 16), K), dim3(256), 0, c->stream, ly.vals, ly.dig, lgL, rb, ab,
                           2 * Lsz, ly.ndig * 4);
    else if (nleaves * K <= c->merkle_quad_max)
        hipLaunchKernelGGL(k_fri_leaf_hash_quad, dim3((unsigned)((nleaves + 63) / 64), K), dim3(256), 0, c->stream, ly.vals, ly.dig, lgL, rb, ab,
                           2 * Lsz, ly.ndig * 4);
    else
        hipLaunchKernelGGL(k_fri_leaf_hash, dim3(nblk(nleaves), K), dim3(256), 0, c->stream, ly.vals, ly.dig, lgL, rb, ab, 2 * Lsz, ly.ndig * 4);
    GLP_HIP(hipGetLastError());
    GLP_TRY(merkle_levels(c, ly.dig, nleaves, g.cap_height, K, ly.ndig * 4, g.hasher));
    f.layers.push_back(ly);
    return GLP_OK;
}
inline const u64 *fri_layer_cap(const ProveGeo &g, const FriLayer &ly) {
    return ly.dig + 4 * merkle_cap_offset(((size_t)1 << ly.lgL) >> ly.ab, g.cap_height);
}
// second half: fold the coefficients (arity 2^ab of the last layer), shift <- shift^arity.  dev_betas == nullptr: one proof, beta by value
int stage_fri_fold(glp_ctx *c, const ProveGeo &g, Scratch &tmp, FriState &f, ext2 beta, const u64 *dev_betas) {
    const u32 ab = f.layers.back().ab;
    const size_t nnew = ((size_t)1 << f.lgcur) >> ab;
    u64 *nxt;
    GLP_TRY(tmp.words(&nxt, (size_t)g.K * 2 * nnew));
    hipLaunchKernelGGL(k_fri_fold, dim3(nblk(nnew), g.K), dim3(256), 0, c->stream, f.cur, nxt, beta, (u32)f.lgcur, ab, dev_betas);
    GLP_HIP(hipGetLastError());
    f.cur = nxt; f.lgcur -= (int)ab;
    f.shift = pow(f.shift, (u64)1 << ab);
    return GLP_OK;
}

// query phase.  Every gather writes into dev_q: `stride` words per query record, `qsec` words from one proof's records to the next; `off` is
// the word offset inside a record and advances by what was written.  The g.nq indices per proof are in dev_idx.
// one initial oracle: the whole leaf (salts ride after the polynomial values), then its Merkle path.  shared: one oracle for all proofs of a batch
int queries_oracle(glp_ctx *c, const ProveGeo &g, const glp_batch *b, bool shared, const u64 *dev_idx, u64 *dev_q, size_t stride, size_t qsec,
                   size_t &off) {
    const u32 ncol = b->ncols + b->salt;
    GLP_TRY(merkle_gather_lde_rows(c, b->lde, ncol, g.lg, g.rb, dev_idx, g.nq, dev_q + off, stride, g.K, shared ? 0 : ncol * g.N, qsec));
    off += ncol;
    GLP_TRY(merkle_gather_paths(c, b->digests, g.N, g.cap_height, dev_idx, g.nq, dev_q + off, stride, 0, g.K, shared ? 0 : b->ndigests * 4, qsec));
    off += 4 * (size_t)(g.lg + g.rb - g.cap_height);
    return GLP_OK;
}
// every commit-phase layer: the evals of the leaf the index falls into, then its Merkle path
int queries_layers(glp_ctx *c, const ProveGeo &g, const std::vector<FriLayer> &layers, const u64 *dev_idx, u64 *dev_q, size_t stride, size_t qsec,
                   size_t &off) {
    u32 shift_bits = 0;
    for (const FriLayer &ly : layers) {
        const u32 arity = 1u << ly.ab;
        const size_t Lsz = (size_t)1 << ly.lgL, nleaves = Lsz >> ly.ab;
        shift_bits += ly.ab;
        hipLaunchKernelGGL(k_fri_gather_leaf, dim3(nblk((size_t)g.nq * arity), g.K), dim3(256), 0, c->stream, ly.vals, ly.lgL, (u32)g.rb, ly.ab, dev_idx,
                           shift_bits, g.nq, dev_q + off, stride, 2 * Lsz, qsec);
        GLP_HIP(hipGetLastError());
        off += 2 * (size_t)arity;
        GLP_TRY(merkle_gather_paths(c, ly.dig, nleaves, g.cap_height, dev_idx, g.nq, dev_q + off, stride, shift_bits, g.K, ly.ndig * 4, qsec));
        off += 4 * (size_t)(ly.lgL - ly.ab - g.cap_height);
    }
    return GLP_OK;
}
// the four initial oracles of a circuit's proof(s), then the layers
int stage_queries(glp_ctx *c, const ProveGeo &g, const glp_batch *const ob[4], const std::vector<FriLayer> &layers, const u64 *dev_idx,
                  u64 *dev_q, size_t stride, size_t qsec) {
    size_t off = 0;
    for (int b = 0; b < 4; b++) GLP_TRY(queries_oracle(c, g, ob[b], b == 0, dev_idx, dev_q, stride, qsec, off));
    GLP_TRY(queries_layers(c, g, layers, dev_idx, dev_q, stride, qsec, off));
    if (off != stride) return set_error(GLP_ERR_ARG, "internal: query record layout mismatch");
    return GLP_OK;
}

// what both glp_prove_batch drivers require of a batch
int batch_check(const ProveGeo &g) {
    GLP_REQUIRE(g.nch == 2, "glp_prove_batch: num_challenges = %u (the batch path evaluates the quotient with the two-challenge kernels)", g.nch);
    GLP_REQUIRE(g.K >= 1 && g.K <= 4096, "glp_prove_batch: batch of %u proofs outside 1..4096", g.K);
    GLP_REQUIRE((size_t)g.K * g.nw * g.N * 8 <= ((size_t)64 << 30), "glp_prove_batch: batch too large (K * num_wires * 2^(degree_bits + rate_bits) words)");
    return GLP_OK;
}
// GLP_BATCH_TRACE: wall time since the previous mark, the stream drained first, one line per step on stderr
struct BatchTrace {
    glp_ctx *c;
    u32 K;
    const char *tag;           // "" or " dev": which driver
    const bool on = getenv("GLP_BATCH_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    BatchTrace(glp_ctx *ctx, u32 K_, const char *tag_) : c(ctx), K(K_), tag(tag_) {}
    void operator()(const char *what) {
        if (!on) return;
        (void)hipStreamSynchronize(c->stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[glp_prove_batch K=%u%s] %-28s %8.3f ms\n", K, tag, what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
};

}  // namespace
