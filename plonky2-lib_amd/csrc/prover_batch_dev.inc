// prover_batch_dev.inc -- glp_prove_batch with the Fiat-Shamir transcripts ON THE DEVICE (PoseidonGoldilocksConfig).
// Included at the end of prover.hip, after prover_batch.inc (whose host-transcript path stays for KeccakGoldilocksConfig and as
// the A/B reference: GLP_BATCH_HOST_TRANSCRIPT=1).
//
// prover_batch.inc advances K proofs in lock step but returns to the host between every two device stages: copy K caps (or
// openings) back, run K transcripts on host threads, upload K challenges -- seven round trips plus one per FRI reduction, ~4 ms
// of a 14 ms batch of 256 zkdsa proofs [REF src/zkdsa/circuits/mod.rs:322-339 proves them one by one], and a rate that depends on
// the box's host cores.  Here each of those steps is ONE small kernel over the K proofs: a 16-lane group per proof keeps the duplex
// sponge of plonky2's `Challenger` (iop/challenger.rs; overwrite mode, challenges popped from the end of the rate) on 12 lanes
// (poseidon.h permute_coop), observes what the previous device stage left in HBM, and writes the challenges where the next stage
// reads them.  Caps, openings, final polynomial, proof-of-work witness and query records go straight into a device image of the
// K proofs; ONE copy brings the batch back.  The host only enqueues launches.
#include "transcript_dev.h"
namespace {

int prove_batch_impl_dev(glp_ctx *c, const glp_circuit *cc, u32 K, const u64 *dev_wires, const u64 *public_inputs, u64 *proofs_out) {
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const int lg = (int)d.degree_bits, rb = (int)d.rate_bits;
    const size_t n = (size_t)1 << lg, N = n << rb;
    const u32 nch = d.num_challenges, nr = d.num_routed_wires, nw = d.num_wires, nc = d.num_constants, qdf = d.quotient_degree_factor;
    const u32 npp = d.num_partial_products, capn = 1u << d.cap_height, nzp = nch * (1 + npp), npi = d.num_public_inputs;
    const u32 nred = d.num_reductions, nq = d.num_query_rounds;
    GLP_REQUIRE(nch == 2, "glp_prove_batch: num_challenges = %u (the batch path evaluates the quotient with the two-challenge kernels)", nch);
    GLP_REQUIRE(K >= 1 && K <= 4096, "glp_prove_batch: batch of %u proofs outside 1..4096", K);
    GLP_REQUIRE((size_t)K * nw * N * 8 <= ((size_t)64 << 30), "glp_prove_batch: batch too large (K * num_wires * 2^(degree_bits + rate_bits) words)");
    const bool trace = getenv("GLP_BATCH_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
        if (!trace) return;
        (void)hipStreamSynchronize(c->stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[glp_prove_batch K=%u dev] %-28s %8.3f ms\n", K, what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    Tmp tmp(c);
    const int hasher = (int)d.hasher;
    BatchHolder wb, zb, qb;
    u64 salt_seed[4] = {0, 0, 0, 0};     // zk circuit: one seed per call, proof k salts with seed3 + k (merkle_fill_salts)
    const u64 *salt = nullptr;
    if (cc->zk) { GLP_TRY(salt_seed_draw(c, salt_seed)); salt = salt_seed; }
    const unsigned tgrid = (K + 15) / 16;
    u64 *dch, *image;
    u32 *dev_err;
    GLP_TRY(tmp.get(&dch, (size_t)K * DCH_WORDS));
    GLP_TRY(tmp.get(&image, (size_t)K * L.total));
    { u64 *e; GLP_TRY(tmp.get(&e, (K + 1) / 2 + 1)); dev_err = (u32 *)e; }
    GLP_HIP(hipMemsetAsync(dev_err, 0, (size_t)K * 4, c->stream));
    if (npi) GLP_HIP(hipMemcpy2DAsync(image + L.pis, L.total * 8, public_inputs, (size_t)npi * 8, (size_t)npi * 8, K, hipMemcpyHostToDevice, c->stream));
    TrGeo g;
    g.dch = dch; g.image = image; g.total = L.total; g.K = K; g.capn = capn; g.nch = nch;

    // ---- wires commitment, transcript 1
    GLP_TRY(batch_build(c, dev_wires, BATCH_VALUES, nw, lg, rb, (int)d.cap_height, &wb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_WIRES));
    const size_t ndig = wb.b->ndigests, cap_off = merkle_cap_offset(N, (int)d.cap_height);
    u64 *dev_chal, *dev_qpp;
    GLP_TRY(tmp.get(&dev_chal, (size_t)K * 2 * MAXCH));
    GLP_TRY(tmp.get(&dev_qpp, (size_t)K * 3 * MAXCH));
    GLP_HIP(hipMemsetAsync(dev_chal, 0, (size_t)K * 2 * MAXCH * 8, c->stream));
    GLP_HIP(hipMemsetAsync(dev_qpp, 0, (size_t)K * 3 * MAXCH * 8, c->stream));
    hipLaunchKernelGGL(k_tr_begin, dim3(tgrid), dim3(256), 0, c->stream, g, cc->digest[0], cc->digest[1], cc->digest[2], cc->digest[3], L.pis, npi,
                       wb.b->digests + 4 * cap_off, ndig * 4, L.caps, dev_chal, dev_qpp);
    GLP_HIP(hipGetLastError());
    mark("wires commit + transcript 1");

    // ---- partial products + Z, commitment, transcript 2 (alphas and their powers)
    u64 *zp, *dens, *tot;
    const u32 nblocks = nblk(n);
    GLP_TRY(tmp.get(&zp, (size_t)K * nzp * n));
    GLP_TRY(tmp.get(&dens, (size_t)K * nzp * n));
    GLP_TRY(tmp.get(&tot, (size_t)K * nch * nblocks));
    {
        PPArgs a;
        a.wires = dev_wires; a.sigmas = cc->dev_sigmas; a.k_is = cc->dev_k_is; a.zp = zp; a.dens = dens;
        for (int i = 0; i < MAXCH; i++) a.betas[i] = a.gammas[i] = 0;
        a.w_n = root_of_unity(lg); a.lg = (u32)lg; a.nr = nr; a.nch = nch; a.npp = npp; a.qdf = qdf;
        a.chal = dev_chal; a.wires_stride = (size_t)nw * n; a.zp_stride = (size_t)nzp * n;
        const size_t small_lds = (size_t)2 * nch * (npp + 2) * n * sizeof(u64);
        if (lg <= 7 && small_lds <= 64 * 1024) {     // at most 128 rows: (row, chunk, challenge) per lane, one workgroup per proof; the running product too
            hipLaunchKernelGGL(k_pp_rows_small, dim3(1, K), dim3(256), small_lds, c->stream, a);
        } else {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pp_rows<2>), dim3(nblocks, K), dim3(256), 0, c->stream, a);
            GLP_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_pp_block_tot, dim3(nblocks, nch, K), dim3(256), 0, c->stream, zp, tot, (u32)lg, nblocks, a.zp_stride);
            hipLaunchKernelGGL(k_pp_scan_tot, dim3(nch, K), dim3(256), 0, c->stream, tot, nblocks);
            hipLaunchKernelGGL(k_pp_apply, dim3(nblocks, nch, K), dim3(256), 0, c->stream, zp, tot, (u32)lg, nblocks, nch, npp, a.zp_stride);
        }
        GLP_HIP(hipGetLastError());
    }
    GLP_TRY(batch_build(c, zp, BATCH_VALUES, nzp, lg, rb, (int)d.cap_height, &zb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_ZS));
    int qdb = 0;
    while ((1u << qdb) < qdf) qdb++;
    const u32 Rq = 1u << qdb, step = 1u << (rb - qdb);
    const u32 nchunks = npp + 1, nterms = nch + nch * nchunks + d.num_gate_constraints;
    const size_t apn = (size_t)nch * nterms;
    u64 *dev_apow, *qv, *qV, *qc, *l0t;
    GLP_TRY(tmp.get(&dev_apow, (size_t)(1 + APL_WORDS) * K * apn));
    hipLaunchKernelGGL(k_tr_alphas, dim3(tgrid), dim3(256), 0, c->stream, g, zb.b->digests + 4 * cap_off, ndig * 4, L.caps + (size_t)capn * 4, nterms, dev_apow,
                       dev_apow + (size_t)K * apn);
    GLP_HIP(hipGetLastError());
    mark("partial products + commit + transcript 2");

    // ---- quotient
    const size_t qstride = (size_t)nch * Rq * n;
    GLP_TRY(tmp.get(&qv, (size_t)K * qstride));
    GLP_TRY(tmp.get(&qV, (size_t)K * qstride));
    GLP_TRY(tmp.get(&qc, (size_t)K * qstride));
    GLP_TRY(tmp.get(&l0t, (size_t)Rq * n));
    const u64 gn = pow(GEN, (u64)n);
    {
        QArgs a;
        QProof qp;
        QBatch qbt;
        memset(&qp, 0, sizeof(qp));
        a.cs = cc->cs->lde; a.gates = cc->dev_gates; a.k_is = cc->dev_k_is; a.k_ratio = cc->k_ratio;
        qp.wl = wb.b->lde; qp.zl = zb.b->lde; qp.out = qv; qp.apow = dev_apow; qp.apl = dev_apow + (size_t)K * apn;
        qbt.pp = dev_qpp; qbt.wl_stride = (size_t)(nw + wb.b->salt) * N; qbt.zl_stride = (size_t)(nzp + zb.b->salt) * N; qbt.out_stride = qstride; qbt.apow_stride = (size_t)nch * nterms;
        const u64 WN = root_of_unity(lg + rb), wR = root_of_unity(rb);
        for (u32 rq = 0; rq < Rq; rq++) {
            const u32 r = rq * step;
            a.shift_r[rq] = mul(GEN, pow(WN, (u64)r));
            a.zh[rq] = sub(mul(gn, pow(wR, (u64)r)), 1);
            a.zh_inv[rq] = inv(a.zh[rq]);
        }
        a.w_n = root_of_unity(lg); a.n_field = (u64)n % glf::P;
        a.lg = (u32)lg; a.rb = (u32)rb; a.step = step; a.nc = nc; a.nsel = d.num_selectors; a.nr = nr; a.nw = nw;
        a.nch = nch; a.npp = npp; a.qdf = qdf; a.num_gates = d.num_gates; a.nterms = nterms;
        a.many_selectors = d.num_selectors > 1; a.gate_mode = 1; a.l0 = l0t;
        hipLaunchKernelGGL(k_l0_table, dim3(nblk(n)), dim3(256), 0, c->stream, a, l0t, Rq);
        GLP_HIP(hipGetLastError());
        LightArgs lg_;
        lg_.count = cc->light_count; lg_.arith_gi = cc->arith_gi; lg_.arith_ops = cc->arith_ops;
        for (u32 i = 0; i < 8; i++) lg_.gi[i] = cc->light_gi[i];
        const dim3 gq(nblk(n), Rq, K);
        if (cc->light_count || cc->arith_ops) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<2, 2>), gq, dim3(256), 0, c->stream, a, qp, qbt, lg_);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<2, 0>), gq, dim3(256), 0, c->stream, a, qp, qbt, lg_);
        GLP_HIP(hipGetLastError());
        if (cc->limb_count) {
            LimbArgs la;
            limb_args(cc, la);
            la.extra_count = cc->limb_extra_count;
            for (int i = 0; i < 4; i++) la.extra_gi[i] = cc->limb_extra_gi[i];
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient_limbs<2>), gq, dim3(256), 0, c->stream, a, qp, qbt, la);
            GLP_HIP(hipGetLastError());
        }
        for (u32 gi : cc->single_gates) {
#define GLP_GATE_LAUNCH(T) case T: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient_gate<2, T>), gq, dim3(256), 0, c->stream, a, qp, qbt, gi); break;
            switch (cc->gates[gi].type) {
                GLP_GATE_LAUNCH(GLP_GATE_CONSTANT) GLP_GATE_LAUNCH(GLP_GATE_PUBLIC_INPUT) GLP_GATE_LAUNCH(GLP_GATE_ARITHMETIC)
                GLP_GATE_LAUNCH(GLP_GATE_POSEIDON) GLP_GATE_LAUNCH(GLP_GATE_U32_INTERLEAVE) GLP_GATE_LAUNCH(GLP_GATE_UNINTERLEAVE_U32)
                GLP_GATE_LAUNCH(GLP_GATE_UNINTERLEAVE_B32) GLP_GATE_LAUNCH(GLP_GATE_U32_ARITHMETIC) GLP_GATE_LAUNCH(GLP_GATE_U32_ADD_MANY)
                GLP_GATE_LAUNCH(GLP_GATE_U32_SUBTRACTION) GLP_GATE_LAUNCH(GLP_GATE_U32_RANGE_CHECK) GLP_GATE_LAUNCH(GLP_GATE_COMPARISON)
                GLP_GATE_LAUNCH(GLP_GATE_BASE_SUM) GLP_GATE_LAUNCH(GLP_GATE_RANDOM_ACCESS)
                GLP_GATE_LAUNCH(GLP_GATE_ARITHMETIC_EXTENSION) GLP_GATE_LAUNCH(GLP_GATE_MUL_EXTENSION)
                GLP_GATE_LAUNCH(GLP_GATE_REDUCING) GLP_GATE_LAUNCH(GLP_GATE_REDUCING_EXTENSION)
            default: break;
            }
#undef GLP_GATE_LAUNCH
            GLP_HIP(hipGetLastError());
        }
    }
    {
        GLP_TRY(intt_values_to_coeffs(c, qv, qV, K * nch * Rq, lg));
        QCArgs q;
        q.V = qV; q.out = qc; q.lg = (u32)lg; q.Rq = Rq;
        q.wM_inv = inv(root_of_unity(lg + qdb)); q.wR_inv = inv(root_of_unity(qdb)); q.g_inv = inv(GEN);
        q.rq_inv = inv((u64)Rq);
        const u64 gni = inv(gn);
        u64 x = 1;
        for (u32 cidx = 0; cidx < Rq; cidx++) { q.gn_inv_pow[cidx] = x; x = mul(x, gni); }
        hipLaunchKernelGGL(k_quotient_combine, dim3(nblk(n), K * nch), dim3(256), 0, c->stream, q);
        GLP_HIP(hipGetLastError());
    }
    GLP_TRY(batch_build(c, qc, BATCH_COEFFS_BITREV, nch * qdf, lg, rb, (int)d.cap_height, &qb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_QUOTIENT));
    const u64 wn = root_of_unity(lg);
    u64 *dev_zetas;
    GLP_TRY(tmp.get(&dev_zetas, (size_t)K * 4));
    hipLaunchKernelGGL(k_tr_zeta, dim3(tgrid), dim3(256), 0, c->stream, g, qb.b->digests + 4 * cap_off, ndig * 4, L.caps + 2 * (size_t)capn * 4, (u32)lg, wn, dev_zetas,
                       dev_err);
    GLP_HIP(hipGetLastError());
    mark("quotient + commit + transcript 3");

    // ---- openings
    const glp_batch *ob[4] = {cc->cs, wb.b, zb.b, qb.b};
    const size_t ostride[4] = {0, 1, 1, 1};            // the constants/sigmas oracle is shared by all proofs
    u64 *zt, *partial;
    GLP_TRY(tmp.get(&zt, (size_t)K * 2 * n));
    const u32 nob = open_blocks(n);
    OpenGeo og;
    og.poff[0] = 0;
    for (int b = 0; b < 5; b++) og.poff[b + 1] = og.poff[b] + (size_t)(b < 4 ? ob[b]->ncols : nch) * nob * 2;     // at g zeta: only the Z columns
    for (int b = 0; b < 4; b++) og.cols[b] = ob[b]->ncols;
    og.openings_off = L.openings; og.nob = nob; og.nch = nch; og.npp = npp; og.nopen = (u32)L.nopen;
    GLP_TRY(tmp.get(&partial, (size_t)K * og.poff[5]));
    auto zeta_tables = [&](size_t which) -> int {
        ZTArgs za;
        za.zt = zt; za.lg = (u32)lg; za.zeta_b = dev_zetas + 2 * which; za.zeta_stride = 4;
        for (int b = 0; b < 24; b++) za.zp2[b] = e_from(0);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_zeta_table<true>), dim3(nblk(n), K), dim3(256), 0, c->stream, za);
        GLP_HIP(hipGetLastError());
        return GLP_OK;
    };
    auto open_launch = [&](const glp_batch *b, size_t bstride, size_t off, u32 cols) -> int {
        hipLaunchKernelGGL(k_open_dot, dim3(nob, cols, K), dim3(256), 0, c->stream, b->coeffs, zt, partial + off, (u32)lg,
                           bstride * b->ncols * n, (size_t)2 * n, og.poff[5]);
        GLP_HIP(hipGetLastError());
        return GLP_OK;
    };
    GLP_TRY(zeta_tables(0));
    for (int b = 0; b < 4; b++) GLP_TRY(open_launch(ob[b], ostride[b], og.poff[b], ob[b]->ncols));
    GLP_TRY(zeta_tables(1));
    GLP_TRY(open_launch(zb.b, 1, og.poff[4], nch));
    hipLaunchKernelGGL(k_open_reduce, dim3(nblk((size_t)K * L.nopen)), dim3(256), 0, c->stream, g, og, partial);
    GLP_HIP(hipGetLastError());
    size_t total_cols = 0;
    for (int b = 0; b < 4; b++) total_cols += ob[b]->ncols;
    u64 *dev_fap, *dev_fpp, *fv, *fcoef;
    GLP_TRY(tmp.get(&dev_fap, (size_t)K * 2 * total_cols));
    GLP_TRY(tmp.get(&dev_fpp, (size_t)K * 10));
    hipLaunchKernelGGL(k_tr_fri_alpha, dim3(tgrid), dim3(256), 0, c->stream, g, og, dev_zetas, dev_fap, dev_fpp);
    GLP_HIP(hipGetLastError());
    mark("openings + transcript 4");

    // ---- FRI: batch polynomial, commit phase
    GLP_TRY(tmp.get(&fv, (size_t)K * 2 * n));
    GLP_TRY(tmp.get(&fcoef, (size_t)K * 2 * n));
    {
        FVArgs a;
        for (int b = 0; b < 4; b++) { a.lde[b] = ob[b]->lde; a.ncols[b] = ob[b]->ncols; a.lde_stride[b] = ostride[b] * (ob[b]->ncols + ob[b]->salt) * N; }
        a.apow = dev_fap; a.out = fv;
        a.red0 = a.red1 = a.zeta = a.zeta_next = a.shift_acc = e_from(0);
        a.w_n = wn; a.g = GEN; a.lg = (u32)lg; a.rb = (u32)rb; a.nch = nch;
        a.pp = dev_fpp; a.apow_stride = 2 * total_cols; a.out_stride = 2 * n;
        if (lg >= 2 && lg <= 7) hipLaunchKernelGGL(k_final_values_small, dim3(1, K), dim3(256), 0, c->stream, a);      // 4..128 points: 256 / n lanes per point
        else hipLaunchKernelGGL(k_final_values, dim3(nblk(n), K), dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
        GLP_TRY(intt_values_to_coeffs(c, fv, fcoef, 2 * K, lg));
        hipLaunchKernelGGL(k_scale_bitrev_pow, dim3(nblk(n), 2 * K), dim3(256), 0, c->stream, fcoef, inv(GEN), (u32)lg);
        GLP_HIP(hipGetLastError());
    }
    struct BLayer { u64 *vals, *dig; u32 lgL, ab; size_t ndig; };
    std::vector<BLayer> layers;
    u64 *cur = fcoef;
    int lgcur = lg;
    u64 shift = GEN;
    u64 *dev_betas;
    GLP_TRY(tmp.get(&dev_betas, (size_t)K * 2));
    for (u32 r = 0; r < nred; r++) {
        const u32 ab = d.reduction_arity_bits[r], lgL = (u32)(lgcur + rb);
        const size_t Lsz = (size_t)1 << lgL, nleaves = Lsz >> ab;
        BLayer ly;
        ly.lgL = lgL; ly.ab = ab; ly.ndig = merkle_num_digests(nleaves, (int)d.cap_height);
        GLP_TRY(tmp.get(&ly.vals, (size_t)K * 2 * Lsz));
        GLP_TRY(tmp.get(&ly.dig, (size_t)K * ly.ndig * 4));
        GLP_TRY(lde_coeffs(c, cur, ly.vals, 2 * K, lgcur, rb, shift));
        if (nleaves * K <= c->merkle_coop_max)
            hipLaunchKernelGGL(k_fri_leaf_hash_coop, dim3((unsigned)((nleaves + 15) / 16), K), dim3(256), 0, c->stream, ly.vals, ly.dig, lgL, (u32)rb,
                               ab, 2 * Lsz, ly.ndig * 4);
        else if (nleaves * K <= c->merkle_quad_max)
            hipLaunchKernelGGL(k_fri_leaf_hash_quad, dim3((unsigned)((nleaves + 63) / 64), K), dim3(256), 0, c->stream, ly.vals, ly.dig, lgL, (u32)rb,
                               ab, 2 * Lsz, ly.ndig * 4);
        else
            hipLaunchKernelGGL(k_fri_leaf_hash, dim3(nblk(nleaves), K), dim3(256), 0, c->stream, ly.vals, ly.dig, lgL, (u32)rb, ab, 2 * Lsz,
                               ly.ndig * 4);
        GLP_HIP(hipGetLastError());
        GLP_TRY(merkle_levels(c, ly.dig, nleaves, (int)d.cap_height, K, ly.ndig * 4, hasher));
        hipLaunchKernelGGL(k_tr_beta, dim3(tgrid), dim3(256), 0, c->stream, g, ly.dig + 4 * merkle_cap_offset(nleaves, (int)d.cap_height), ly.ndig * 4,
                           L.fri_caps + (size_t)r * capn * 4, dev_betas);
        GLP_HIP(hipGetLastError());
        u64 *nxt;
        const size_t nnew = ((size_t)1 << lgcur) >> ab;
        GLP_TRY(tmp.get(&nxt, (size_t)K * 2 * nnew));
        hipLaunchKernelGGL(k_fri_fold, dim3(nblk(nnew), K), dim3(256), 0, c->stream, cur, nxt, e_from(0), (u32)lgcur, ab, (const u64 *)dev_betas);
        GLP_HIP(hipGetLastError());
        cur = nxt; lgcur -= (int)ab;
        shift = pow(shift, (u64)1 << ab);
        layers.push_back(ly);
    }
    const size_t fl = (size_t)1 << lgcur;
    if (fl != L.final_len) return set_error(GLP_ERR_ARG, "reduction_arity_bits inconsistent with degree_bits");
    u64 *dev_pst, *dev_best, *dev_next, *dev_ppos;
    GLP_TRY(tmp.get(&dev_pst, (size_t)K * 12));
    GLP_TRY(tmp.get(&dev_best, K));
    GLP_TRY(tmp.get(&dev_next, K));
    GLP_TRY(tmp.get(&dev_ppos, (K + 1) / 2));
    GLP_HIP(hipMemsetAsync(dev_next, 0, (size_t)K * 8, c->stream));
    GLP_HIP(hipMemsetAsync(dev_best, 0xFF, (size_t)K * 8, c->stream));
    hipLaunchKernelGGL(k_tr_final, dim3(tgrid), dim3(256), 0, c->stream, g, cur, (u32)lgcur, L.final_poly, dev_pst, (u32 *)dev_ppos, dev_err);
    GLP_HIP(hipGetLastError());
    mark("fri combine + layers + transcript 5");

    // ---- proof of work: one persistent launch over the K sponges, then transcript 6 (response check, query indices)
    GLP_TRY(pow_batch_launch(c, tmp, dev_pst, (const u32 *)dev_ppos, d.proof_of_work_bits, dev_best, dev_next, K));
    u64 *dev_idx;
    GLP_TRY(tmp.get(&dev_idx, (size_t)K * nq));
    hipLaunchKernelGGL(k_tr_queries, dim3(tgrid), dim3(256), 0, c->stream, g, dev_best, d.proof_of_work_bits, L.pow, nq, (u64)N, dev_idx, dev_err);
    GLP_HIP(hipGetLastError());
    mark("proof of work + transcript 6");

    // ---- query phase: every gather writes straight into the image
    u64 *dev_q = image + L.queries;
    const size_t stride = L.query_stride, qsec = L.total;        // batch stride of the query records = one whole proof
    size_t off = 0;
    for (int b = 0; b < 4; b++) {
        const u32 ncol = ob[b]->ncols + ob[b]->salt;      // the whole leaf, salts last
        GLP_TRY(merkle_gather_lde_rows(c, ob[b]->lde, ncol, lg, rb, dev_idx, nq, dev_q + off, stride, K, ostride[b] * ncol * N, qsec));
        off += ncol;
        GLP_TRY(merkle_gather_paths(c, ob[b]->digests, N, (int)d.cap_height, dev_idx, nq, dev_q + off, stride, 0, K, ostride[b] * ndig * 4, qsec));
        off += 4 * (size_t)L.depth0;
    }
    u32 shift_bits = 0;
    for (size_t r = 0; r < layers.size(); r++) {
        const BLayer &ly = layers[r];
        const u32 arity = 1u << ly.ab;
        const size_t Lsz = (size_t)1 << ly.lgL, nleaves = Lsz >> ly.ab;
        shift_bits += ly.ab;
        hipLaunchKernelGGL(k_fri_gather_leaf, dim3(nblk((size_t)nq * arity), K), dim3(256), 0, c->stream, ly.vals, ly.lgL, (u32)rb, ly.ab, dev_idx,
                           shift_bits, nq, dev_q + off, stride, 2 * Lsz, qsec);
        GLP_HIP(hipGetLastError());
        off += 2 * (size_t)arity;
        GLP_TRY(merkle_gather_paths(c, ly.dig, nleaves, (int)d.cap_height, dev_idx, nq, dev_q + off, stride, shift_bits, K, ly.ndig * 4, qsec));
        off += 4 * (size_t)L.step_depth[r];
    }
    if (off != stride) return set_error(GLP_ERR_ARG, "internal: query record layout mismatch");
    // one copy brings the K proofs back; the error flags ride behind it
    std::vector<u32> err(K, 0);
    GLP_HIP(hipMemcpyAsync(proofs_out, image, (size_t)K * L.total * 8, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipMemcpyAsync(err.data(), dev_err, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    mark("queries + copy back");
    for (u32 k = 0; k < K; k++) {
        if (err[k] & 1u) return set_error(GLP_ERR_PROVE, "Opening point is in the subgroup. (proof %u of the batch)", k);
        if (err[k] & 2u) return set_error(GLP_ERR_ARG, "proof of work: 8 pending inputs (the rate is 8) (proof %u of the batch)", k);
        if (err[k] & 4u) return set_error(GLP_ERR_PROVE, "Proof of work failed. This is highly unlikely! (proof %u of the batch)", k);
        if (err[k] & 8u) return set_error(GLP_ERR_PROVE, "proof-of-work response check failed (proof %u of the batch)", k);
    }
    return GLP_OK;
}

}  // namespace

extern "C" int glp_prove_batch(glp_ctx *c, const glp_circuit *cc, uint32_t num_proofs, const uint64_t *wires, int wires_on_device,
                               const uint64_t *public_inputs, uint64_t *proofs_out) {
    GLP_REQUIRE(c && cc && wires && proofs_out, "null argument");
    GLP_REQUIRE(cc->ctx == c, "circuit belongs to another context");
    GLP_REQUIRE(public_inputs || cc->d.num_public_inputs == 0, "public_inputs is null");
    GLP_REQUIRE(num_proofs >= 1, "empty batch");
    GLP_TRY(bind(c));
    static const u64 no_pis = 0;
    const u64 *pis = public_inputs ? public_inputs : &no_pis;
    // transcripts on the device (PoseidonGoldilocksConfig); on host threads for KeccakGoldilocksConfig or with GLP_BATCH_HOST_TRANSCRIPT=1
    const bool dev_tr = cc->d.hasher == GLP_HASH_POSEIDON && !getenv("GLP_BATCH_HOST_TRANSCRIPT");
    auto impl = dev_tr ? prove_batch_impl_dev : prove_batch_impl;
    if (wires_on_device) return impl(c, cc, num_proofs, wires, pis, proofs_out);
    const size_t tot = (size_t)num_proofs * cc->d.num_wires << cc->d.degree_bits;
    void *dv = nullptr;
    GLP_TRY(c->alloc(&dv, tot * 8));
    int rc = h2d(c, dv, wires, tot * 8);
    if (rc == GLP_OK) rc = impl(c, cc, num_proofs, (const u64 *)dv, pis, proofs_out);
    (void)hipStreamSynchronize(c->stream);
    c->release(dv);
    return rc;
}
