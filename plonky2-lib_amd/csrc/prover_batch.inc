// prover_batch.inc -- many independent proofs of ONE circuit per launch (BASELINE config 5: a batch of zkdsa
// simple-signature proofs [REF src/zkdsa/circuits/mod.rs:24-43,322-339]).  Included at the end of prover.hip.
//
// A 2^3-row proof is ~150 kernel launches and ~20 host round trips of a few microseconds of device work each: proved one
// by one, such proofs are bound by launch and synchronisation latency (2.3 k proofs/s per GPU with four host threads,
// profiles/r01_secondary_workloads.txt).  Here the K proofs advance in lock step: every device stage is ONE launch over
// all K proofs (the kernels of prover.hip / merkle.hip take a proof index in a grid dimension and per-proof strides; the
// transforms simply see K * columns independent columns), every host round trip moves the K caps / openings at once, and
// the K Fiat-Shamir transcripts between two stages run on a small pool of host threads.  Each proof is word for word the
// proof glp_prove returns for the same witness (tests/test_gpu_batch.py).
#include <chrono>
#include "host_pool.h"

namespace {

// the cap level of K trees -> host [K][capn * 4] (one strided copy)
int caps_to_host(glp_ctx *c, const u64 *dev_digests, size_t dig_stride_words, size_t cap_off_digests, u32 capn, u32 K, std::vector<u64> &out) {
    out.resize((size_t)K * capn * 4);
    GLP_HIP(hipMemcpy2DAsync(out.data(), (size_t)capn * 32, dev_digests + 4 * cap_off_digests, dig_stride_words * 8, (size_t)capn * 32, K,
                             hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

int prove_batch_impl(glp_ctx *c, const glp_circuit *cc, u32 K, const u64 *dev_wires, const u64 *public_inputs, u64 *proofs_out) {
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
    HostPool &pool = ctx_host_pool(c);       // persistent: thread start-up costs more than a small batch
    const bool trace = getenv("GLP_BATCH_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
        if (!trace) return;
        (void)hipStreamSynchronize(c->stream);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[glp_prove_batch K=%u] %-28s %8.3f ms\n", K, what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    Tmp tmp(c);
    auto P = [&](u32 k) { return proofs_out + (size_t)k * L.total; };      // every word of the layout is written below
    const int hasher = (int)d.hasher;
    std::vector<Challenger> ch(K, Challenger(hasher));
    std::vector<u64> pih((size_t)K * 4, 0), caps;
    BatchHolder wb, zb, qb;
    u64 salt_seed[4] = {0, 0, 0, 0};     // zk circuit: one seed per call, proof k salts with seed3 + k (merkle_fill_salts)
    const u64 *salt = nullptr;
    if (cc->zk) { GLP_TRY(salt_seed_draw(c, salt_seed)); salt = salt_seed; }

    // ---- wires commitment
    pool.run(K, [&](size_t k) {
        host_hash_no_pad(public_inputs + k * npi, npi, &pih[4 * k]);
        if (npi) memcpy(P((u32)k) + L.pis, public_inputs + k * npi, (size_t)npi * 8);
    });
    mark("pi hashes (host)");
    GLP_TRY(batch_build(c, dev_wires, BATCH_VALUES, nw, lg, rb, (int)d.cap_height, &wb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_WIRES));
    const size_t ndig = wb.b->ndigests, cap_off = merkle_cap_offset(N, (int)d.cap_height);
    GLP_TRY(caps_to_host(c, wb.b->digests, ndig * 4, cap_off, capn, K, caps));
    mark("wires commit + caps");
    std::vector<u64> chal((size_t)K * 2 * MAXCH, 0);
    pool.run(K, [&](size_t k) {
        memcpy(P((u32)k) + L.caps, &caps[k * capn * 4], (size_t)capn * 32);
        ch[k].observe_hashes(cc->digest, 1);
        ch[k].observe(&pih[4 * k], 4);
        ch[k].observe_hashes(&caps[k * capn * 4], capn);
        for (u32 i = 0; i < nch; i++) chal[k * 2 * MAXCH + i] = ch[k].get();
        for (u32 i = 0; i < nch; i++) chal[k * 2 * MAXCH + MAXCH + i] = ch[k].get();
    });

    mark("transcript 1 (host)");
    // ---- partial products + Z, commitment
    u64 *dev_chal, *zp, *dens, *tot;
    const u32 nblocks = nblk(n);
    GLP_TRY(tmp.get(&dev_chal, chal.size()));
    GLP_TRY(h2d(c, dev_chal, chal.data(), chal.size() * 8));
    GLP_TRY(tmp.get(&zp, (size_t)K * nzp * n));
    GLP_TRY(tmp.get(&dens, (size_t)K * nzp * n));
    GLP_TRY(tmp.get(&tot, (size_t)K * nch * nblocks));
    {
        PPArgs a;
        a.wires = dev_wires; a.sigmas = cc->dev_sigmas; a.k_is = cc->dev_k_is; a.zp = zp; a.dens = dens;
        for (int i = 0; i < MAXCH; i++) a.betas[i] = a.gammas[i] = 0;
        a.w_n = root_of_unity(lg); a.lg = (u32)lg; a.nr = nr; a.nch = nch; a.npp = npp; a.qdf = qdf;
        a.chal = dev_chal; a.wires_stride = (size_t)nw * n; a.zp_stride = (size_t)nzp * n;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pp_rows<2>), dim3(nblocks, K), dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pp_block_tot, dim3(nblocks, nch, K), dim3(256), 0, c->stream, zp, tot, (u32)lg, nblocks, a.zp_stride);
        hipLaunchKernelGGL(k_pp_scan_tot, dim3(nch, K), dim3(256), 0, c->stream, tot, nblocks);
        hipLaunchKernelGGL(k_pp_apply, dim3(nblocks, nch, K), dim3(256), 0, c->stream, zp, tot, (u32)lg, nblocks, nch, npp, a.zp_stride);
        GLP_HIP(hipGetLastError());
    }
    GLP_TRY(batch_build(c, zp, BATCH_VALUES, nzp, lg, rb, (int)d.cap_height, &zb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_ZS));
    GLP_TRY(caps_to_host(c, zb.b->digests, ndig * 4, cap_off, capn, K, caps));

    mark("partial products + commit");
    // ---- quotient
    int qdb = 0;
    while ((1u << qdb) < qdf) qdb++;
    const u32 Rq = 1u << qdb, step = 1u << (rb - qdb);
    const u32 nchunks = npp + 1, nterms = nch + nch * nchunks + d.num_gate_constraints;
    const size_t apn = (size_t)nch * nterms;            // per proof: apn whole powers; the limb forms (APL_WORDS words each) follow all of them
    std::vector<u64> apow((size_t)(1 + APL_WORDS) * K * apn), qpp((size_t)K * 3 * MAXCH, 0);
    pool.run(K, [&](size_t k) {
        memcpy(P((u32)k) + L.caps + capn * 4, &caps[k * capn * 4], (size_t)capn * 32);
        ch[k].observe_hashes(&caps[k * capn * 4], capn);
        for (u32 i = 0; i < nch; i++) {
            const u64 alpha = ch[k].get();
            u64 x = 1;
            for (u32 t = 0; t < nterms; t++) {
                const size_t e = (k * nch + i) * nterms + t;
                apow[e] = x;
                apl_words(x, &apow[(size_t)K * apn + APL_WORDS * e]);
                x = mul(x, alpha);
            }
        }
        for (u32 i = 0; i < nch; i++) { qpp[k * 3 * MAXCH + i] = chal[k * 2 * MAXCH + i]; qpp[k * 3 * MAXCH + MAXCH + i] = chal[k * 2 * MAXCH + MAXCH + i]; }
        memcpy(&qpp[k * 3 * MAXCH + 2 * MAXCH], &pih[4 * k], 32);
    });
    mark("transcript 2 + alpha powers (host)");
    u64 *dev_apow, *dev_qpp, *qv, *qV, *qc, *l0t;
    GLP_TRY(tmp.get(&dev_apow, apow.size()));
    GLP_TRY(h2d(c, dev_apow, apow.data(), apow.size() * 8));
    GLP_TRY(tmp.get(&dev_qpp, qpp.size()));
    GLP_TRY(h2d(c, dev_qpp, qpp.data(), qpp.size() * 8));
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
        const dim3 g(nblk(n), Rq, K);
        if (cc->light_count || cc->arith_ops) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<2, 2>), g, dim3(256), 0, c->stream, a, qp, qbt, lg_);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient<2, 0>), g, dim3(256), 0, c->stream, a, qp, qbt, lg_);
        GLP_HIP(hipGetLastError());
        if (cc->limb_count) {
            LimbArgs la;
            limb_args(cc, la);
            la.extra_count = cc->limb_extra_count;
            for (int i = 0; i < 4; i++) la.extra_gi[i] = cc->limb_extra_gi[i];
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient_limbs<2>), g, dim3(256), 0, c->stream, a, qp, qbt, la);
            GLP_HIP(hipGetLastError());
        }
        for (u32 gi : cc->single_gates) {
#define GLP_GATE_LAUNCH(T) case T: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_quotient_gate<2, T>), g, dim3(256), 0, c->stream, a, qp, qbt, gi); break;
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
        hipLaunchKernelGGL(k_quotient_combine, dim3(nblk(n), K * nch), dim3(256), 0, c->stream, q);     // [K][nch] channels, contiguous
        GLP_HIP(hipGetLastError());
    }
    GLP_TRY(batch_build(c, qc, BATCH_COEFFS_BITREV, nch * qdf, lg, rb, (int)d.cap_height, &qb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_QUOTIENT));
    GLP_TRY(caps_to_host(c, qb.b->digests, ndig * 4, cap_off, capn, K, caps));

    mark("quotient + commit");
    // ---- openings
    std::vector<u64> zetas((size_t)K * 4);            // zeta, zeta_next per proof
    std::vector<int> err(K, 0);
    const u64 wn = root_of_unity(lg);
    pool.run(K, [&](size_t k) {
        memcpy(P((u32)k) + L.caps + 2 * capn * 4, &caps[k * capn * 4], (size_t)capn * 32);
        ch[k].observe_hashes(&caps[k * capn * 4], capn);
        const ext2 zeta = ch[k].get_ext();
        ext2 zp2 = zeta;
        for (int i = 0; i < lg; i++) zp2 = e_sqr(zp2);
        if (e_eq(zp2, e_from(1))) err[k] = 1;
        const ext2 zn = e_scale(zeta, wn);
        zetas[4 * k] = zeta.a; zetas[4 * k + 1] = zeta.b; zetas[4 * k + 2] = zn.a; zetas[4 * k + 3] = zn.b;
    });
    for (u32 k = 0; k < K; k++) if (err[k]) return set_error(GLP_ERR_PROVE, "Opening point is in the subgroup. (proof %u of the batch)", k);
    mark("transcript 3 (host)");
    const glp_batch *ob[4] = {cc->cs, wb.b, zb.b, qb.b};
    const size_t ostride[4] = {0, 1, 1, 1};            // the constants/sigmas oracle is shared by all proofs
    u64 *dev_zetas, *zt, *partial;
    GLP_TRY(tmp.get(&dev_zetas, zetas.size()));
    GLP_TRY(h2d(c, dev_zetas, zetas.data(), zetas.size() * 8));
    GLP_TRY(tmp.get(&zt, (size_t)K * 2 * n));
    const u32 nob = open_blocks(n);
    size_t poff[6] = {0, 0, 0, 0, 0, 0};                // per proof, in partial-sum words
    for (int b = 0; b < 5; b++) poff[b + 1] = poff[b] + (size_t)(b < 4 ? ob[b]->ncols : nch) * nob * 2;     // at g zeta: only the Z columns
    GLP_TRY(tmp.get(&partial, (size_t)K * poff[5]));
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
                           bstride * b->ncols * n, (size_t)2 * n, poff[5]);
        GLP_HIP(hipGetLastError());
        return GLP_OK;
    };
    GLP_TRY(zeta_tables(0));
    for (int b = 0; b < 4; b++) GLP_TRY(open_launch(ob[b], ostride[b], poff[b], ob[b]->ncols));
    GLP_TRY(zeta_tables(1));
    GLP_TRY(open_launch(zb.b, 1, poff[4], nch));
    std::vector<u64> hp((size_t)K * poff[5]);
    GLP_TRY(d2h(c, hp.data(), partial, hp.size() * 8));
    mark("openings (device + copy)");
    size_t total_cols = 0;
    for (int b = 0; b < 4; b++) total_cols += ob[b]->ncols;
    std::vector<u64> fap((size_t)K * 2 * total_cols), fpp((size_t)K * 10);
    pool.run(K, [&](size_t k) {
        const u64 *h = hp.data() + k * poff[5];
        std::vector<ext2> open[4], all;
        for (int b = 0; b < 4; b++) open_batch_finish(h + poff[b], ob[b]->ncols, nob, open[b]);
        open_batch_finish(h + poff[4], nch, nob, all);
        u64 *op = P((u32)k) + L.openings;
        size_t o = 0;
        auto put = [&](ext2 e) { op[o++] = e.a; op[o++] = e.b; };
        for (u32 i = 0; i < nc + nr; i++) put(open[0][i]);
        for (u32 i = 0; i < nw; i++) put(open[1][i]);
        for (u32 i = 0; i < nch; i++) put(open[2][i]);
        for (u32 i = 0; i < nch; i++) put(all[i]);
        for (u32 i = 0; i < nch * npp; i++) put(open[2][nch + i]);
        for (u32 i = 0; i < nch * qdf; i++) put(open[3][i]);
        const u64 *p_cs = op, *p_w = op + 2 * (nc + nr), *p_zs = p_w + 2 * nw, *p_zn = p_zs + 2 * nch;
        const u64 *p_pp = p_zn + 2 * nch, *p_q = p_pp + 2 * nch * npp;
        ch[k].observe(p_cs, 2 * (nc + nr)); ch[k].observe(p_w, 2 * nw); ch[k].observe(p_zs, 2 * nch);
        ch[k].observe(p_pp, 2 * (size_t)nch * npp); ch[k].observe(p_q, 2 * (size_t)nch * qdf); ch[k].observe(p_zn, 2 * nch);
        // FRI batch polynomial: alpha powers over all columns, the two reduced openings
        const ext2 alpha = ch[k].get_ext();
        u64 *ap = &fap[k * 2 * total_cols];
        ext2 x = e_from(1), red0 = e_from(0), red1 = e_from(0);
        size_t j = 0;
        for (int b = 0; b < 4; b++)
            for (u32 col = 0; col < ob[b]->ncols; col++, j++) {
                ap[2 * j] = x.a; ap[2 * j + 1] = x.b;
                red0 = e_add(red0, e_mul(x, open[b][col]));
                x = e_mul(x, alpha);
            }
        x = e_from(1);
        for (u32 col = 0; col < nch; col++) { red1 = e_add(red1, e_mul(x, all[col])); x = e_mul(x, alpha); }
        const ext2 sa = e_pow(alpha, nch);
        u64 *v = &fpp[k * 10];
        v[0] = red0.a; v[1] = red0.b; v[2] = red1.a; v[3] = red1.b;
        v[4] = zetas[4 * k]; v[5] = zetas[4 * k + 1]; v[6] = zetas[4 * k + 2]; v[7] = zetas[4 * k + 3];
        v[8] = sa.a; v[9] = sa.b;
    });

    mark("transcript 4 + fri alpha powers (host)");
    // ---- FRI: batch polynomial, commit phase
    u64 *dev_fap, *dev_fpp, *fv, *fcoef;
    GLP_TRY(tmp.get(&dev_fap, fap.size()));
    GLP_TRY(h2d(c, dev_fap, fap.data(), fap.size() * 8));
    GLP_TRY(tmp.get(&dev_fpp, fpp.size()));
    GLP_TRY(h2d(c, dev_fpp, fpp.data(), fpp.size() * 8));
    GLP_TRY(tmp.get(&fv, (size_t)K * 2 * n));
    GLP_TRY(tmp.get(&fcoef, (size_t)K * 2 * n));
    {
        FVArgs a;
        for (int b = 0; b < 4; b++) { a.lde[b] = ob[b]->lde; a.ncols[b] = ob[b]->ncols; a.lde_stride[b] = ostride[b] * (ob[b]->ncols + ob[b]->salt) * N; }
        a.apow = dev_fap; a.out = fv;
        a.red0 = a.red1 = a.zeta = a.zeta_next = a.shift_acc = e_from(0);
        a.w_n = wn; a.g = GEN; a.lg = (u32)lg; a.rb = (u32)rb; a.nch = nch;
        a.pp = dev_fpp; a.apow_stride = 2 * total_cols; a.out_stride = 2 * n;
        hipLaunchKernelGGL(k_final_values, dim3(nblk(n), K), dim3(256), 0, c->stream, a);
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
    std::vector<u64> betas_h((size_t)K * 2);
    for (u32 r = 0; r < nred; r++) {
        const u32 ab = d.reduction_arity_bits[r], lgL = (u32)(lgcur + rb);
        const size_t Lsz = (size_t)1 << lgL, nleaves = Lsz >> ab;
        BLayer ly;
        ly.lgL = lgL; ly.ab = ab; ly.ndig = merkle_num_digests(nleaves, (int)d.cap_height);
        GLP_TRY(tmp.get(&ly.vals, (size_t)K * 2 * Lsz));
        GLP_TRY(tmp.get(&ly.dig, (size_t)K * ly.ndig * 4));
        GLP_TRY(lde_coeffs(c, cur, ly.vals, 2 * K, lgcur, rb, shift));
        if (hasher == GLP_HASH_KECCAK25)
            hipLaunchKernelGGL(k_fri_leaf_hash_keccak, dim3(nblk(nleaves), K), dim3(256), 0, c->stream, ly.vals, ly.dig, lgL, (u32)rb, ab, 2 * Lsz,
                               ly.ndig * 4);
        else if (nleaves * K <= c->merkle_coop_max)
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
        GLP_TRY(caps_to_host(c, ly.dig, ly.ndig * 4, merkle_cap_offset(nleaves, (int)d.cap_height), capn, K, caps));
        pool.run(K, [&](size_t k) {
            memcpy(P((u32)k) + L.fri_caps + (size_t)r * capn * 4, &caps[k * capn * 4], (size_t)capn * 32);
            ch[k].observe_hashes(&caps[k * capn * 4], capn);
            const ext2 beta = ch[k].get_ext();
            betas_h[2 * k] = beta.a; betas_h[2 * k + 1] = beta.b;
        });
        GLP_TRY(h2d(c, dev_betas, betas_h.data(), betas_h.size() * 8));
        u64 *nxt;
        const size_t nnew = ((size_t)1 << lgcur) >> ab;
        GLP_TRY(tmp.get(&nxt, (size_t)K * 2 * nnew));
        hipLaunchKernelGGL(k_fri_fold, dim3(nblk(nnew), K), dim3(256), 0, c->stream, cur, nxt, e_from(0), (u32)lgcur, ab, (const u64 *)dev_betas);
        GLP_HIP(hipGetLastError());
        cur = nxt; lgcur -= (int)ab;
        shift = pow(shift, (u64)1 << ab);
        layers.push_back(ly);
    }
    mark("fri combine + layers");
    const size_t fl = (size_t)1 << lgcur;
    if (fl != L.final_len) return set_error(GLP_ERR_ARG, "reduction_arity_bits inconsistent with degree_bits");
    std::vector<u64> fh((size_t)K * 2 * fl);
    GLP_TRY(d2h(c, fh.data(), cur, fh.size() * 8));

    // ---- proof of work: every proof's sponge (state + pending inputs), one persistent launch
    std::vector<u64> pst((size_t)K * 12);
    std::vector<u32> ppos(K);
    pool.run(K, [&](size_t k) {
        u64 *pf = P((u32)k) + L.final_poly;
        const u64 *h = &fh[k * 2 * fl];
        for (size_t p = 0; p < fl; p++) {
            const size_t kk = bitrev32((u32)p, lgcur);
            pf[2 * kk] = h[p]; pf[2 * kk + 1] = h[fl + p];
        }
        ch[k].observe(pf, 2 * L.final_len);
        memcpy(&pst[k * 12], ch[k].st, 96);
        for (int i = 0; i < ch[k].nin; i++) pst[k * 12 + i] = ch[k].in[i];
        ppos[k] = (u32)ch[k].nin;
    });
    for (u32 k = 0; k < K; k++) GLP_REQUIRE(ppos[k] < 8, "proof of work: %u pending inputs (the rate is 8)", ppos[k]);
    mark("final poly + transcript 5 (host)");
    u64 *dev_pst, *dev_best, *dev_ppos, *dev_next;
    GLP_TRY(tmp.get(&dev_pst, pst.size()));
    GLP_TRY(tmp.get(&dev_best, K));
    GLP_TRY(tmp.get(&dev_next, K));
    GLP_HIP(hipMemsetAsync(dev_next, 0, (size_t)K * 8, c->stream));
    GLP_TRY(tmp.get(&dev_ppos, (K + 1) / 2));
    GLP_TRY(h2d(c, dev_pst, pst.data(), pst.size() * 8));
    GLP_TRY(h2d(c, dev_ppos, ppos.data(), (size_t)K * 4));
    std::vector<u64> best(K, ~0ull);
    GLP_TRY(h2d(c, dev_best, best.data(), (size_t)K * 8));
    {
        // persistent workgroups, a few per CU; each walks the proofs until none has candidates left below its witness
        if (hasher == GLP_HASH_KECCAK25)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pow_batch<GLP_HASH_KECCAK25>), dim3((unsigned)c->num_cus * 8), dim3(256), 0, c->stream, dev_pst,
                               (const u32 *)dev_ppos, d.proof_of_work_bits, (unsigned long long *)dev_best, (unsigned long long *)dev_next, K);
        else
            GLP_TRY(pow_batch_launch(c, tmp, dev_pst, (const u32 *)dev_ppos, d.proof_of_work_bits, dev_best, dev_next, K));
        GLP_HIP(hipGetLastError());
    }
    GLP_TRY(d2h(c, best.data(), dev_best, (size_t)K * 8));
    mark("proof of work");
    std::vector<u64> xi((size_t)K * nq);
    std::fill(err.begin(), err.end(), 0);
    pool.run(K, [&](size_t k) {
        if (best[k] == ~0ull) { err[k] = 1; return; }
        P((u32)k)[L.pow] = best[k];
        ch[k].observe(&best[k], 1);
        const u64 resp = ch[k].get();
        if (d.proof_of_work_bits && (resp >> (64 - d.proof_of_work_bits)) != 0) { err[k] = 2; return; }
        for (u32 q = 0; q < nq; q++) xi[k * nq + q] = ch[k].get() % (u64)N;
    });
    for (u32 k = 0; k < K; k++) {
        if (err[k] == 1) return set_error(GLP_ERR_PROVE, "Proof of work failed. This is highly unlikely! (proof %u of the batch)", k);
        if (err[k] == 2) return set_error(GLP_ERR_PROVE, "proof-of-work response check failed (proof %u of the batch)", k);
    }

    mark("transcript 6 (host)");
    // ---- query phase: every gather writes into a device image of the K query sections
    u64 *dev_idx, *dev_q;
    const size_t stride = L.query_stride, qsec = (size_t)nq * stride;
    GLP_TRY(tmp.get(&dev_idx, xi.size()));
    GLP_TRY(tmp.get(&dev_q, (size_t)K * qsec));
    GLP_TRY(h2d(c, dev_idx, xi.data(), xi.size() * 8));
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
    // one strided copy puts every proof's query section in its place
    GLP_HIP(hipMemcpy2DAsync(proofs_out + L.queries, L.total * 8, dev_q, qsec * 8, qsec * 8, K, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    mark("queries");
    return GLP_OK;
}

}  // namespace

