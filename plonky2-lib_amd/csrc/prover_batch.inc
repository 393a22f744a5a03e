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
// This file is the driver: transcript steps, uploads and copies back.  The device stages are the functions of prover_stages.inc.
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

// K10 for K sponges at once: pst [K][12] (the pending inputs already in place), ppos [K] where the witness goes -> best [K], the smallest
// witness of each (~0: none below 2^40).  One launch (Poseidon: k_pow_prepare + k_pow_batch2), one copy back.
int pow_search_batch(glp_ctx *c, Scratch &tmp, int hasher, const std::vector<u64> &pst, const std::vector<u32> &ppos, u32 bits, std::vector<u64> &best) {
    const u32 K = (u32)ppos.size();
    u64 *dev_pst, *dev_best, *dev_ppos, *dev_next;
    GLP_TRY(tmp.words(&dev_pst, pst.size()));
    GLP_TRY(tmp.words(&dev_best, K));
    GLP_TRY(tmp.words(&dev_next, K));
    GLP_HIP(hipMemsetAsync(dev_next, 0, (size_t)K * 8, c->stream));
    GLP_TRY(tmp.words(&dev_ppos, (K + 1) / 2));
    GLP_TRY(h2d(c, dev_pst, pst.data(), pst.size() * 8));
    GLP_TRY(h2d(c, dev_ppos, ppos.data(), (size_t)K * 4));
    best.assign(K, ~0ull);
    GLP_TRY(h2d(c, dev_best, best.data(), (size_t)K * 8));
    // persistent workgroups, a few per CU; each walks the proofs until none has candidates left below its witness
    if (hasher == GLP_HASH_KECCAK25)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pow_batch<GLP_HASH_KECCAK25>), dim3((unsigned)c->num_cus * 8), dim3(256), 0, c->stream, dev_pst,
                           (const u32 *)dev_ppos, bits, (unsigned long long *)dev_best, (unsigned long long *)dev_next, K);
    else
        GLP_TRY(pow_batch_launch(c, tmp, dev_pst, (const u32 *)dev_ppos, bits, dev_best, dev_next, K));
    GLP_HIP(hipGetLastError());
    return d2h(c, best.data(), dev_best, (size_t)K * 8);
}

int prove_batch_impl(glp_ctx *c, const glp_circuit *cc, u32 K, const u64 *dev_wires, const u64 *public_inputs, u64 *proofs_out) {
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const ProveGeo g = prove_geo(cc, K);
    GLP_TRY(batch_check(g));
    const int lg = g.lg, rb = g.rb, hasher = g.hasher;
    const size_t n = g.n, N = g.N;
    const u32 nch = g.nch, nw = g.nw, qdf = g.qdf, nzp = g.nzp, capn = g.capn, nterms = g.nterms, npi = d.num_public_inputs;
    const u32 nred = d.num_reductions, nq = d.num_query_rounds;
    HostPool &pool = ctx_host_pool(c);       // persistent: thread start-up costs more than a small batch
    BatchTrace mark(c, K, "");
    Scratch tmp(c);
    auto P = [&](u32 k) { return proofs_out + (size_t)k * L.total; };      // every word of the layout is written below
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
    GLP_TRY(tmp.words(&dev_chal, chal.size()));
    GLP_TRY(h2d(c, dev_chal, chal.data(), chal.size() * 8));
    GLP_TRY(tmp.words(&zp, (size_t)K * nzp * n));
    GLP_TRY(tmp.words(&dens, (size_t)K * nzp * n));
    GLP_TRY(tmp.words(&tot, (size_t)K * nch * nblk(n)));
    GLP_TRY(stage_partial_products(c, g, dev_wires, nullptr, nullptr, dev_chal, zp, dens, tot));
    GLP_TRY(batch_build(c, zp, BATCH_VALUES, nzp, lg, rb, (int)d.cap_height, &zb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_ZS));
    GLP_TRY(caps_to_host(c, zb.b->digests, ndig * 4, cap_off, capn, K, caps));

    mark("partial products + commit");
    // ---- quotient
    const size_t apn = (size_t)nch * nterms;            // per proof: apn whole powers; the limb forms (APL_WORDS words each) follow all of them
    std::vector<u64> apow((size_t)(1 + APL_WORDS) * K * apn), qpp((size_t)K * 3 * MAXCH, 0);
    pool.run(K, [&](size_t k) {
        memcpy(P((u32)k) + L.caps + capn * 4, &caps[k * capn * 4], (size_t)capn * 32);
        ch[k].observe_hashes(&caps[k * capn * 4], capn);
        u64 alphas[MAXCH];
        for (u32 i = 0; i < nch; i++) alphas[i] = ch[k].get();
        alpha_power_table(alphas, nch, nterms, &apow[k * apn], &apow[(size_t)K * apn + APL_WORDS * k * apn]);
        for (u32 i = 0; i < nch; i++) { qpp[k * 3 * MAXCH + i] = chal[k * 2 * MAXCH + i]; qpp[k * 3 * MAXCH + MAXCH + i] = chal[k * 2 * MAXCH + MAXCH + i]; }
        memcpy(&qpp[k * 3 * MAXCH + 2 * MAXCH], &pih[4 * k], 32);
    });
    mark("transcript 2 + alpha powers (host)");
    u64 *dev_apow, *dev_qpp, *qv, *qV, *qc, *l0t;
    GLP_TRY(tmp.words(&dev_apow, apow.size()));
    GLP_TRY(h2d(c, dev_apow, apow.data(), apow.size() * 8));
    GLP_TRY(tmp.words(&dev_qpp, qpp.size()));
    GLP_TRY(h2d(c, dev_qpp, qpp.data(), qpp.size() * 8));
    const size_t qstride = (size_t)nch * g.Rq * n;
    GLP_TRY(tmp.words(&qv, (size_t)K * qstride));
    GLP_TRY(tmp.words(&qV, (size_t)K * qstride));
    GLP_TRY(tmp.words(&qc, (size_t)K * qstride));
    GLP_TRY(tmp.words(&l0t, (size_t)g.Rq * n));
    {
        QProof qp;
        QBatch qbt;
        quotient_proof_args(g, wb.b, zb.b, qv, dev_apow, dev_qpp, qp, qbt);
        GLP_TRY(stage_quotient_eval(c, g, qp, qbt, l0t));
        GLP_TRY(stage_quotient_coeffs(c, g, qv, qV, qc));
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
    u64 *dev_zetas, *zt, *partial;
    GLP_TRY(tmp.words(&dev_zetas, zetas.size()));
    GLP_TRY(h2d(c, dev_zetas, zetas.data(), zetas.size() * 8));
    GLP_TRY(tmp.words(&zt, (size_t)K * 2 * n));
    size_t poff[6];                                     // per proof, in partial-sum words
    open_offsets(g, ob, poff);
    GLP_TRY(tmp.words(&partial, (size_t)K * poff[5]));
    GLP_TRY(stage_open(c, g, ob, nullptr, dev_zetas, zt, partial, poff));
    std::vector<u64> hp((size_t)K * poff[5]);
    GLP_TRY(d2h(c, hp.data(), partial, hp.size() * 8));
    mark("openings (device + copy)");
    const size_t total_cols = oracle_cols(ob);
    std::vector<u64> fap((size_t)K * 2 * total_cols), fpp((size_t)K * 10);
    pool.run(K, [&](size_t k) {
        std::vector<ext2> open[4], zs_next;
        u64 *op = P((u32)k) + L.openings;
        openings_to_proof(g, ob, hp.data() + k * poff[5], poff, open, zs_next, op);
        observe_openings(ch[k], g, op);
        // FRI batch polynomial: alpha powers over all columns, the two reduced openings
        ext2 pt[5];
        fri_alpha_powers(g, ob, open, zs_next, ch[k].get_ext(), e_make(zetas[4 * k], zetas[4 * k + 1]), e_make(zetas[4 * k + 2], zetas[4 * k + 3]),
                         &fap[k * 2 * total_cols], pt);
        for (int i = 0; i < 5; i++) { fpp[k * 10 + 2 * i] = pt[i].a; fpp[k * 10 + 2 * i + 1] = pt[i].b; }
    });

    mark("transcript 4 + fri alpha powers (host)");
    // ---- FRI: batch polynomial, commit phase
    u64 *dev_fap, *dev_fpp, *fv, *fcoef;
    GLP_TRY(tmp.words(&dev_fap, fap.size()));
    GLP_TRY(h2d(c, dev_fap, fap.data(), fap.size() * 8));
    GLP_TRY(tmp.words(&dev_fpp, fpp.size()));
    GLP_TRY(h2d(c, dev_fpp, fpp.data(), fpp.size() * 8));
    GLP_TRY(tmp.words(&fv, (size_t)K * 2 * n));
    GLP_TRY(tmp.words(&fcoef, (size_t)K * 2 * n));
    GLP_TRY(stage_fri_values(c, g, ob, dev_fap, nullptr, dev_fpp, fv, fcoef));
    FriState fri;
    fri.start(fcoef, lg);
    u64 *dev_betas;
    GLP_TRY(tmp.words(&dev_betas, (size_t)K * 2));
    std::vector<u64> betas_h((size_t)K * 2);
    for (u32 r = 0; r < nred; r++) {
        GLP_TRY(stage_fri_commit(c, g, tmp, fri));
        const FriLayer &ly = fri.layers.back();
        GLP_TRY(caps_to_host(c, ly.dig, ly.ndig * 4, merkle_cap_offset(((size_t)1 << ly.lgL) >> ly.ab, g.cap_height), capn, K, caps));
        pool.run(K, [&](size_t k) {
            memcpy(P((u32)k) + L.fri_caps + (size_t)r * capn * 4, &caps[k * capn * 4], (size_t)capn * 32);
            ch[k].observe_hashes(&caps[k * capn * 4], capn);
            const ext2 beta = ch[k].get_ext();
            betas_h[2 * k] = beta.a; betas_h[2 * k + 1] = beta.b;
        });
        GLP_TRY(h2d(c, dev_betas, betas_h.data(), betas_h.size() * 8));
        GLP_TRY(stage_fri_fold(c, g, tmp, fri, e_from(0), dev_betas));
    }
    mark("fri combine + layers");
    const int lgcur = fri.lgcur;
    const size_t fl = (size_t)1 << lgcur;
    if (fl != L.final_len) return set_error(GLP_ERR_ARG, "reduction_arity_bits inconsistent with degree_bits");
    std::vector<u64> fh((size_t)K * 2 * fl);
    GLP_TRY(d2h(c, fh.data(), fri.cur, fh.size() * 8));

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
    std::vector<u64> best;
    GLP_TRY(pow_search_batch(c, tmp, hasher, pst, ppos, d.proof_of_work_bits, best));
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
    GLP_TRY(tmp.words(&dev_idx, xi.size()));
    GLP_TRY(tmp.words(&dev_q, (size_t)K * qsec));
    GLP_TRY(h2d(c, dev_idx, xi.data(), xi.size() * 8));
    GLP_TRY(stage_queries(c, g, ob, fri.layers, dev_idx, dev_q, stride, qsec));
    // one strided copy puts every proof's query section in its place
    GLP_HIP(hipMemcpy2DAsync(proofs_out + L.queries, L.total * 8, dev_q, qsec * 8, qsec * 8, K, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    mark("queries");
    return GLP_OK;
}

}  // namespace

