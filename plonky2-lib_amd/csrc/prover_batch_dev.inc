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
// Between the transcript kernels the device stages are the functions of prover_stages.inc, fed the arrays those kernels wrote.
#include "transcript_dev.h"
namespace {

int prove_batch_impl_dev(glp_ctx *c, const glp_circuit *cc, u32 K, const u64 *dev_wires, const u64 *public_inputs, u64 *proofs_out) {
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const ProveGeo pg = prove_geo(cc, K);
    GLP_TRY(batch_check(pg));
    const int lg = pg.lg, rb = pg.rb, hasher = pg.hasher;
    const size_t n = pg.n, N = pg.N;
    const u32 nch = pg.nch, nw = pg.nw, qdf = pg.qdf, npp = pg.npp, nzp = pg.nzp, capn = pg.capn, nterms = pg.nterms, npi = d.num_public_inputs;
    const u32 nred = d.num_reductions, nq = d.num_query_rounds;
    BatchTrace mark(c, K, " dev");
    Scratch tmp(c);
    BatchHolder wb, zb, qb;
    u64 salt_seed[4] = {0, 0, 0, 0};     // zk circuit: one seed per call, proof k salts with seed3 + k (merkle_fill_salts)
    const u64 *salt = nullptr;
    if (cc->zk) { GLP_TRY(salt_seed_draw(c, salt_seed)); salt = salt_seed; }
    const unsigned tgrid = (K + 15) / 16;
    u64 *dch, *image;
    u32 *dev_err;
    GLP_TRY(tmp.words(&dch, (size_t)K * DCH_WORDS));
    GLP_TRY(tmp.words(&image, (size_t)K * L.total));
    { u64 *e; GLP_TRY(tmp.words(&e, (K + 1) / 2 + 1)); dev_err = (u32 *)e; }
    GLP_HIP(hipMemsetAsync(dev_err, 0, (size_t)K * 4, c->stream));
    if (npi) GLP_HIP(hipMemcpy2DAsync(image + L.pis, L.total * 8, public_inputs, (size_t)npi * 8, (size_t)npi * 8, K, hipMemcpyHostToDevice, c->stream));
    TrGeo g;
    g.dch = dch; g.image = image; g.total = L.total; g.K = K; g.capn = capn; g.nch = nch;

    // ---- wires commitment, transcript 1
    GLP_TRY(batch_build(c, dev_wires, BATCH_VALUES, nw, lg, rb, (int)d.cap_height, &wb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_WIRES));
    const size_t ndig = wb.b->ndigests, cap_off = merkle_cap_offset(N, (int)d.cap_height);
    u64 *dev_chal, *dev_qpp;
    GLP_TRY(tmp.words(&dev_chal, (size_t)K * 2 * MAXCH));
    GLP_TRY(tmp.words(&dev_qpp, (size_t)K * 3 * MAXCH));
    GLP_HIP(hipMemsetAsync(dev_chal, 0, (size_t)K * 2 * MAXCH * 8, c->stream));
    GLP_HIP(hipMemsetAsync(dev_qpp, 0, (size_t)K * 3 * MAXCH * 8, c->stream));
    hipLaunchKernelGGL(k_tr_begin, dim3(tgrid), dim3(256), 0, c->stream, g, cc->digest[0], cc->digest[1], cc->digest[2], cc->digest[3], L.pis, npi,
                       wb.b->digests + 4 * cap_off, ndig * 4, L.caps, dev_chal, dev_qpp);
    GLP_HIP(hipGetLastError());
    mark("wires commit + transcript 1");

    // ---- partial products + Z, commitment, transcript 2 (alphas and their powers)
    u64 *zp, *dens, *tot;
    GLP_TRY(tmp.words(&zp, (size_t)K * nzp * n));
    GLP_TRY(tmp.words(&dens, (size_t)K * nzp * n));
    GLP_TRY(tmp.words(&tot, (size_t)K * nch * nblk(n)));
    GLP_TRY(stage_partial_products(c, pg, dev_wires, nullptr, nullptr, dev_chal, zp, dens, tot));
    GLP_TRY(batch_build(c, zp, BATCH_VALUES, nzp, lg, rb, (int)d.cap_height, &zb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_ZS));
    const size_t apn = (size_t)nch * nterms;
    u64 *dev_apow, *qv, *qV, *qc, *l0t;
    GLP_TRY(tmp.words(&dev_apow, (size_t)(1 + APL_WORDS) * K * apn));
    hipLaunchKernelGGL(k_tr_alphas, dim3(tgrid), dim3(256), 0, c->stream, g, zb.b->digests + 4 * cap_off, ndig * 4, L.caps + (size_t)capn * 4, nterms, dev_apow,
                       dev_apow + (size_t)K * apn);
    GLP_HIP(hipGetLastError());
    mark("partial products + commit + transcript 2");

    // ---- quotient
    const size_t qstride = (size_t)nch * pg.Rq * n;
    GLP_TRY(tmp.words(&qv, (size_t)K * qstride));
    GLP_TRY(tmp.words(&qV, (size_t)K * qstride));
    GLP_TRY(tmp.words(&qc, (size_t)K * qstride));
    GLP_TRY(tmp.words(&l0t, (size_t)pg.Rq * n));
    {
        QProof qp;
        QBatch qbt;
        quotient_proof_args(pg, wb.b, zb.b, qv, dev_apow, dev_qpp, qp, qbt);
        GLP_TRY(stage_quotient_eval(c, pg, qp, qbt, l0t));
        GLP_TRY(stage_quotient_coeffs(c, pg, qv, qV, qc));
    }
    GLP_TRY(batch_build(c, qc, BATCH_COEFFS_BITREV, nch * qdf, lg, rb, (int)d.cap_height, &qb.b, nullptr, K, hasher, salt, GLP_SALT_TAG_QUOTIENT));
    const u64 wn = root_of_unity(lg);
    u64 *dev_zetas;
    GLP_TRY(tmp.words(&dev_zetas, (size_t)K * 4));
    hipLaunchKernelGGL(k_tr_zeta, dim3(tgrid), dim3(256), 0, c->stream, g, qb.b->digests + 4 * cap_off, ndig * 4, L.caps + 2 * (size_t)capn * 4, (u32)lg, wn, dev_zetas,
                       dev_err);
    GLP_HIP(hipGetLastError());
    mark("quotient + commit + transcript 3");

    // ---- openings
    const glp_batch *ob[4] = {cc->cs, wb.b, zb.b, qb.b};
    u64 *zt, *partial;
    GLP_TRY(tmp.words(&zt, (size_t)K * 2 * n));
    OpenGeo og;
    open_offsets(pg, ob, og.poff);
    for (int b = 0; b < 4; b++) og.cols[b] = ob[b]->ncols;
    og.openings_off = L.openings; og.nob = open_blocks(n); og.nch = nch; og.npp = npp; og.nopen = (u32)L.nopen;
    GLP_TRY(tmp.words(&partial, (size_t)K * og.poff[5]));
    GLP_TRY(stage_open(c, pg, ob, nullptr, dev_zetas, zt, partial, og.poff));
    hipLaunchKernelGGL(k_open_reduce, dim3(nblk((size_t)K * L.nopen)), dim3(256), 0, c->stream, g, og, partial);
    GLP_HIP(hipGetLastError());
    const size_t total_cols = oracle_cols(ob);
    u64 *dev_fap, *dev_fpp, *fv, *fcoef;
    GLP_TRY(tmp.words(&dev_fap, (size_t)K * 2 * total_cols));
    GLP_TRY(tmp.words(&dev_fpp, (size_t)K * 10));
    hipLaunchKernelGGL(k_tr_fri_alpha, dim3(tgrid), dim3(256), 0, c->stream, g, og, dev_zetas, dev_fap, dev_fpp);
    GLP_HIP(hipGetLastError());
    mark("openings + transcript 4");

    // ---- FRI: batch polynomial, commit phase
    GLP_TRY(tmp.words(&fv, (size_t)K * 2 * n));
    GLP_TRY(tmp.words(&fcoef, (size_t)K * 2 * n));
    GLP_TRY(stage_fri_values(c, pg, ob, dev_fap, nullptr, dev_fpp, fv, fcoef));
    FriState fri;
    fri.start(fcoef, lg);
    u64 *dev_betas;
    GLP_TRY(tmp.words(&dev_betas, (size_t)K * 2));
    for (u32 r = 0; r < nred; r++) {
        GLP_TRY(stage_fri_commit(c, pg, tmp, fri));
        const FriLayer &ly = fri.layers.back();
        hipLaunchKernelGGL(k_tr_beta, dim3(tgrid), dim3(256), 0, c->stream, g, fri_layer_cap(pg, ly), ly.ndig * 4,
                           L.fri_caps + (size_t)r * capn * 4, dev_betas);
        GLP_HIP(hipGetLastError());
        GLP_TRY(stage_fri_fold(c, pg, tmp, fri, e_from(0), dev_betas));
    }
    const int lgcur = fri.lgcur;
    const size_t fl = (size_t)1 << lgcur;
    if (fl != L.final_len) return set_error(GLP_ERR_ARG, "reduction_arity_bits inconsistent with degree_bits");
    u64 *dev_pst, *dev_best, *dev_next, *dev_ppos;
    GLP_TRY(tmp.words(&dev_pst, (size_t)K * 12));
    GLP_TRY(tmp.words(&dev_best, K));
    GLP_TRY(tmp.words(&dev_next, K));
    GLP_TRY(tmp.words(&dev_ppos, (K + 1) / 2));
    GLP_HIP(hipMemsetAsync(dev_next, 0, (size_t)K * 8, c->stream));
    GLP_HIP(hipMemsetAsync(dev_best, 0xFF, (size_t)K * 8, c->stream));
    hipLaunchKernelGGL(k_tr_final, dim3(tgrid), dim3(256), 0, c->stream, g, fri.cur, (u32)lgcur, L.final_poly, dev_pst, (u32 *)dev_ppos, dev_err);
    GLP_HIP(hipGetLastError());
    mark("fri combine + layers + transcript 5");

    // ---- proof of work: one persistent launch over the K sponges, then transcript 6 (response check, query indices)
    GLP_TRY(pow_batch_launch(c, tmp, dev_pst, (const u32 *)dev_ppos, d.proof_of_work_bits, dev_best, dev_next, K));
    u64 *dev_idx;
    GLP_TRY(tmp.words(&dev_idx, (size_t)K * nq));
    hipLaunchKernelGGL(k_tr_queries, dim3(tgrid), dim3(256), 0, c->stream, g, dev_best, d.proof_of_work_bits, L.pow, nq, (u64)N, dev_idx, dev_err);
    GLP_HIP(hipGetLastError());
    mark("proof of work + transcript 6");

    // ---- query phase: every gather writes straight into the image
    u64 *dev_q = image + L.queries;
    const size_t stride = L.query_stride, qsec = L.total;        // batch stride of the query records = one whole proof
    GLP_TRY(stage_queries(c, pg, ob, fri.layers, dev_idx, dev_q, stride, qsec));
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
    if (!wires_on_device) GLP_TRY(host_wires_check(c, "glp_prove_batch", "wires", cc, num_proofs, wires));
    GLP_TRY(public_inputs_check(c, "glp_prove_batch", cc, num_proofs, public_inputs));
    GLP_TRY(bind(c));
    static const u64 no_pis = 0;
    const u64 *pis = public_inputs ? public_inputs : &no_pis;
    // transcripts on the device (PoseidonGoldilocksConfig); on host threads for KeccakGoldilocksConfig or with GLP_BATCH_HOST_TRANSCRIPT=1
    const bool dev_tr = cc->d.hasher == GLP_HASH_POSEIDON && !getenv("GLP_BATCH_HOST_TRANSCRIPT");
    auto impl = dev_tr ? prove_batch_impl_dev : prove_batch_impl;
    Scratch sc(c);
    const u64 *dev_wires;
    GLP_TRY(sc.input(wires, wires_on_device, (size_t)num_proofs * cc->d.num_wires << cc->d.degree_bits, &dev_wires));
    return impl(c, cc, num_proofs, dev_wires, pis, proofs_out);
}
