// prover.hip -- `CircuitData::prove` after witness generation, on one MI355X.
//
// Replaces plonky2 0.1.4 `plonk/prover.rs::prove_with_partition_witness` (from "compute wires
// commitment" on), `plonk/vanishing_poly.rs`, `plonk/proof.rs::OpeningSet::new`,
// `fri/oracle.rs::prove_openings`, `fri/prover.rs::{fri_committed_trees, fri_proof_of_work,
// fri_prover_query_rounds}` and `iop/challenger.rs`, i.e. everything behind `data.prove(pw)`
// [REF src/ecdsa/gadgets/ecdsa.rs:349] except witness generation (CPU, the reference's generators).
// Gate bodies: plonky2 gates/{noop,constant,public_input,arithmetic_base}.rs and the reference's
// [REF src/u32/gates/interleave_u32.rs:84-135, uninterleave_to_u32.rs:93-150, uninterleave_to_b32.rs:95-150].
//
// Data stays on the GPU between stages; the host runs the Fiat-Shamir transcript (a few dozen
// Poseidon permutations) and sequences kernels.  Per proof the PCIe traffic is caps, openings,
// query paths (KBs) in and challenges out.
//
// One translation unit, in this order: the kernels (pp_kernels.inc, quotient_kernels.inc, fri_kernels.inc), the host helpers, the
// stage functions (prover_stages.inc), the single-proof session and prove_impl, the circuit handle and the entry points of the byte
// format (circuit_create.inc, over circuit_common.h and proof_bytes.h), the prove / session / staged-witness C ABI, openings and FRI of caller-held batches
// (fri_openings.inc), the permutation argument and the gate programs of a caller-held circuit (perm_seam.inc, gate_program.inc), its identity check at zeta (zeta_check.inc), its own running arguments (trace_program.inc, running_columns.inc), the witness checker (witness_check.inc), the program gates of a circuit (circuit_program.inc) and the batch drivers (prover_batch*.inc).
#include <algorithm>
#include <string.h>
#include "batch.h"
#include "common.h"
#include "host_pool.h"   // host_field_check, the transcripts' host threads
#include "merkle.h"
#include "ntt.h"
#include "poseidon.h"
#include "proof_bytes.h"
#include "prover_types.h"
#include "fri_shape.h"      // POW_MAX_BITS and the FRI shape rules
#include "witness_plan.h"   // witness_row_gate, the gate of a row: one text with k_witness_fill and the witness planner

// ------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ u64 dpow(u64 b, u64 e) {
    u64 r = 1;
    while (e) { if (e & 1) r = mul(r, b); b = sqr(b); e >>= 1; }
    return r;
}

#include "pp_kernels.inc"
#include "quotient_kernels.inc"
#include "fri_kernels.inc"

// ------------------------------------------------------------------------------------------ host side
namespace {
struct BatchHolder {
    glp_batch *b = nullptr;
    ~BatchHolder() { batch_destroy(b); }
};
inline unsigned nblk(size_t n) { return (unsigned)((n + 255) / 256); }
// the batch proof-of-work search for PoseidonGoldilocksConfig (k_pow_prepare + k_pow_batch2); st / pos / best / next as for k_pow_batch
int pow_batch_launch(glp_ctx *c, Scratch &tmp, const u64 *dev_pst, const u32 *dev_ppos, u32 bits, u64 *dev_best, u64 *dev_next, u32 K) {
    u64 *dev_k;
    GLP_TRY(tmp.words(&dev_k, (size_t)K * 12 + 1));              // + the ticket counter
    hipLaunchKernelGGL(k_pow_prepare, dim3((K + 63) / 64), dim3(64), 0, c->stream, dev_pst, dev_ppos, dev_k, K);
    GLP_HIP(hipGetLastError());
    constexpr u32 CHUNKS = 8;                                  // chunks of 256 candidates per non-persistent workgroup
    const double expected = (double)K * (bits >= 8 ? (double)(1ull << (bits - 8)) : 1.0);      // chunks: K 2^bits / 256
    const u32 tail = (u32)c->num_cus * 4;                      // these stay until every proof is finished
    const u32 body = (u32)std::min<double>(4.0 * expected / CHUNKS + 1.0, (double)(1u << 22));
    hipLaunchKernelGGL(k_pow_batch2, dim3(body + tail), dim3(256), 0, c->stream, dev_k, dev_ppos, bits,
                       (unsigned long long *)dev_best, (unsigned long long *)dev_next, K, CHUNKS, body);
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}
int batch_cap_host(glp_ctx *c, const glp_batch *b, std::vector<u64> &cap) {
    const size_t N = (size_t)1 << (b->lg + b->rate_bits);
    cap.resize((size_t)4 << b->cap_height);
    return d2h(c, cap.data(), b->digests + 4 * merkle_cap_offset(N, b->cap_height), cap.size() * 8);
}
}  // namespace

// The half of the quotient's way back to coefficients that needs no circuit (batch.h): the library's own quotient
// (stage_quotient_coeffs) and a caller's (glp_batch_from_coset_values, glp_coset_ifft) both end here.  One n-point inverse
// transform per plane, then k_quotient_combine: undo the plane twist, inverse DFT across the planes, undo the coset shift.
int glp::coset_planes_to_chunk_coeffs(glp_ctx *c, const u64 *pv, u64 *pV, u64 *out, u32 channels, int lg, int sub_bits, u64 shift) {
    const u32 Rq = 1u << sub_bits;
    const size_t n = (size_t)1 << lg;
    GLP_TRY(intt_values_to_coeffs(c, pv, pV, channels * Rq, lg));
    QCArgs q;
    q.lg = (u32)lg; q.Rq = Rq;
    q.wM_inv = inv(root_of_unity(lg + sub_bits)); q.wR_inv = inv(root_of_unity(sub_bits)); q.g_inv = inv(shift);
    q.rq_inv = inv((u64)Rq);
    const u64 gni = inv(pow(shift, (u64)n));
    u64 x = 1;
    for (u32 cidx = 0; cidx < Rq; cidx++) { q.gn_inv_pow[cidx] = x; x = mul(x, gni); }
    for (u32 c0 = 0; c0 < channels; c0 += GRID_YZ_MAX) {      // the channel rides in grid.y; the prover's [K][nch] channels fit one launch
        q.V = pV + (size_t)c0 * Rq * n; q.out = out + (size_t)c0 * Rq * n;
        hipLaunchKernelGGL(k_quotient_combine, dim3(nblk(n), std::min(GRID_YZ_MAX, channels - c0)), dim3(256), 0, c->stream, q);
        GLP_HIP(hipGetLastError());
    }
    return GLP_OK;
}
#include "prover_stages.inc"

// One proof in flight, cut at the points where the Fiat-Shamir transcript needs something from the device or the device
// needs a challenge.  glp_prove() drives it with the built-in Challenger; the glp_session_* entry points hand the same
// steps to a caller that keeps its own transcript (the Rust prover's `Challenger`): SURVEY.md section 8(b).
struct glp_session {
    glp_ctx *c;
    const glp_circuit *cc;
    const glp_circuit_desc &d;
    const Layout &L;
    const ProveGeo g;                  // K = 1
    Scratch tmp;
    u64 *owned_wires = nullptr;        // device copy made by begin() when the caller passed host memory
    const u64 *dev_wires = nullptr;
    u64 pih[4] = {0, 0, 0, 0};
    u64 salt_seed[4] = {0, 0, 0, 0};   // zk circuit: the seed of this proof's salts (drawn in begin), else unused
    const u64 *salt = nullptr;         // salt_seed for a zk circuit, nullptr otherwise
    BatchHolder wb, zb, qb;
    u64 betas[MAXCH] = {}, gammas[MAXCH] = {};
    ext2 zeta = {0, 0}, zeta_next = {0, 0};
    const glp_batch *ob[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<ext2> open[4], zs_next;
    FriState fri;
    bool layer_open = false;           // a commit-phase layer has been committed and waits for its beta
    std::vector<u64> proof_words;      // the proof being assembled (glp_proof_words(circuit) words)
    std::vector<u64> cap;
    enum Stage { S_NEW, S_WIRES, S_ZS, S_QUOTIENT, S_OPEN, S_FRI, S_FINAL, S_DONE } stage = S_NEW;

    glp_session(glp_ctx *ctx, const glp_circuit *circ) : c(ctx), cc(circ), d(circ->d), L(circ->L), g(prove_geo(circ, 1)), tmp(ctx) {}
    ~glp_session() { if (owned_wires) { (void)hipStreamSynchronize(c->stream); c->release(owned_wires); } }
    u64 *proof() { return proof_words.data(); }
    // commits an oracle of this proof; its cap -> cap and the proof's cap slot `slot`
    int commit(const u64 *dev_in, int kind, u32 ncols, BatchHolder &out, u32 tag, u32 slot, const u64 *host_src = nullptr) {
        GLP_TRY(batch_build(c, dev_in, kind, ncols, g.lg, g.rb, g.cap_height, &out.b, host_src, 1, g.hasher, salt, tag));
        GLP_TRY(batch_cap_host(c, out.b, cap));
        memcpy(proof() + L.caps + (size_t)slot * g.capn * 4, cap.data(), g.capn * 32);
        return GLP_OK;
    }

    // K1-K4 over the witness; wires cap -> proof, cap
    // host_wires != nullptr: the witness is still in host memory and is uploaded into wires_dev chunk by chunk, overlapped
    // with the iNTT / LDE of the chunks already there
    int begin(const u64 *wires_dev, const u64 *public_inputs, const u64 *host_wires = nullptr) {
        GLP_REQUIRE(stage == S_NEW, "session already begun");
        proof_words.assign(L.total, 0);
        dev_wires = wires_dev;
        if (cc->zk) { GLP_TRY(salt_seed_draw(c, salt_seed)); salt = salt_seed; }
        host_hash_no_pad(public_inputs, d.num_public_inputs, pih);
        if (d.num_public_inputs) memcpy(proof() + L.pis, public_inputs, (size_t)d.num_public_inputs * 8);
        GLP_TRY(commit(dev_wires, BATCH_VALUES, g.nw, wb, GLP_SALT_TAG_WIRES, 0, host_wires));
        stage = S_WIRES;
        return GLP_OK;
    }
    // K5 + commitment of Z and the partial products
    int partial_products(const u64 *betas_in, const u64 *gammas_in) {
        GLP_REQUIRE(stage == S_WIRES, "partial_products: call after begin");
        for (u32 i = 0; i < g.nch; i++) { betas[i] = betas_in[i]; gammas[i] = gammas_in[i]; }
        u64 *zp, *dens, *tot;
        GLP_TRY(tmp.words(&zp, (size_t)g.nzp * g.n));
        GLP_TRY(tmp.words(&dens, (size_t)g.nzp * g.n));
        GLP_TRY(tmp.words(&tot, (size_t)g.nch * nblk(g.n)));
        {
            StageScope st(c, "partial_products", 8.0 * g.n * (2.0 * g.nr + g.nzp));
            GLP_TRY(stage_partial_products(c, g, dev_wires, betas, gammas, nullptr, zp, dens, tot));
        }
        GLP_TRY(commit(zp, BATCH_VALUES, g.nzp, zb, GLP_SALT_TAG_ZS, 1));
        stage = S_ZS;
        return GLP_OK;
    }
    // K6 + commitment of the quotient chunks
    int quotient(const u64 *alphas) {
        GLP_REQUIRE(stage == S_ZS, "quotient: call after partial_products");
        const u32 nch = g.nch;
        const size_t apn = (size_t)nch * g.nterms, qlen = (size_t)nch * g.Rq * g.n;
        std::vector<u64> apow((1 + APL_WORDS) * apn);
        alpha_power_table(alphas, nch, g.nterms, apow.data(), apow.data() + apn);
        u64 *dev_apow, *qv, *qV, *qc;
        GLP_TRY(tmp.words(&dev_apow, apow.size()));
        GLP_TRY(h2d(c, dev_apow, apow.data(), apow.size() * 8));
        GLP_TRY(tmp.words(&qv, qlen));
        GLP_TRY(tmp.words(&qV, qlen));
        GLP_TRY(tmp.words(&qc, qlen));
        QProof qp;
        QBatch qbt;
        quotient_proof_args(g, wb.b, zb.b, qv, dev_apow, nullptr, qp, qbt);      // pp == nullptr: one proof, described by qp
        for (u32 i = 0; i < nch; i++) { qp.betas[i] = betas[i]; qp.gammas[i] = gammas[i]; }
        memcpy(qp.pih, pih, 32);
        {
            StageScope st(c, "quotient_eval", 8.0 * g.n * g.Rq * (g.nc + g.nr + g.nw + g.nzp + 2.0 * nch));
            u64 *l0t;
            GLP_TRY(tmp.words(&l0t, (size_t)g.Rq * g.n));
            GLP_TRY(stage_quotient_eval(c, g, qp, qbt, l0t));
        }
        {
            StageScope st(c, "quotient_intt", 16.0 * g.n * g.Rq * nch);
            GLP_TRY(stage_quotient_coeffs(c, g, qv, qV, qc));
        }
        GLP_TRY(commit(qc, BATCH_COEFFS_BITREV, nch * g.qdf, qb, GLP_SALT_TAG_QUOTIENT, 2));
        stage = S_QUOTIENT;
        return GLP_OK;
    }
    // K7: every committed polynomial at zeta, Z at g zeta; openings -> proof (OpeningSet order)
    int open_at(ext2 zeta_in) {
        GLP_REQUIRE(stage == S_QUOTIENT, "open: call after quotient");
        zeta = zeta_in;
        {
            ext2 zp = zeta;
            for (int i = 0; i < g.lg; i++) zp = e_sqr(zp);
            if (e_eq(zp, e_from(1))) return set_error(GLP_ERR_PROVE, "Opening point is in the subgroup.");
        }
        zeta_next = e_scale(zeta, root_of_unity(g.lg));
        ob[0] = cc->cs; ob[1] = wb.b; ob[2] = zb.b; ob[3] = qb.b;
        StageScope st(c, "openings", 8.0 * g.n * (L.oracle_cols[0] + L.oracle_cols[1] + L.oracle_cols[2] + L.oracle_cols[3] + g.nch));
        // five evaluations (four batches at zeta, the Z batch at g zeta) queued back to back, one copy back
        u64 *zt, *partial;
        size_t poff[6];
        open_offsets(g, ob, poff);
        GLP_TRY(tmp.words(&zt, 2 * g.n));
        GLP_TRY(tmp.words(&partial, poff[5]));
        const ext2 points[2] = {zeta, zeta_next};
        GLP_TRY(stage_open(c, g, ob, points, nullptr, zt, partial, poff));
        std::vector<u64> hp(poff[5]);
        GLP_TRY(d2h(c, hp.data(), partial, hp.size() * 8));
        openings_to_proof(g, ob, hp.data(), poff, open, zs_next, proof() + L.openings);
        stage = S_OPEN;
        return GLP_OK;
    }
    // K8: alpha-combination of all openings batches, quotient by (X - zeta) / (X - g zeta) -> FRI polynomial
    int fri_combine(ext2 alpha) {
        GLP_REQUIRE(stage == S_OPEN, "fri_combine: call after open");
        u64 *fcoef, *dev_ap, *fv;
        GLP_TRY(tmp.words(&fcoef, 2 * g.n));
        {
            StageScope st(c, "fri_combine", 8.0 * g.n * (L.oracle_cols[0] + L.oracle_cols[1] + L.oracle_cols[2] + L.oracle_cols[3]));
            std::vector<u64> ap(2 * oracle_cols(ob));
            ext2 pt[5];
            fri_alpha_powers(g, ob, open, zs_next, alpha, zeta, zeta_next, ap.data(), pt);
            GLP_TRY(tmp.words(&dev_ap, ap.size()));
            GLP_TRY(h2d(c, dev_ap, ap.data(), ap.size() * 8));
            GLP_TRY(tmp.words(&fv, 2 * g.n));
            GLP_TRY(stage_fri_values(c, g, ob, dev_ap, pt, nullptr, fv, fcoef));
        }
        fri.start(fcoef, g.lg);
        stage = S_FRI;
        return GLP_OK;
    }
    // K9, first half: LDE of the current polynomial on its coset, Merkle tree over arity-sized leaves; cap -> proof, cap
    int fri_commit_layer() {
        GLP_REQUIRE(stage == S_FRI && !layer_open && fri.layers.size() < d.num_reductions, "fri_commit: no layer left or beta pending");
        StageScope st(c, "fri_commit", 0.0);
        const size_t r = fri.layers.size();
        GLP_TRY(stage_fri_commit(c, g, tmp, fri));
        cap.resize((size_t)g.capn * 4);
        GLP_TRY(d2h(c, cap.data(), fri_layer_cap(g, fri.layers.back()), (size_t)g.capn * 32));
        memcpy(proof() + L.fri_caps + r * g.capn * 4, cap.data(), (size_t)g.capn * 32);
        layer_open = true;
        return GLP_OK;
    }
    // K9, second half: fold the coefficients with beta (arity 2^ab), shift <- shift^arity
    int fri_fold(ext2 beta) {
        GLP_REQUIRE(stage == S_FRI && layer_open, "fri_fold: call after fri_commit");
        StageScope st(c, "fri_commit", 0.0);
        GLP_TRY(stage_fri_fold(c, g, tmp, fri, beta, nullptr));
        layer_open = false;
        return GLP_OK;
    }
    // final polynomial (natural coefficient order) -> proof
    int fri_final_poly() {
        GLP_REQUIRE(stage == S_FRI && !layer_open && fri.layers.size() == d.num_reductions, "fri_final_poly: reductions not finished");
        const size_t fl = (size_t)1 << fri.lgcur;
        if (fl != L.final_len) return set_error(GLP_ERR_ARG, "reduction_arity_bits inconsistent with degree_bits");
        std::vector<u64> h(2 * fl);
        GLP_TRY(d2h(c, h.data(), fri.cur, h.size() * 8));
        for (size_t p = 0; p < fl; p++) {
            const size_t k = bitrev32((u32)p, fri.lgcur);
            proof()[L.final_poly + 2 * k] = h[p];
            proof()[L.final_poly + 2 * k + 1] = h[fl + p];
        }
        stage = S_FINAL;
        return GLP_OK;
    }
    // query phase: leaves and Merkle paths of the four initial oracles and of every commit-phase layer
    int queries(u64 pow_witness, const u64 *indices, u32 nq) {
        GLP_REQUIRE(stage == S_FINAL, "queries: call after fri_final_poly");
        GLP_REQUIRE(nq == d.num_query_rounds, "queries: %u indices, the circuit has %u query rounds", nq, d.num_query_rounds);
        proof()[L.pow] = pow_witness;
        StageScope st(c, "fri_queries", 0.0);
        std::vector<u64> xi(indices, indices + nq);
        for (u32 q = 0; q < nq; q++) GLP_REQUIRE(xi[q] < (u64)g.N, "query index %llu outside the LDE domain", (unsigned long long)xi[q]);
        // every gather writes straight into a device image of the proof's query section; one copy brings it back
        u64 *dev_idx, *dev_q;
        const size_t qsec = (size_t)nq * L.query_stride;
        GLP_TRY(tmp.words(&dev_idx, nq));
        GLP_TRY(tmp.words(&dev_q, qsec));
        GLP_TRY(h2d(c, dev_idx, xi.data(), nq * 8));
        GLP_TRY(stage_queries(c, g, ob, fri.layers, dev_idx, dev_q, L.query_stride, qsec));
        GLP_TRY(d2h(c, proof() + L.queries, dev_q, qsec * 8));
        stage = S_DONE;
        return GLP_OK;
    }
};

// The sponge a proof-of-work search or a one-call FRI proof resumes from: K states of 12 words, K x npending buffered inputs.  Every
// word is a field element and must be canonical: pos::permute and pos::pow_round0_consts add round constants with glf::add
// (canonical in), and a word >= p names no state that a transcript can be in.  Host check, before any launch.
static int sponge_args_check(const u64 *states, const u64 *pending, u32 npending, u32 K, bool many) {
    for (u32 k = 0; k < K; k++) {
        for (u32 i = 0; i < 12; i++) {
            const u64 v = states[(size_t)k * 12 + i];
            if (v < P) continue;
            if (many) return set_error(GLP_ERR_ARG, "sponge_states[%u][%u] = 0x%016llx is not canonical", k, i, (unsigned long long)v);
            return set_error(GLP_ERR_ARG, "sponge_state[%u] = 0x%016llx is not canonical", i, (unsigned long long)v);
        }
        for (u32 i = 0; i < npending; i++) {
            const u64 v = pending[(size_t)k * npending + i];
            if (v < P) continue;
            if (many) return set_error(GLP_ERR_ARG, "pending_inputs[%u][%u] = 0x%016llx is not canonical", k, i, (unsigned long long)v);
            return set_error(GLP_ERR_ARG, "pending_inputs[%u] = 0x%016llx is not canonical", i, (unsigned long long)v);
        }
    }
    return GLP_OK;
}

// K10: smallest witness w >= 0 such that the sponge (state + pending inputs + w) squeezes a value with `bits` leading
// zeros.  The search covers candidates in increasing order, so the result does not depend on launch geometry.
static int pow_search(glp_ctx *c, const u64 st[12], const u64 *pending, u32 npending, u32 bits, u64 *witness, int hasher = GLP_HASH_POSEIDON) {
    StageScope stg(c, "fri_pow", 0.0);
    GLP_REQUIRE(npending < 8, "proof of work: %u pending inputs (the rate is 8)", npending);
    PowArgs a;
    memcpy(a.st, st, 96);
    for (u32 i = 0; i < npending; i++) a.st[i] = pending[i];
    a.pos = npending; a.bits = bits;
    Scratch tmp(c);
    u64 *best;
    GLP_TRY(tmp.words(&best, 1));
    a.best = (unsigned long long *)best;
    const u64 none = ~0ull;
    u64 found = none;
    // expected 2^bits tries: size a launch at four times that (a 2^20-candidate launch is 0.6 ms of hashing)
    const u64 batch = 1ull << std::min<u32>(20, std::max<u32>(14, bits + 2));
    for (u64 base = 0; found == none; base += batch) {
        if (base >= (1ull << 40)) return set_error(GLP_ERR_PROVE, "Proof of work failed. This is highly unlikely!");
        GLP_TRY(h2d(c, best, &none, 8));
        a.base = base;
        if (hasher == GLP_HASH_KECCAK25) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pow<GLP_HASH_KECCAK25>), dim3((unsigned)(batch / 256)), dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pow<GLP_HASH_POSEIDON>), dim3((unsigned)(batch / 256)), dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
        GLP_TRY(d2h(c, &found, best, 8));
    }
    *witness = found;
    return GLP_OK;
}

// prove(): the session driven by the library's own transcript (plonk/prover.rs order)
static int prove_impl(glp_ctx *c, const glp_circuit *cc, const u64 *dev_wires, const u64 *public_inputs, u64 *proof,
                      const u64 *host_wires = nullptr) {
    glp_session s(c, cc);
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const u32 nch = s.g.nch, capn = s.g.capn;
    GLP_TRY(s.begin(dev_wires, public_inputs, host_wires));
    Challenger ch((int)d.hasher);
    ch.observe_hashes(cc->digest, 1);
    ch.observe(s.pih, 4);                       // InnerHasher (Poseidon) HashOut
    ch.observe_hashes(s.cap.data(), capn);
    u64 betas[MAXCH], gammas[MAXCH], alphas[MAXCH];
    for (u32 i = 0; i < nch; i++) betas[i] = ch.get();
    for (u32 i = 0; i < nch; i++) gammas[i] = ch.get();
    GLP_TRY(s.partial_products(betas, gammas));
    ch.observe_hashes(s.cap.data(), capn);
    for (u32 i = 0; i < nch; i++) alphas[i] = ch.get();
    GLP_TRY(s.quotient(alphas));
    ch.observe_hashes(s.cap.data(), capn);
    GLP_TRY(s.open_at(ch.get_ext()));
    observe_openings(ch, s.g, s.proof() + L.openings);
    GLP_TRY(s.fri_combine(ch.get_ext()));
    for (u32 r = 0; r < d.num_reductions; r++) {
        GLP_TRY(s.fri_commit_layer());
        ch.observe_hashes(s.cap.data(), capn);
        GLP_TRY(s.fri_fold(ch.get_ext()));
    }
    GLP_TRY(s.fri_final_poly());
    ch.observe(s.proof() + L.final_poly, 2 * L.final_len);
    u64 found;
    GLP_TRY(pow_search(c, ch.st, ch.in, (u32)ch.nin, d.proof_of_work_bits, &found, (int)d.hasher));
    ch.observe(&found, 1);
    const u64 resp = ch.get();
    if (d.proof_of_work_bits && (resp >> (64 - d.proof_of_work_bits)) != 0)
        return set_error(GLP_ERR_PROVE, "proof-of-work response check failed");
    std::vector<u64> xi(d.num_query_rounds);
    for (u32 q = 0; q < d.num_query_rounds; q++) xi[q] = ch.get() % (u64)s.g.N;
    GLP_TRY(s.queries(found, xi.data(), d.num_query_rounds));
    memcpy(proof, s.proof(), L.total * 8);
    return GLP_OK;
}

#include "circuit_create.inc"

// The host field arrays of a prove call are canonical or the call is refused by name, before anything is allocated or launched: the
// witness where it is in host memory, and the public inputs.  K == 0: one proof, no proof index in the message.
static int host_wires_check(glp_ctx *c, const char *fn, const char *name, const glp_circuit *cc, u32 K, const u64 *host_wires) {
    return host_field_check(c, fn, name, host_wires, K, cc->d.num_wires, (size_t)1 << cc->d.degree_bits);
}
static int public_inputs_check(glp_ctx *c, const char *fn, const glp_circuit *cc, u32 K, const u64 *public_inputs) {
    if (!public_inputs || !cc->d.num_public_inputs) return GLP_OK;
    return host_field_check(c, fn, "public_inputs", public_inputs, K, 0, cc->d.num_public_inputs);
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

int glp_session_begin(glp_ctx *c, const glp_circuit *cc, const uint64_t *wires, int wires_on_device, const uint64_t *public_inputs,
                      glp_session **out, uint64_t *wires_cap_out, uint64_t public_inputs_hash_out[4]) {
    GLP_REQUIRE(c && cc && wires && out && wires_cap_out && public_inputs_hash_out, "null argument");
    *out = nullptr;
    GLP_REQUIRE(cc->ctx == c, "circuit belongs to another context");
    GLP_REQUIRE(public_inputs || cc->d.num_public_inputs == 0, "public_inputs is null");
    if (!wires_on_device) GLP_TRY(host_wires_check(c, "glp_session_begin", "wires", cc, 0, wires));
    GLP_TRY(public_inputs_check(c, "glp_session_begin", cc, 0, public_inputs));
    GLP_TRY(bind(c));
    std::unique_ptr<glp_session> s(new glp_session(c, cc));
    const u64 *dw = wires;
    if (!wires_on_device) {
        const size_t tot = (size_t)cc->d.num_wires << cc->d.degree_bits;
        void *dv = nullptr;
        GLP_TRY(c->alloc(&dv, tot * 8));
        s->owned_wires = (u64 *)dv;
        dw = s->owned_wires;
    }
    GLP_TRY(s->begin(dw, public_inputs, wires_on_device ? nullptr : wires));
    memcpy(wires_cap_out, s->cap.data(), (size_t)s->g.capn * 32);
    memcpy(public_inputs_hash_out, s->pih, 32);
    *out = s.release();
    return GLP_OK;
}
#define GLP_SESSION_ENTER(S)                         \
    GLP_REQUIRE((S) != nullptr, "null session");     \
    GLP_TRY(bind((S)->c))
int glp_session_partial_products(glp_session *s, const uint64_t *betas, const uint64_t *gammas, uint64_t *zs_cap_out) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(betas && gammas && zs_cap_out, "null argument");
    for (u32 i = 0; i < s->g.nch; i++) GLP_REQUIRE(betas[i] < P && gammas[i] < P, "challenge %u is not a canonical field element", i);
    GLP_TRY(s->partial_products(betas, gammas));
    memcpy(zs_cap_out, s->cap.data(), (size_t)s->g.capn * 32);
    return GLP_OK;
}
int glp_session_quotient(glp_session *s, const uint64_t *alphas, uint64_t *quotient_cap_out) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(alphas && quotient_cap_out, "null argument");
    for (u32 i = 0; i < s->g.nch; i++) GLP_REQUIRE(alphas[i] < P, "challenge %u is not a canonical field element", i);
    GLP_TRY(s->quotient(alphas));
    memcpy(quotient_cap_out, s->cap.data(), (size_t)s->g.capn * 32);
    return GLP_OK;
}
size_t glp_num_openings(const glp_circuit *cc) { return cc ? cc->L.nopen : 0; }
size_t glp_final_poly_len(const glp_circuit *cc) { return cc ? cc->L.final_len : 0; }
int glp_session_open(glp_session *s, const uint64_t zeta[2], uint64_t *openings_out) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(zeta && openings_out, "null argument");
    GLP_REQUIRE(zeta[0] < P && zeta[1] < P, "zeta is not canonical");
    GLP_TRY(s->open_at(e_make(zeta[0], zeta[1])));
    memcpy(openings_out, s->proof() + s->L.openings, s->L.nopen * 16);
    return GLP_OK;
}
int glp_session_fri_combine(glp_session *s, const uint64_t alpha[2]) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(alpha && alpha[0] < P && alpha[1] < P, "alpha is null or not canonical");
    return s->fri_combine(e_make(alpha[0], alpha[1]));
}
int glp_session_fri_commit(glp_session *s, uint64_t *cap_out) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(cap_out, "null argument");
    GLP_TRY(s->fri_commit_layer());
    memcpy(cap_out, s->cap.data(), (size_t)s->g.capn * 32);
    return GLP_OK;
}
int glp_session_fri_fold(glp_session *s, const uint64_t beta[2]) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(beta && beta[0] < P && beta[1] < P, "beta is null or not canonical");
    return s->fri_fold(e_make(beta[0], beta[1]));
}
int glp_session_fri_final_poly(glp_session *s, uint64_t *coeffs_out) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(coeffs_out, "null argument");
    GLP_TRY(s->fri_final_poly());
    memcpy(coeffs_out, s->proof() + s->L.final_poly, s->L.final_len * 16);
    return GLP_OK;
}
int glp_pow_search(glp_ctx *c, const uint64_t sponge_state[12], const uint64_t *pending_inputs, uint32_t num_pending, uint32_t bits,
                   uint64_t *witness_out) {
    GLP_REQUIRE(c && sponge_state && witness_out && (pending_inputs || num_pending == 0), "null argument");
    GLP_REQUIRE(bits <= POW_MAX_BITS, "proof_of_work_bits=%u: this build searches at most 2^40 candidates and accepts up to %u bits", bits,
                POW_MAX_BITS);
    GLP_REQUIRE(num_pending < 8, "proof of work: %u pending inputs (the rate is 8)", num_pending);
    GLP_TRY(sponge_args_check(sponge_state, pending_inputs, num_pending, 1, false));
    GLP_TRY(bind(c));
    return pow_search(c, sponge_state, pending_inputs, num_pending, bits, witness_out);
}
int glp_pow_search_h(glp_ctx *c, uint32_t hasher, const uint64_t sponge_state[12], const uint64_t *pending_inputs, uint32_t num_pending,
                     uint32_t bits, uint64_t *witness_out) {
    GLP_REQUIRE(c && sponge_state && witness_out && (pending_inputs || num_pending == 0), "null argument");
    GLP_REQUIRE(bits <= POW_MAX_BITS, "proof_of_work_bits=%u: this build searches at most 2^40 candidates and accepts up to %u bits", bits,
                POW_MAX_BITS);
    if (hasher != GLP_HASH_POSEIDON && hasher != GLP_HASH_KECCAK25) return set_error(GLP_ERR_UNSUPPORTED, "hasher %u is not one of GLP_HASH_*", hasher);
    GLP_REQUIRE(num_pending < 8, "proof of work: %u pending inputs (the rate is 8)", num_pending);
    GLP_TRY(sponge_args_check(sponge_state, pending_inputs, num_pending, 1, false));
    GLP_TRY(bind(c));
    return pow_search(c, sponge_state, pending_inputs, num_pending, bits, witness_out, (int)hasher);
}
int glp_session_queries(glp_session *s, uint64_t pow_witness, const uint64_t *indices, uint32_t num_indices) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(indices, "null argument");
    GLP_REQUIRE(pow_witness < P, "glp_session_queries: pow_witness = 0x%016llx is not a canonical field element (>= p)", (unsigned long long)pow_witness);
    return s->queries(pow_witness, indices, num_indices);
}
int glp_session_proof(glp_session *s, uint64_t *proof_out) {
    GLP_SESSION_ENTER(s);
    GLP_REQUIRE(proof_out, "null argument");
    GLP_REQUIRE(s->stage == glp_session::S_DONE, "the proof is not finished (call glp_session_queries first)");
    memcpy(proof_out, s->proof(), s->L.total * 8);
    return GLP_OK;
}
void glp_session_end(glp_session *s) {
    if (!s) return;
    (void)hipSetDevice(s->c->device);
    delete s;
}
int glp_prove_device(glp_ctx *c, const glp_circuit *cc, const uint64_t *dev_wires, const uint64_t *public_inputs, uint64_t *proof_out) {
    GLP_REQUIRE(c && cc && dev_wires && proof_out, "null argument");
    GLP_REQUIRE(cc->ctx == c, "circuit belongs to another context");
    GLP_REQUIRE(public_inputs || cc->d.num_public_inputs == 0, "public_inputs is null");
    GLP_TRY(public_inputs_check(c, "glp_prove_device", cc, 0, public_inputs));
    GLP_TRY(bind(c));
    return prove_impl(c, cc, dev_wires, public_inputs, proof_out);
}

int glp_prove(glp_ctx *c, const glp_circuit *cc, const uint64_t *wires, const uint64_t *public_inputs, uint64_t *proof_out) {
    GLP_REQUIRE(c && cc && wires && proof_out, "null argument");
    GLP_REQUIRE(cc->ctx == c, "circuit belongs to another context");
    GLP_REQUIRE(public_inputs || cc->d.num_public_inputs == 0, "public_inputs is null");
    GLP_TRY(host_wires_check(c, "glp_prove", "wires", cc, 0, wires));
    GLP_TRY(public_inputs_check(c, "glp_prove", cc, 0, public_inputs));
    GLP_TRY(bind(c));
    const size_t tot = (size_t)cc->d.num_wires << cc->d.degree_bits;
    Scratch sc(c);
    u64 *dv;                  // filled by the wires commitment's own chunked upload (batch_build, host_src)
    GLP_TRY(sc.words(&dv, tot));
    return prove_impl(c, cc, dv, public_inputs, proof_out, wires);
}

// ---- staged witnesses (include/glp.h "witnesses that start in host memory, pipelined")
}  // extern "C"
struct glp_witness {
    glp_ctx *c = nullptr;
    const glp_circuit *cc = nullptr;
    u64 *dev = nullptr;            // [num_wires][n], from the context's pool
    hipEvent_t ready = nullptr;    // recorded on the copy stream behind the upload
    bool routed_only = false, filled = false;
};
extern "C" {
int glp_host_alloc(glp_ctx *c, size_t bytes, void **host_out) {
    GLP_REQUIRE(c && host_out && bytes > 0, "null argument or zero size");
    *host_out = nullptr;
    GLP_TRY(bind(c));
    GLP_HIP(hipHostMalloc(host_out, bytes, hipHostMallocDefault));
    return GLP_OK;
}
int glp_host_free(glp_ctx *c, void *host) {
    GLP_REQUIRE(c, "null context");
    if (!host) return GLP_OK;
    GLP_TRY(bind(c));
    GLP_HIP(hipHostFree(host));
    return GLP_OK;
}
void glp_witness_free(glp_witness *w) {
    if (!w) return;
    (void)hipSetDevice(w->c->device);
    if (w->ready) { (void)hipEventSynchronize(w->ready); (void)hipEventDestroy(w->ready); }
    if (w->dev) { (void)hipStreamSynchronize(w->c->stream); w->c->release(w->dev); }
    delete w;
}
int glp_witness_stage(glp_ctx *c, const glp_circuit *cc, const uint64_t *host_wires, uint32_t flags, glp_witness **out) {
    GLP_REQUIRE(c && cc && host_wires && out, "null argument");
    *out = nullptr;
    GLP_REQUIRE(cc->ctx == c, "circuit belongs to another context");
    GLP_REQUIRE((flags & ~GLP_WITNESS_ROUTED_ONLY) == 0, "unknown flags 0x%x", flags);
    // the blinding rows of a zk circuit hold random advice wires that no generator derives: glp_witness_fill cannot rebuild them
    GLP_REQUIRE(!(cc->zk && (flags & GLP_WITNESS_ROUTED_ONLY)), "GLP_WITNESS_ROUTED_ONLY: a zero-knowledge circuit needs its full witness");
    GLP_TRY(bind(c));
    const size_t n = (size_t)1 << cc->d.degree_bits;
    const u32 nw = cc->d.num_wires, nr = cc->d.num_routed_wires;
    // only the columns that are copied are read: with GLP_WITNESS_ROUTED_ONLY the routed ones
    GLP_TRY(host_field_check(c, "glp_witness_stage", "host_wires", host_wires, 0, (flags & GLP_WITNESS_ROUTED_ONLY) ? nr : nw, n));
    std::unique_ptr<glp_witness, void (*)(glp_witness *)> w(new glp_witness(), glp_witness_free);
    w->c = c; w->cc = cc; w->routed_only = (flags & GLP_WITNESS_ROUTED_ONLY) != 0;
    void *dv = nullptr;
    GLP_TRY(c->alloc(&dv, (size_t)nw * n * 8));
    w->dev = (u64 *)dv;
    GLP_HIP(hipEventCreateWithFlags(&w->ready, hipEventDisableTiming));
    const u32 ncopy = w->routed_only ? nr : nw;
    GLP_HIP(hipMemcpyAsync(w->dev, host_wires, (size_t)ncopy * n * 8, hipMemcpyHostToDevice, c->copy_stream));
    if (ncopy < nw) GLP_HIP(hipMemsetAsync(w->dev + (size_t)ncopy * n, 0, (size_t)(nw - ncopy) * n * 8, c->copy_stream));
    GLP_HIP(hipEventRecord(w->ready, c->copy_stream));
    *out = w.release();
    return GLP_OK;
}
int glp_prove_staged(glp_ctx *c, const glp_circuit *cc, glp_witness *w, const uint64_t *public_inputs, uint64_t *proof_out) {
    GLP_REQUIRE(c && cc && w && proof_out, "null argument");
    GLP_REQUIRE(cc->ctx == c && w->c == c && w->cc == cc, "witness, circuit and context do not belong together");
    GLP_REQUIRE(public_inputs || cc->d.num_public_inputs == 0, "public_inputs is null");
    GLP_TRY(public_inputs_check(c, "glp_prove_staged", cc, 0, public_inputs));
    GLP_TRY(bind(c));
    GLP_HIP(hipStreamWaitEvent(c->stream, w->ready, 0));
    if (w->routed_only && !w->filled) {
        GLP_TRY(glp_witness_fill(c, cc, w->dev, 1));
        w->filled = true;
    }
    return prove_impl(c, cc, w->dev, public_inputs, proof_out);
}
}  // extern "C"

#include "prover_batch.inc"
#include "fri_openings.inc"
#include "perm_seam.inc"
#include "gate_program.inc"
#include "zeta_check.inc"
#include "trace_program.inc"
#include "running_columns.inc"
#include "witness_check.inc"
#include "circuit_program.inc"
#include "prover_batch_dev.inc"
