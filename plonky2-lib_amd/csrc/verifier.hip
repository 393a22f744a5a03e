// verifier.hip -- `CircuitData::verify(proof)` for the proofs this library produces [REF src/ecdsa/gadgets/ecdsa.rs:352,
// src/zkdsa/circuits/mod.rs:346: every reference test ends in `data.verify(proof)`]: the part that needs HIP.
//
// Verification is a few thousand Poseidon permutations and one constraint evaluation at a single point: glp_verify runs on
// the host, like the transcript, and touches no device memory (the circuit handle supplies the gate table, the coset
// shifts, the digest and the constants/sigmas cap).  That host half -- the extension-field algebra, the gate bodies, the transcript,
// the identity at zeta, the query rounds -- is verify_host.h, over the verifier's view of the circuit (circuit_common.h), where a
// stand-alone program runs it without a device; here are its entry points (glp_verify, glp_verify_n) and the batch driver that
// runs its front half beside the device's query rounds (glp_verify_batch).  It shares no code with the CPU checker the tests use:
// the two verifiers and the two provers are cross-checked against each other in tests/test_gpu_prove.py.
//
// The FRI query rounds are stated twice, once per side: verify_fri_host (verify_host.h: glp_verify, the independent host restatement)
// and k_fri_verify_queries (verify_dev.h), the one device kernel behind glp_verify_batch (the plonk instance of a circuit) and
// glp_fri_verify* (fri_verify.inc: any instance).  Both report a failure as the same status word (FV_*, fri_shape.h), query_failure() words it.
#include <chrono>
#include <string>
#include <thread>
#include "host_pool.h"
#include "merkle.h"
#include "prover_types.h"
#include "transcript_dev.h"
#include "verify_dev.h"
#include "verify_host.h"

// ------------------------------------------------------------------------------------------ query rounds on the device
// glp_verify_batch (a GPU verifier for batch self-checking; every reference driver proves and then
// verifies [REF src/zkdsa/circuits/mod.rs:341-347, src/ecdsa/gadgets/ecdsa.rs:349-352]).  Per proof the transcript, the proof of
// work and the one constraint evaluation at zeta stay on host threads (verify_front: a few dozen permutations); the query
// rounds -- K x num_query_rounds independent checks, each a few dozen to a few hundred permutations (Merkle paths of the four
// initial oracles and of every FRI layer), `fri_combine_initial`, the arity-2^k interpolations and the final polynomial -- are
// one launch of k_fri_verify_queries (verify_dev.h) on the plonk instance of the circuit: a 16-lane group per (proof, query),
// hashes in the 12-lane cooperative form (poseidon.h permute_coop: ~5x lower latency per hash than one state per lane, which is
// what matters for a chain of dependent hashes), the alpha-combination and the Lagrange terms spread over the lanes of the group.
//
// What surrounds that launch is the same for glp_verify_batch and glp_fri_verify* (fri_verify.inc) and stands here once.
namespace {
// The proofs go up (pageable host memory: the copy blocks its caller) on a thread of their own while the host half runs.  done() joins
// it; so does the destructor, when the call returns early or a host task throws.  Declared after the Scratch whose buffers it fills.
struct Uploader {
    hipError_t err = hipSuccess;
    std::thread t;
    template <class F> Uploader(glp_ctx *c, F copies) : t([this, c, copies] { err = hipSetDevice(c->device); if (err == hipSuccess) err = copies(); }) {}
    Uploader(const Uploader &) = delete;
    ~Uploader() { if (t.joinable()) t.join(); }
    int done() { t.join(); return err == hipSuccess ? GLP_OK : set_error(GLP_ERR_HIP, "upload of the proofs: %s", hipGetErrorString(err)); }
};
// every query round of every proof in one launch, timed as `stage`
int launch_queries(glp_ctx *c, int hasher, const char *stage, const FVArgs &a) {
    StageScope st(c, stage, 8.0 * a.K * a.total);
    const unsigned nblocks = (unsigned)(((size_t)a.K * a.nq + 15) / 16);
    if (hasher == GLP_HASH_KECCAK25) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fri_verify_queries<GLP_HASH_KECCAK25>), dim3(nblocks), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fri_verify_queries<GLP_HASH_POSEIDON>), dim3(nblocks), dim3(256), 0, c->stream, a);
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}
// its status words, back on the host (a copy into pageable memory blocks its caller until the stream gets there)
int read_status(glp_ctx *c, const FVArgs &a, std::vector<u32> &hs) {
    hs.resize((size_t)a.K * a.nq);
    GLP_HIP(hipMemcpyAsync(hs.data(), a.status, hs.size() * 4, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}
// why[k] is empty for the proofs the host half accepted: for those the first failing check of the first failing query becomes the
// reason (reason(q, status word)); then the verdict and the reason of every proof go out
template <class Reason>
void write_verdicts(u32 K, u32 nq, const std::vector<u32> &hs, std::vector<std::string> &why, Reason reason, int32_t *status_out, char *reasons_out) {
    for (u32 k = 0; k < K; k++) {
        for (u32 q = 0; q < nq && why[k].empty(); q++)
            if (hs[(size_t)k * nq + q]) why[k] = reason(q, hs[(size_t)k * nq + q]);
        status_out[k] = why[k].empty() ? GLP_OK : GLP_ERR_PROVE;
        if (reasons_out) {
            char *o = reasons_out + (size_t)k * GLP_REASON_LEN;
            memset(o, 0, GLP_REASON_LEN);
            strncpy(o, why[k].c_str(), GLP_REASON_LEN - 1);
        }
    }
}

// ---- glp_verify_batch, step by step.  What one call holds:
struct VBatch {
    glp_ctx *c;
    const glp_circuit *cc;
    u32 K;
    const u64 *proofs;                  // the caller's, [K][L.total]
    u32 tstride = 0;                    // words of one per-proof table (FT_*)
    size_t prog_at = 0;                 // where the range program starts in the host block
    std::vector<u64> hv;                // the host block: the K tables, then the range program
    std::vector<std::string> why;       // per proof the reason of its rejection; empty: accepted so far
    u64 *dev_proofs = nullptr, *dev_hv = nullptr;
    u32 *dev_status = nullptr;          // [K][num_query_rounds]
};
// what the device's transcripts send back for the host's half of the check (one block, one copy), and the event behind that copy
struct DevFront {
    std::vector<u64> h_back;
    const u64 *h_chal = nullptr, *h_qpp = nullptr, *h_apow = nullptr, *h_zetas = nullptr;
    const u32 *h_err = nullptr;
    hipEvent_t ev_chal = nullptr;
    ~DevFront() { if (ev_chal) (void)hipEventDestroy(ev_chal); }
};
struct VTimes {         // GLP_BATCH_TRACE: milliseconds since the call began
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    double front = 0, up = 0, chal = 0, van = 0;
    double since() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); }
};

// one host block: the K per-proof tables (FT_*), then the range program of the plonk instance (tests/fri_restate.py::plonk_instance):
// every column of the four oracles at zeta (point 0), the Z columns also at g zeta (point 1)
constexpr size_t PLONK_PROG_BYTES = 15 * sizeof(u32);
void host_block(VBatch &b) {
    const Layout &L = b.cc->L;
    b.tstride = (FT_XIDX + b.cc->d.num_query_rounds + 3) & ~3u;
    b.prog_at = (size_t)b.K * b.tstride;
    u32 prog[15], leaf_off = 0;
    for (u32 o = 0; o < 4; o++) {
        prog[3 * o] = leaf_off; prog[3 * o + 1] = 0; prog[3 * o + 2] = L.oracle_cols[o];
        if (o == 2) { prog[12] = leaf_off; prog[13] = 0; prog[14] = b.cc->d.num_challenges; }
        leaf_off += L.leaf_len[o] + 4 * L.depth0;
    }
    static_assert(sizeof(prog) == PLONK_PROG_BYTES, "the range program of the plonk instance");
    b.why.assign(b.K, std::string());
    b.hv.assign(b.prog_at + (sizeof(prog) + 7) / 8, 0);
    memcpy(&b.hv[b.prog_at], prog, sizeof(prog));
}
// the host-transcript front, one proof per task on the context's pool: canonical form, transcript, proof of work, vanishing polynomial
// at zeta (verify_front); what the query rounds need of it goes into the proof's table
void front_on_host(VBatch &b) {
    const glp_circuit_desc &d = b.cc->d;
    ctx_host_pool(b.c).run(b.K, [&](size_t k) {
        VChal v;
        if (verify_front(*b.cc, b.proofs + k * b.cc->L.total, v) != GLP_OK) { b.why[k] = g_last_error; return; }
        u64 *o = &b.hv[k * b.tstride];
        auto put = [&](u32 at, const E &e) { o[at] = e.v.a; o[at + 1] = e.v.b; };
        put(FT_ALPHA, v.fri_alpha); put(FT_Z, v.zeta); put(FT_Z + 2, v.zeta_next); put(FT_RED, v.red0); put(FT_RED + 2, v.red1);
        for (u32 r = 0; r < d.num_reductions; r++) put(FT_BETAS + 2 * r, v.fri_betas[r]);
        for (u32 q = 0; q < d.num_query_rounds; q++) o[FT_XIDX + q] = v.x_index[q];
    });
}
// the device-transcript front, host side: the canonical-form scan alone, beside the upload
void canonical_on_host(VBatch &b) {
    ctx_host_pool(b.c).run(b.K, [&](size_t k) {
        if (verify_canonical(*b.cc, b.proofs + k * b.cc->L.total) != GLP_OK) b.why[k] = g_last_error;
    });
}
// the device-transcript front, device side, once the proofs are up: the K transcripts as the batch prover runs them (transcript_dev.h; the
// uploaded proofs are the image its kernels read), the tables packed on the device, and what the host's half of the check needs on its
// way back while the query rounds run (f.ev_chal: that copy has landed)
int front_on_device(VBatch &b, Scratch &sc, DevFront &f) {
    glp_ctx *c = b.c;
    const glp_circuit *cc = b.cc;
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const u32 K = b.K, nq = d.num_query_rounds, nred = d.num_reductions, nch = d.num_challenges, capn = 1u << d.cap_height;
    u64 *dev_proofs = b.dev_proofs;
    const u32 total_cols = L.oracle_cols[0] + L.oracle_cols[1] + L.oracle_cols[2] + L.oracle_cols[3];
    u64 *dch, *dev_apl, *dev_fap, *dev_fpp, *dev_betas, *dev_idx;
    GLP_TRY(sc.words(&dch, (size_t)K * DCH_WORDS));
    // betas | gammas, public-input hash, alpha powers, zetas, error bits: one block, one copy back
    const size_t w_chal = (size_t)K * 2 * MAXCH, w_qpp = (size_t)K * 3 * MAXCH, w_apow = (size_t)K * nch * 2, w_zetas = (size_t)K * 4, w_err = (K + 1) / 2;
    u64 *dev_back;
    GLP_TRY(sc.words(&dev_back, w_chal + w_qpp + w_apow + w_zetas + w_err));
    u64 *dev_chal = dev_back, *dev_qpp = dev_chal + w_chal, *dev_apow = dev_qpp + w_qpp, *dev_zetas = dev_apow + w_apow;
    u32 *dev_err = (u32 *)(dev_zetas + w_zetas);
    GLP_TRY(sc.words(&dev_apl, (size_t)K * nch * 2 * APL_WORDS));
    GLP_TRY(sc.words(&dev_fap, (size_t)K * 2 * total_cols));
    GLP_TRY(sc.words(&dev_fpp, (size_t)K * 10));
    GLP_TRY(sc.words(&dev_betas, (size_t)std::max<u32>(nred, 1) * K * 2));
    GLP_TRY(sc.words(&dev_idx, (size_t)K * nq));
    GLP_HIP(hipMemsetAsync(dev_back, 0, (w_chal + w_qpp + w_apow + w_zetas + w_err) * 8, c->stream));
    TrGeo g;
    g.dch = dch; g.image = dev_proofs; g.total = L.total; g.K = K; g.capn = capn; g.nch = nch;
    const dim3 tg((K + 15) / 16), tb(256);
    const size_t cap4 = (size_t)capn * 4;
    // a cap is "copied" from the image onto itself: source = image + offset with the proof stride, destination offset the same
    hipLaunchKernelGGL(k_tr_begin, tg, tb, 0, c->stream, g, cc->digest[0], cc->digest[1], cc->digest[2], cc->digest[3], L.pis, d.num_public_inputs,
                       dev_proofs + L.caps, L.total, L.caps, dev_chal, dev_qpp);
    hipLaunchKernelGGL(k_tr_alphas, tg, tb, 0, c->stream, g, dev_proofs + L.caps + cap4, L.total, L.caps + cap4, 2u, dev_apow, dev_apl);
    hipLaunchKernelGGL(k_tr_zeta, tg, tb, 0, c->stream, g, dev_proofs + L.caps + 2 * cap4, L.total, L.caps + 2 * cap4, d.degree_bits,
                       root_of_unity((int)d.degree_bits), dev_zetas, dev_err);
    OpenGeo og;
    memset(&og, 0, sizeof(og));
    for (int o = 0; o < 4; o++) og.cols[o] = L.oracle_cols[o];
    og.openings_off = L.openings; og.nch = nch; og.npp = d.num_partial_products; og.nopen = (u32)L.nopen;
    hipLaunchKernelGGL(k_tr_fri_alpha, tg, tb, 0, c->stream, g, og, dev_zetas, dev_fap, dev_fpp);
    for (u32 r = 0; r < nred; r++)
        hipLaunchKernelGGL(k_tr_beta, tg, tb, 0, c->stream, g, dev_proofs + L.fri_caps + r * cap4, L.total, L.fri_caps + r * cap4, dev_betas + (size_t)r * K * 2);
    hipLaunchKernelGGL(k_trv_final, tg, tb, 0, c->stream, g, L.final_poly, 2u * L.final_len);
    hipLaunchKernelGGL(k_trv_queries, tg, tb, 0, c->stream, g, d.proof_of_work_bits, L.pow, nq, (u64)1 << (d.degree_bits + d.rate_bits), dev_idx, dev_err);
    hipLaunchKernelGGL(k_trv_pack, dim3((K + 255) / 256), dim3(256), 0, c->stream, K, b.tstride, dev_fap, total_cols, dev_fpp, dev_betas, nred, dev_idx, nq, b.dev_hv);
    GLP_HIP(hipGetLastError());
    // what the host's half of the check needs comes back while the query rounds run
    f.h_back.resize(w_chal + w_qpp + w_apow + w_zetas + w_err);
    GLP_HIP(hipMemcpyAsync(f.h_back.data(), dev_back, f.h_back.size() * 8, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipEventCreateWithFlags(&f.ev_chal, hipEventDisableTiming));
    GLP_HIP(hipEventRecord(f.ev_chal, c->stream));
    f.h_chal = f.h_back.data(); f.h_qpp = f.h_chal + w_chal; f.h_apow = f.h_qpp + w_qpp; f.h_zetas = f.h_apow + w_apow; f.h_err = (const u32 *)(f.h_zetas + w_zetas);
    return GLP_OK;
}
// the FRI part of a proof, fri_caps | queries | final_poly | pow, is the FriProof layout the kernel reads (layer caps at offset 0); the
// circuit's constants / sigmas cap is shared, the three caps of a proof sit at its front
FVArgs plonk_query_args(const VBatch &b) {
    const glp_circuit *cc = b.cc;
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    const u32 nred = d.num_reductions, capn = 1u << d.cap_height;
    FVArgs a;
    memset(&a, 0, sizeof(a));
    a.proofs = b.dev_proofs + L.fri_caps; a.table = b.dev_hv; a.prog = (const u32 *)(b.dev_hv + b.prog_at); a.status = b.dev_status;
    a.total = L.total; a.queries = L.queries - L.fri_caps; a.query_stride = L.query_stride; a.final_poly = L.final_poly - L.fri_caps;
    a.tstride = b.tstride; a.nq = d.num_query_rounds; a.K = b.K; a.lgN = d.degree_bits + d.rate_bits; a.cap_height = d.cap_height; a.depth0 = L.depth0; a.nred = nred;
    a.final_len = L.final_len; a.nor = 4; a.npts = 2; a.nranges[0] = 4; a.nranges[1] = 1;
    a.caps[0] = cc->cs->digests + 4 * merkle_cap_offset((size_t)1 << a.lgN, (int)d.cap_height);
    for (u32 o = 1; o < 4; o++) { a.caps[o] = b.dev_proofs + L.caps + (size_t)(o - 1) * capn * 4; a.cap_stride[o] = (u32)L.total; }
    for (u32 o = 0; o < 4; o++) a.leaf_len[o] = L.leaf_len[o];
    for (u32 r = 0; r < nred; r++) { a.ab[r] = d.reduction_arity_bits[r]; a.step_depth[r] = L.step_depth[r]; a.gA[r] = root_of_unity((int)d.reduction_arity_bits[r]); }
    a.wN = root_of_unity((int)a.lgN);
    return a;
}
// the device-transcript front, host side again, with the challenges back: same order of checks as verify_front -- canonical form
// (canonical_on_host), proof of work, then the identity at zeta
void identity_on_host(VBatch &b, const DevFront &f) {
    const u32 nch = b.cc->d.num_challenges;
    ctx_host_pool(b.c).run(b.K, [&](size_t k) {
        if (!b.why[k].empty()) return;
        if (f.h_err[k] & 8u) { set_error(GLP_ERR_PROVE, "Invalid proof of work witness."); b.why[k] = g_last_error; return; }
        u64 alphas[MAXCH] = {0, 0, 0, 0};
        for (u32 i = 0; i < nch; i++) alphas[i] = f.h_apow[(k * nch + i) * 2 + 1];
        const E zeta(e_make(f.h_zetas[4 * k], f.h_zetas[4 * k + 1]));
        if (verify_vanishing(*b.cc, b.proofs + k * b.cc->L.total, &f.h_chal[k * 2 * MAXCH], &f.h_chal[k * 2 * MAXCH + MAXCH], alphas, zeta,
                             &f.h_qpp[k * 3 * MAXCH + 2 * MAXCH]) != GLP_OK)
            b.why[k] = g_last_error;
    });
}
void trace_line(bool dev_tr, u32 K, const VTimes &t) {
    if (dev_tr) fprintf(stderr, "[glp_verify_batch K=%u dev] canonical scan %.3f ms | upload done at %.3f | challenges back at %.3f | identity at zeta done at %.3f | query rounds done at %.3f ms\n",
                        K, t.front, t.up, t.chal, t.van, t.since());
    else fprintf(stderr, "[glp_verify_batch K=%u] host half %.3f ms | upload done at %.3f | query rounds done at %.3f ms\n", K, t.front, t.up, t.since());
}
}  // namespace

extern "C" int glp_verify_batch(glp_ctx *c, const glp_circuit *cc, uint32_t K, const uint64_t *proofs, int32_t *status_out, char *reasons_out) {
    GLP_REQUIRE(c && cc && proofs && status_out, "null argument");
    GLP_REQUIRE(cc->ctx == c, "circuit belongs to another context");
    GLP_REQUIRE(K >= 1 && K <= 65536, "glp_verify_batch: batch of %u proofs outside 1..65536", K);
    GLP_TRY(bind(c));
    const glp_circuit_desc &d = cc->d;
    const Layout &L = cc->L;
    GLP_REQUIRE(L.total <= 0xFFFFFFFFu, "glp_verify_batch: proofs of %zu words (the query kernel takes a cap stride below 2^32 words)", L.total);
    VBatch b = {c, cc, K, proofs};
    host_block(b);
    Scratch sc(c);
    GLP_TRY(sc.words(&b.dev_proofs, (size_t)K * L.total));
    GLP_TRY(sc.words(&b.dev_hv, b.hv.size()));
    GLP_TRY(sc.array(&b.dev_status, (size_t)K * d.num_query_rounds));
    const bool trace = getenv("GLP_BATCH_TRACE") != nullptr;
    VTimes t;
    u64 *dev_proofs = b.dev_proofs, *dev_prog = b.dev_hv + b.prog_at;
    const u64 *host_prog = &b.hv[b.prog_at];
    const size_t proof_bytes = (size_t)K * L.total * 8;
    Uploader up(c, [=] {        // the proofs, and behind them the range program: nothing waits for it on the calling thread
        hipError_t e = hipMemcpyAsync(dev_proofs, proofs, proof_bytes, hipMemcpyHostToDevice, c->stream);
        return e != hipSuccess ? e : hipMemcpyAsync(dev_prog, host_prog, PLONK_PROG_BYTES, hipMemcpyHostToDevice, c->stream);
    });
    // PoseidonGoldilocksConfig: the K transcripts run on the device, as the batch prover's do.  The host keeps the canonical-form scan
    // (beside the upload) and the vanishing-polynomial identity (beside the query rounds).  KeccakGoldilocksConfig, or
    // GLP_VERIFY_HOST_TRANSCRIPT=1: everything of verify_front on host threads.
    const bool dev_tr = d.hasher == GLP_HASH_POSEIDON && getenv("GLP_VERIFY_HOST_TRANSCRIPT") == nullptr;
    DevFront f;
    if (dev_tr) canonical_on_host(b); else front_on_host(b);
    t.front = t.since();
    GLP_TRY(up.done());
    t.up = t.since();
    // Proofs the host half already rejected still ride along (their slots hold zero challenges and every index is in range); their
    // device status is ignored.
    if (dev_tr) GLP_TRY(front_on_device(b, sc, f));
    else GLP_HIP(hipMemcpyAsync(b.dev_hv, b.hv.data(), b.prog_at * 8, hipMemcpyHostToDevice, c->stream));
    // every query round of every proof in one launch
    const FVArgs a = plonk_query_args(b);
    GLP_TRY(launch_queries(c, (int)d.hasher, "verify_queries", a));
    if (dev_tr) {
        GLP_HIP(hipEventSynchronize(f.ev_chal));
        t.chal = t.since();
        identity_on_host(b, f);
        t.van = t.since();
    }
    // (enqueued only now: the identity at zeta ran beside the query rounds)
    std::vector<u32> hs;
    GLP_TRY(read_status(c, a, hs));
    if (trace) trace_line(dev_tr, K, t);
    write_verdicts(K, d.num_query_rounds, hs, b.why, [](u32 q, u32 word) { query_failure(q, word); return g_last_error; }, status_out, reasons_out);
    return GLP_OK;
}

extern "C" int glp_verify(const glp_circuit *cc, const uint64_t *proof_words) {
    GLP_REQUIRE(cc && proof_words, "null argument");
    return verify_impl(*cc, proof_words);
}
extern "C" int glp_verify_n(const glp_circuit *cc, const uint64_t *proof_words, size_t num_words) {
    GLP_REQUIRE(cc && proof_words, "null argument");
    return verify_impl_n(*cc, proof_words, num_words);
}

#include "fri_verify.inc"
