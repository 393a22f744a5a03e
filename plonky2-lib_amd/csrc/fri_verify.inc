// fri_verify.inc -- glp_fri_verify*: plonky2 `fri/verifier.rs::verify_fri_proof` for any FriInstanceInfo the prover side (glp_fri_*,
// fri_openings.inc) accepts, for K proofs of one instance in one launch.  Included by verifier.hip after glp_verify_batch, with which
// it shares the query-round kernel (k_fri_verify_queries, verify_dev.h: glp_verify_batch runs it on the plonk instance) and what
// surrounds its launch (common.h: Scratch; verifier.hip: Uploader, launch_queries, read_status, write_verdicts): per proof the canonical-form
// scan and (one-call form) the transcript run on the context's host threads beside the upload of the proofs; every query round of
// every proof is one launch.  The verifier holds no glp_batch, only caps: it has its own description (glp_fri_verify_desc) and shares
// the shape rules with the prover through fri_shape.h.
// The Python restatement the tests hold it to is tests/fri_restate.py::verify_fri_proof; the check numbers are that function's.
#include <stdarg.h>
#include "fri_shape.h"

namespace {
// red_b = sum_j alpha^j opening_{b,j} of every (point, proof) from the uploaded openings into the table: the shape of k_fri_table
// (fri_kernels.inc: one workgroup per (point, proof)), without its alpha-power output.  Thread t sums the openings t, t + 256, ..
struct FRArgs {
    const u64 *open;        // [K][nopen][2]
    u64 *table;             // [K][tstride]; reads FT_ALPHA, writes FT_RED + 2 b
    size_t nopen;
    u32 tstride, first[GLP_FRI_MAX_POINTS], len[GLP_FRI_MAX_POINTS];
};
__global__ __launch_bounds__(256) void k_fri_verify_red(FRArgs a) {
    const u32 b = blockIdx.y, k = blockIdx.x, t = threadIdx.x, len = a.len[b];      // grid (K, points): K may reach 65536, one past what grid.y holds
    u64 *tb = a.table + (size_t)k * a.tstride;
    const u64 *op = a.open + ((size_t)k * a.nopen + a.first[b]) * 2;
    const ext2 alpha = rd2(tb + FT_ALPHA);
    ext2 a256 = alpha;
#pragma unroll
    for (int i = 0; i < 8; i++) a256 = e_sqr(a256);
    ext2 part = e_from(0);
    if (t < len)
        for (long long j = (long long)(((len - 1 - t) >> 8) << 8) + t; j >= 0; j -= 256) part = e_add(e_mul(part, a256), rd2(op + 2 * j));
    part = e_mul(part, e_pow(alpha, (u64)t));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part = e_add(part, e_make(shfl_xor64(part.a, m), shfl_xor64(part.b, m)));
    __shared__ u64 sh[4][2];
    if ((t & 63) == 0) { sh[t >> 6][0] = part.a; sh[t >> 6][1] = part.b; }
    __syncthreads();
    if (t == 0) {
        ext2 s = e_make(sh[0][0], sh[0][1]);
        for (int i = 1; i < 4; i++) s = e_add(s, e_make(sh[i][0], sh[i][1]));
        tb[FT_RED + 2 * b] = s.a;
        tb[FT_RED + 2 * b + 1] = s.b;
    }
}

// the description, checked and laid out: word offsets inside the FriProof (the caps start at 0), the range program
struct FVPlan {
    u32 nor = 0, npts = 0, lgN = 0, cap_height = 0, capn = 0, depth0 = 0, nred = 0, nq = 0, final_len = 0, pow_bits = 0;
    int hasher = GLP_HASH_POSEIDON;
    u32 leaf_len[GLP_FRI_MAX_ORACLES], shared[GLP_FRI_MAX_ORACLES];
    u32 ab[16], step_depth[16];
    u32 first[GLP_FRI_MAX_POINTS], len[GLP_FRI_MAX_POINTS], nranges[GLP_FRI_MAX_POINTS];
    std::vector<u32> prog;
    size_t o_queries = 0, query_stride = 0, o_final = 0, o_pow = 0, total = 0, nopen = 0;
};
int fv_plan(const glp_fri_verify_desc *d, FVPlan &p) {
    GLP_REQUIRE(d, "desc is null");
    GLP_TRY(fri_shape_counts(d->num_oracles, d->oracles, d->num_points, d->points));
    GLP_REQUIRE(d->hasher == GLP_HASH_POSEIDON || d->hasher == GLP_HASH_KECCAK25, "hasher = %u is not one of GLP_HASH_*", d->hasher);
    GLP_REQUIRE(d->log_n <= 32 && d->rate_bits <= 32 && d->log_n + d->rate_bits >= 1 && d->log_n + d->rate_bits <= 32,
                "log_n = %u, rate_bits = %u: log_n + rate_bits outside 1..32", d->log_n, d->rate_bits);
    p.lgN = d->log_n + d->rate_bits;
    GLP_REQUIRE(d->cap_height <= p.lgN, "cap_height = %u above log_n + rate_bits = %u", d->cap_height, p.lgN);
    u32 ncols[GLP_FRI_MAX_ORACLES];
    for (u32 o = 0; o < d->num_oracles; o++) {
        GLP_REQUIRE(d->oracles[o].num_cols <= 0x7FFFFFFFu - GLP_SALT_SIZE, "oracles[%u].num_cols = %u is too large", o, d->oracles[o].num_cols);
        ncols[o] = d->oracles[o].num_cols;
    }
    GLP_TRY(fri_shape_rules(ncols, d->num_oracles, d->log_n, d->rate_bits, d->cap_height, d->num_points, d->points, false, d->num_reductions,
                            d->reduction_arity_bits, d->proof_of_work_bits, d->num_query_rounds));
    p.nor = d->num_oracles; p.npts = d->num_points; p.cap_height = d->cap_height; p.capn = 1u << d->cap_height; p.depth0 = p.lgN - d->cap_height;
    p.nred = d->num_reductions; p.nq = d->num_query_rounds; p.pow_bits = d->proof_of_work_bits; p.hasher = (int)d->hasher;
    for (u32 o = 0; o < p.nor; o++) {
        p.leaf_len[o] = ncols[o] + (d->oracles[o].salted ? GLP_SALT_SIZE : 0);
        p.shared[o] = d->oracles[o].shared != 0;
    }
    for (u32 r = 0; r < p.nred; r++) p.ab[r] = d->reduction_arity_bits[r];
    const FriProofLayout f = fri_proof_layout(p.lgN, d->rate_bits, d->cap_height, p.leaf_len, p.nor, p.ab, p.nred, p.nq);
    for (u32 o = 0; o < p.nor; o++) GLP_REQUIRE(f.leaf_off[o] <= 0x7FFFFFFFu, "oracles: a query record of more than 2^31 words");
    for (u32 r = 0; r < p.nred; r++) p.step_depth[r] = f.step_depth[r];
    p.query_stride = f.query_stride; p.final_len = f.final_len;
    p.o_queries = f.queries; p.o_final = f.final_poly; p.o_pow = f.pow; p.total = f.total;
    for (u32 b = 0; b < p.npts; b++) {
        const glp_fri_point &pt = d->points[b];
        p.first[b] = (u32)p.nopen; p.len[b] = 0; p.nranges[b] = pt.num_ranges;
        for (u32 r = 0; r < pt.num_ranges; r++) {
            const glp_fri_range &rg = pt.ranges[r];
            p.prog.push_back((u32)f.leaf_off[rg.oracle]); p.prog.push_back(rg.col_begin); p.prog.push_back(rg.num_cols);
            p.len[b] += rg.num_cols;
        }
        p.nopen += p.len[b];
    }
    return GLP_OK;
}

// field elements (and Poseidon digests) must be canonical; a KeccakHash<25> digest is 25 bytes in a 4-word slot.  -> "" or the reason
bool fv_digests_ok(int hasher, const u64 *dig, size_t count, size_t *at) {
    if (hasher != GLP_HASH_KECCAK25) { *at = first_noncanonical(dig, 4 * count); return *at == 4 * count; }
    for (size_t i = 0; i < count; i++) if (dig[4 * i + 3] > 0xFF) { *at = 4 * i; return false; }
    return true;
}
std::string fv_fmt(const char *fmt, ...) {
    char buf[GLP_REASON_LEN];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}
std::string fv_canonical(const FVPlan &p, const u64 *proof) {
    size_t at = 0;
    if (p.hasher != GLP_HASH_KECCAK25) {
        at = first_noncanonical(proof, p.total);
        return at == p.total ? std::string() : fv_fmt("proof word %zu is not a canonical field element [check 1]", at);
    }
    auto fields = [&](size_t off, size_t n) { at = off + first_noncanonical(proof + off, n); return at == off + n; };
    auto digests = [&](size_t off, size_t n) { const bool ok = fv_digests_ok(p.hasher, proof + off, n, &at); at += off; return ok; };
    bool field_bad = false;
    auto scan = [&]() {
        if (!digests(0, (size_t)p.nred * p.capn)) return false;
        for (u32 q = 0; q < p.nq; q++) {
            size_t o = p.o_queries + (size_t)q * p.query_stride;
            for (u32 k = 0; k < p.nor; k++) {
                if (!fields(o, p.leaf_len[k])) { field_bad = true; return false; }
                o += p.leaf_len[k];
                if (!digests(o, p.depth0)) return false;
                o += 4 * (size_t)p.depth0;
            }
            for (u32 r = 0; r < p.nred; r++) {
                if (!fields(o, (size_t)2 << p.ab[r])) { field_bad = true; return false; }
                o += (size_t)2 << p.ab[r];
                if (!digests(o, p.step_depth[r])) return false;
                o += 4 * (size_t)p.step_depth[r];
            }
        }
        if (!fields(p.o_final, 2 * (size_t)p.final_len + 1)) { field_bad = true; return false; }
        return true;
    };
    if (scan()) return std::string();
    return field_bad ? fv_fmt("proof word %zu is not a canonical field element [check 1]", at) : fv_fmt("digest at word %zu is longer than 25 bytes [check 1]", at);
}

inline void fv_resume(Challenger &ch, const u64 *state, const u64 *pending, u32 npending) {
    memcpy(ch.st, state, 96);
    for (u32 i = 0; i < npending; i++) ch.in[i] = pending[i];
    ch.nin = (int)npending;
    // as in glp_fri_prove: with nothing pending the caller's last observation permuted and refilled the output buffer
    if (npending == 0) { memcpy(ch.out, ch.st, 64); ch.nout = 8; }
}

std::string fv_query_reason(u32 q, u32 word) {
    const u32 check = word & 0xFF, detail = word >> 8;
    switch (check) {
    case FV_POINT: return fv_fmt("query point equals opening point %u (query %u) [check 3]", detail, q);
    case FV_INITIAL: return fv_fmt("Invalid Merkle proof (query %u, initial tree %u) [check 4]", q, detail);
    case FV_FOLD: return fv_fmt("FRI consistency check failed (query %u, reduction %u) [check 5]", q, detail);
    case FV_LAYER: return fv_fmt("Invalid Merkle proof (query %u, reduction %u) [check 6]", q, detail);
    default: return fv_fmt("Final polynomial evaluation is invalid (query %u) [check 7]", q);
    }
}

// alphas != nullptr: the stepped form (the caller's challenges); else the one-call form (the library's transcript from states / pending)
int fri_verify_core(glp_ctx *c, const glp_fri_verify_desc *d, u32 K, const u64 *points, const u64 *const *caps, const u64 *openings, const u64 *proofs,
                    const u64 *states, const u64 *pending, u32 npending, const u64 *alphas, const u64 *betas, const u64 *indices,
                    int32_t *status_out, char *reasons_out) {
    FVPlan p;
    GLP_TRY(fv_plan(d, p));
    GLP_REQUIRE(K >= 1 && K <= 65536, "num_proofs = %u outside 1..65536", K);
    GLP_REQUIRE(points, "points is null");
    GLP_REQUIRE(caps, "caps is null");
    for (u32 o = 0; o < p.nor; o++) GLP_REQUIRE(caps[o], "caps[%u] is null", o);
    GLP_REQUIRE(openings, "openings is null");
    GLP_REQUIRE(proofs, "proofs is null");
    GLP_REQUIRE(status_out, "status_out is null");
    const bool stepped = alphas != nullptr;
    const u32 nq = p.nq, nred = p.nred, npts = p.npts, capn4 = p.capn * 4;
    const u64 N = (u64)1 << p.lgN;
    if (stepped) {
        GLP_REQUIRE(indices, "indices is null");
        GLP_REQUIRE(betas || nred == 0, "betas is null");
    } else {
        GLP_REQUIRE(states, "sponge_states is null");
        GLP_REQUIRE(npending < 8, "num_pending = %u (the rate is 8)", npending);
        GLP_REQUIRE(pending || npending == 0, "pending_inputs is null");
    }
    GLP_TRY(bind(c));
    const u32 tstride = (FT_XIDX + nq + 3) & ~3u;
    // one host block, one copy: the K tables, the caps (shared: one, else K), the range program
    size_t cap_at[GLP_FRI_MAX_ORACLES], words = (size_t)K * tstride;
    for (u32 o = 0; o < p.nor; o++) { cap_at[o] = words; words += (size_t)(p.shared[o] ? 1 : K) * capn4; }
    const size_t prog_at = words;
    words += (p.prog.size() + 1) / 2;
    std::vector<u64> hv(words, 0);
    for (u32 o = 0; o < p.nor; o++) memcpy(&hv[cap_at[o]], caps[o], (size_t)(p.shared[o] ? 1 : K) * capn4 * 8);
    memcpy(&hv[prog_at], p.prog.data(), p.prog.size() * 4);

    Scratch sc(c);
    u64 *dev_proofs = nullptr, *dev_hv = nullptr, *dev_open = nullptr;
    u32 *dev_status = nullptr;
    GLP_TRY(sc.words(&dev_proofs, (size_t)K * p.total));
    GLP_TRY(sc.words(&dev_hv, hv.size()));
    GLP_TRY(sc.array(&dev_status, (size_t)K * nq));
    if (stepped) GLP_TRY(sc.words(&dev_open, (size_t)K * p.nopen * 2));
    // the proofs (and, stepped, the openings) go up on a thread of their own while the host half runs
    const size_t proof_bytes = (size_t)K * p.total * 8, open_bytes = (size_t)K * p.nopen * 16;
    Uploader up(c, [=] {
        hipError_t e = hipMemcpyAsync(dev_proofs, proofs, proof_bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && stepped) e = hipMemcpyAsync(dev_open, openings, open_bytes, hipMemcpyHostToDevice, c->stream);
        return e;
    });
    // ---- host half, one proof per task: canonical form of everything the proof brings, then the challenges
    std::vector<std::string> why(K);
    std::vector<int> arg_err(K, 0);         // stepped: 1 alpha, 2 beta, 3 index
    std::string shared_why;
    for (u32 o = 0; o < p.nor && shared_why.empty(); o++) {
        size_t at;
        if (p.shared[o] && !fv_digests_ok(p.hasher, caps[o], p.capn, &at)) shared_why = fv_fmt("caps[%u] (shared) word %zu is not canonical [check 1]", o, at);
    }
    ctx_host_pool(c).run(K, [&](size_t k) {
        const u64 *proof = proofs + k * p.total, *op = openings + k * p.nopen * 2, *z = points + k * npts * 2;
        u64 *tb = &hv[k * tstride];
        size_t at;
        why[k] = shared_why;
        for (u32 o = 0; o < p.nor && why[k].empty(); o++)
            if (!p.shared[o] && !fv_digests_ok(p.hasher, caps[o] + k * capn4, p.capn, &at)) why[k] = fv_fmt("caps[%u] word %zu is not canonical [check 1]", o, at);
        if (why[k].empty() && (at = first_noncanonical(z, 2 * (size_t)npts)) != 2 * (size_t)npts) why[k] = fv_fmt("points[%zu] is not canonical [check 1]", at / 2);
        if (why[k].empty() && (at = first_noncanonical(op, 2 * p.nopen)) != 2 * p.nopen) why[k] = fv_fmt("opening %zu is not canonical [check 1]", at / 2);
        if (why[k].empty()) why[k] = fv_canonical(p, proof);
        if (stepped) {
            // the caller's challenges are arguments: a bad one is an error of the call, whatever the proof
            if (first_noncanonical(alphas + 2 * k, 2) != 2) { arg_err[k] = 1; return; }
            if (first_noncanonical(betas + 2 * k * nred, 2 * (size_t)nred) != 2 * (size_t)nred) { arg_err[k] = 2; return; }
            for (u32 q = 0; q < nq; q++) if (indices[k * nq + q] >= N) { arg_err[k] = 3; return; }
        }
        if (!why[k].empty()) return;        // rides along with a zero table: every index in range, its device status ignored
        ext2 alpha;
        if (stepped) {
            alpha = e_make(alphas[2 * k], alphas[2 * k + 1]);
            for (u32 r = 0; r < 2 * nred; r++) tb[FT_BETAS + r] = betas[2 * k * nred + r];
            for (u32 q = 0; q < nq; q++) tb[FT_XIDX + q] = indices[k * nq + q];
        } else {
            // fri/verifier.rs order: alpha; per reduction observe the cap, draw beta; the final polynomial; the witness; the response; the indices
            Challenger ch(p.hasher);
            fv_resume(ch, states + k * 12, pending + k * npending, npending);
            alpha = ch.get_ext();
            for (u32 r = 0; r < nred; r++) {
                ch.observe_hashes(proof + (size_t)r * capn4, p.capn);
                const ext2 beta = ch.get_ext();
                tb[FT_BETAS + 2 * r] = beta.a; tb[FT_BETAS + 2 * r + 1] = beta.b;
            }
            ch.observe(proof + p.o_final, 2 * (size_t)p.final_len);
            ch.observe(proof + p.o_pow, 1);
            const u64 resp = ch.get();
            if (p.pow_bits && (resp >> (64 - p.pow_bits)) != 0) {
                why[k] = "Invalid proof of work witness. [check 2]";
                for (u32 r = 0; r < 2 * nred; r++) tb[FT_BETAS + r] = 0;
                return;
            }
            for (u32 q = 0; q < nq; q++) tb[FT_XIDX + q] = ch.get() % N;
            // PrecomputedReducedOpenings, beside the transcript
            for (u32 b = 0; b < npts; b++) {
                ext2 red = e_from(0);
                const u64 *o = op + 2 * (size_t)p.first[b];
                for (size_t j = p.len[b]; j-- > 0;) red = e_add(e_mul(red, alpha), e_make(o[2 * j], o[2 * j + 1]));
                tb[FT_RED + 2 * b] = red.a; tb[FT_RED + 2 * b + 1] = red.b;
            }
        }
        tb[FT_ALPHA] = alpha.a; tb[FT_ALPHA + 1] = alpha.b;
        for (u32 b = 0; b < 2 * npts; b++) tb[FT_Z + b] = z[b];
    });
    GLP_TRY(up.done());
    for (u32 k = 0; k < K; k++) {
        GLP_REQUIRE(arg_err[k] != 1, "alphas[%u] is not canonical", k);
        GLP_REQUIRE(arg_err[k] != 2, "betas[%u] holds a word that is not canonical", k);
        GLP_REQUIRE(arg_err[k] != 3, "indices[%u] holds an index outside the LDE domain (N = %llu)", k, (unsigned long long)N);
    }
    // ---- device half: every query round of every proof in one launch
    GLP_HIP(hipMemcpyAsync(dev_hv, hv.data(), hv.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (stepped) {
        FRArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.open = dev_open; ra.table = dev_hv; ra.nopen = p.nopen; ra.tstride = tstride;
        for (u32 b = 0; b < npts; b++) { ra.first[b] = p.first[b]; ra.len[b] = p.len[b]; }
        hipLaunchKernelGGL(k_fri_verify_red, dim3(K, npts), dim3(256), 0, c->stream, ra);
        GLP_HIP(hipGetLastError());
    }
    FVArgs a;
    memset(&a, 0, sizeof(a));
    a.proofs = dev_proofs; a.table = dev_hv; a.prog = (const u32 *)(dev_hv + prog_at); a.status = dev_status;
    a.total = p.total; a.queries = p.o_queries; a.query_stride = p.query_stride; a.final_poly = p.o_final;
    a.tstride = tstride; a.nq = nq; a.K = K; a.lgN = p.lgN; a.cap_height = p.cap_height; a.depth0 = p.depth0; a.nred = nred; a.final_len = p.final_len;
    a.nor = p.nor; a.npts = npts;
    for (u32 o = 0; o < p.nor; o++) { a.caps[o] = dev_hv + cap_at[o]; a.cap_stride[o] = p.shared[o] ? 0 : capn4; a.leaf_len[o] = p.leaf_len[o]; }
    for (u32 b = 0; b < npts; b++) a.nranges[b] = p.nranges[b];
    for (u32 r = 0; r < nred; r++) { a.ab[r] = p.ab[r]; a.step_depth[r] = p.step_depth[r]; a.gA[r] = root_of_unity((int)p.ab[r]); }
    a.wN = root_of_unity((int)p.lgN);
    GLP_TRY(launch_queries(c, p.hasher, "fri_verify_queries", a));
    std::vector<u32> hs;
    GLP_TRY(read_status(c, a, hs));
    write_verdicts(K, nq, hs, why, fv_query_reason, status_out, reasons_out);
    return GLP_OK;
}
}  // namespace

extern "C" {
size_t glp_fri_verify_proof_words(const glp_fri_verify_desc *d) {
    FVPlan p;
    return fv_plan(d, p) == GLP_OK ? p.total : 0;
}
size_t glp_fri_verify_num_openings(const glp_fri_verify_desc *d) {
    FVPlan p;
    return fv_plan(d, p) == GLP_OK ? p.nopen : 0;
}
int glp_fri_verify_many(glp_ctx *c, const glp_fri_verify_desc *d, uint32_t num_proofs, const uint64_t *points, const uint64_t *const *caps,
                        const uint64_t *openings, const uint64_t *proofs, const uint64_t *sponge_states, const uint64_t *pending_inputs,
                        uint32_t num_pending, int32_t *status_out, char *reasons_out) {
    GLP_REQUIRE(c, "ctx is null");
    return fri_verify_core(c, d, num_proofs, points, caps, openings, proofs, sponge_states, pending_inputs, num_pending, nullptr, nullptr, nullptr, status_out,
                           reasons_out);
}
int glp_fri_verify_queries_many(glp_ctx *c, const glp_fri_verify_desc *d, uint32_t num_proofs, const uint64_t *points, const uint64_t *const *caps,
                                const uint64_t *openings, const uint64_t *proofs, const uint64_t *alphas, const uint64_t *betas, const uint64_t *indices,
                                int32_t *status_out, char *reasons_out) {
    GLP_REQUIRE(c, "ctx is null");
    GLP_REQUIRE(alphas, "alphas is null");
    return fri_verify_core(c, d, num_proofs, points, caps, openings, proofs, nullptr, nullptr, 0, alphas, betas, indices, status_out, reasons_out);
}
int glp_fri_verify(glp_ctx *c, const glp_fri_verify_desc *d, const uint64_t *const *caps, const uint64_t *openings, const uint64_t *proof,
                   const uint64_t sponge_state[12], const uint64_t *pending_inputs, uint32_t num_pending) {
    GLP_REQUIRE(c, "ctx is null");
    GLP_REQUIRE(d, "desc is null");
    GLP_TRY(fri_shape_counts(d->num_oracles, d->oracles, d->num_points, d->points));
    u64 z[2 * GLP_FRI_MAX_POINTS];
    for (u32 b = 0; b < d->num_points; b++) { z[2 * b] = d->points[b].point[0]; z[2 * b + 1] = d->points[b].point[1]; }
    int32_t status = GLP_OK;
    char reason[GLP_REASON_LEN];
    GLP_TRY(fri_verify_core(c, d, 1, z, caps, openings, proof, sponge_state, pending_inputs, num_pending, nullptr, nullptr, nullptr, &status, reason));
    return status == GLP_OK ? GLP_OK : set_error(GLP_ERR_PROVE, "%s", reason);
}
}  // extern "C"
