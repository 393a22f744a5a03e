// fri_verify.inc -- glp_fri_verify*: plonky2 `fri/verifier.rs::verify_fri_proof` for any FriInstanceInfo the prover side (glp_fri_*,
// fri_openings.inc) accepts, for K proofs of one instance in one launch.  Included by verifier.hip after glp_verify_batch, whose
// structure it mirrors: per proof the canonical-form scan and (one-call form) the transcript run on the context's host threads
// beside the upload of the proofs; every query round of every proof is one launch of k_fri_verify_queries, the generic sibling of
// k_verify_queries (same launch shape, same helpers: verify_dev.h).  The verifier holds no glp_batch, only caps: it has its own
// description (glp_fri_verify_desc) and shares the shape rules with the prover through fri_shape.h.
// The Python restatement the tests hold it to is tests/fri_restate.py::verify_fri_proof; the check numbers are that function's.
#include <stdarg.h>
#include "fri_shape.h"

namespace {
// per-proof table, one stride per proof (the `vchal` style): alpha, z_b, red_b = sum_j alpha^j opening_{b,j}, betas (ext each), x_index[nq]
constexpr u32 FT_ALPHA = 0, FT_Z = 2, FT_RED = FT_Z + 2 * GLP_FRI_MAX_POINTS, FT_BETAS = FT_RED + 2 * GLP_FRI_MAX_POINTS, FT_XIDX = FT_BETAS + 32;
// status word of one (proof, query): 0 = accepted, else check | detail << 8 (detail: oracle for 4, point for 3, reduction for 5 and 6)
constexpr u32 FV_POINT = 3, FV_INITIAL = 4, FV_FOLD = 5, FV_LAYER = 6, FV_FINAL = 7;

struct FVArgs {
    const u64 *proofs;      // [K][total]
    const u64 *table;       // [K][tstride]
    const u32 *prog;        // the range program, shared by all proofs: per range (leaf offset in the query record, col_begin, num_cols), points in order
    const u64 *caps[GLP_FRI_MAX_ORACLES];       // oracle o of proof k: caps[o] + k * cap_stride[o]
    u32 *status;            // [K][nq]
    size_t total, queries, query_stride, final_poly;
    u32 tstride, nq, K, lgN, cap_height, depth0, nred, final_len, nor, npts;
    u32 leaf_len[GLP_FRI_MAX_ORACLES], cap_stride[GLP_FRI_MAX_ORACLES];     // polynomials + salts; 0 for a shared cap, else 4 << cap_height
    u32 nranges[GLP_FRI_MAX_POINTS];
    u32 ab[16], step_depth[16];
    u64 wN, gA[16];         // root_of_unity(lgN), root_of_unity(ab[r])
};

template <int HASHER>
__global__ __launch_bounds__(256) void k_fri_verify_queries(FVArgs a) {
    const int tid = threadIdx.x, l = tid & 15, lane = tid & 63, gb = lane & ~15;
    const size_t grp0 = (size_t)blockIdx.x * 16 + (tid >> 4), ngrp = (size_t)a.K * a.nq;
    const bool live = grp0 < ngrp;
    const size_t grp = live ? grp0 : 0;                   // idle groups redo group 0 (the shuffles need every lane) and write nothing
    const u32 k = (u32)(grp / a.nq), q = (u32)(grp % a.nq);
    const u64 *proof = a.proofs + (size_t)k * a.total, *tb = a.table + (size_t)k * a.tstride;
    const u64 *rec = proof + a.queries + (size_t)q * a.query_stride;
    const u64 *w = rec;
    size_t x_index = (size_t)tb[FT_XIDX + q];
    const ext2 alpha = rd2(tb + FT_ALPHA);
    const u32 capn4 = 4u << a.cap_height;
    u32 code = 0;
#define FV_FAIL(C, DETAIL) do { if (code == 0) code = (C) | ((u32)(DETAIL) << 8); } while (0)
    // ---- initial trees: the path covers the whole leaf, salts included; the evaluations stay where they are in the proof image
    for (u32 o = 0; o < a.nor; o++) {
        const u32 leaf_len = a.leaf_len[o];
        const u64 *cap = a.caps[o] + (size_t)k * a.cap_stride[o];
        if (merkle_bad<HASHER>(w, leaf_len, x_index, w + leaf_len, a.depth0, cap, l, gb)) FV_FAIL(FV_INITIAL, o);
        w += leaf_len + 4 * (size_t)a.depth0;
    }
    // ---- fri_combine_initial: sum <- sum alpha^(len_b) + (sum_j alpha^j eval_{b,j} - red_b) / (x - z_b), j across the point's ranges in order
    ext2 a16 = alpha;
#pragma unroll
    for (int i = 0; i < 4; i++) a16 = e_sqr(a16);
    const ext2 al = e_pow(alpha, (u64)l);
    u64 subgroup_x = mul(GEN, dvpow(a.wN, (u64)(__brevll((unsigned long long)x_index) >> (64 - a.lgN))));
    ext2 old_eval = e_from(0);
    {
        const u32 *pe = a.prog;
        for (u32 b = 0; b < a.npts; b++) {
            ext2 mine = e_from(0), off = e_from(1);       // this lane's share of sum_j alpha^j eval_j; alpha^(polynomials of the point so far)
            for (u32 i = 0; i < a.nranges[b]; i++, pe += 3) {
                const u32 ncols = pe[2];
                const u64 *ev = rec + pe[0] + pe[1];
                ext2 part = e_from(0);                    // lane l: sum_i ev[l + 16 i] (alpha^16)^i, Horner from the top
                if ((u32)l < ncols)
                    for (int j = (int)(((ncols - 1 - (u32)l) >> 4) << 4) + l; j >= 0; j -= 16) part = e_add(e_mul(part, a16), e_from(ev[j]));
                mine = e_add(mine, e_mul(off, part));
                off = e_mul(off, e_pow(alpha, (u64)ncols));
            }
            const ext2 r = group_sum(e_mul(mine, al));
            const ext2 d = e_sub(e_from(subgroup_x), rd2(tb + FT_Z + 2 * b));
            if (d.a == 0 && d.b == 0) FV_FAIL(FV_POINT, b);       // reject, never divide by zero
            old_eval = e_add(e_mul(old_eval, off), e_mul(e_sub(r, rd2(tb + FT_RED + 2 * b)), e_inv(d)));
        }
    }
    // ---- reductions: consistency with the previous layer, interpolation of the coset at beta, Merkle path of the layer
    for (u32 r = 0; r < a.nred; r++) {
        const u32 ab = a.ab[r], arity = 1u << ab;
        const u64 *ev = w, *path = w + 2 * (size_t)arity;
        const size_t coset_index = x_index >> ab, within = x_index & (arity - 1);
        if (!e_eq(rd2(ev + 2 * within), old_eval)) FV_FAIL(FV_FOLD, r);
        {   // compute_evaluation: sum_i vals_i prod_{j != i} (beta - p_j) / (p_i - p_j), p_j = coset_start gA^j; lane l takes i = l
            const u64 gA = a.gA[r];
            const u32 rw = (u32)(__brev((unsigned)within) >> (32 - ab));
            const u64 coset_start = mul(subgroup_x, dvpow(gA, (u64)(arity - rw)));
            const ext2 beta = rd2(tb + FT_BETAS + 2 * r);
            ext2 acc = e_from(0);
            for (u32 i = (u32)l; i < arity; i += 16) {
                const u64 pi = mul(coset_start, dvpow(gA, (u64)i));
                ext2 num = e_from(1);
                u64 den = 1, pj = coset_start;
                for (u32 j = 0; j < arity; j++) {
                    if (j != i) { num = e_mul(num, e_sub(beta, e_from(pj))); den = mul(den, sub(pi, pj)); }
                    pj = mul(pj, gA);
                }
                const u32 bi = (u32)(__brev((unsigned)i) >> (32 - ab));                   // reverse_index_bits(evals)
                acc = e_add(acc, e_scale(e_mul(rd2(ev + 2 * bi), num), glf::inv(den)));
            }
            old_eval = group_sum(acc);
        }
        const u64 *cap = proof + (size_t)r * capn4;
        if (merkle_bad<HASHER>(ev, 2 * arity, coset_index, path, a.step_depth[r], cap, l, gb)) FV_FAIL(FV_LAYER, r);
        for (u32 i = 0; i < ab; i++) subgroup_x = sqr(subgroup_x);
        x_index = coset_index;
        w += 2 * (size_t)arity + 4 * (size_t)a.step_depth[r];
    }
    {   // final_poly.eval(subgroup_x)
        ext2 acc = e_from(0);
        for (u32 i = a.final_len; i-- > 0;) acc = e_add(e_scale(acc, subgroup_x), rd2(proof + a.final_poly + 2 * (size_t)i));
        if (!e_eq(acc, old_eval)) FV_FAIL(FV_FINAL, 0);
    }
#undef FV_FAIL
    if (live && l == 0) a.status[grp] = code;
}

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
    u32 leaf_off[GLP_FRI_MAX_ORACLES];
    size_t q = 0;
    for (u32 o = 0; o < p.nor; o++) {
        p.leaf_len[o] = ncols[o] + (d->oracles[o].salted ? GLP_SALT_SIZE : 0);
        p.shared[o] = d->oracles[o].shared != 0;
        GLP_REQUIRE(q <= 0x7FFFFFFFu, "oracles: a query record of more than 2^31 words");
        leaf_off[o] = (u32)q;
        q += p.leaf_len[o] + 4 * (size_t)p.depth0;
    }
    u32 lg = p.lgN;
    for (u32 r = 0; r < p.nred; r++) {
        p.ab[r] = d->reduction_arity_bits[r];
        lg -= p.ab[r];
        p.step_depth[r] = lg - d->cap_height;
        q += 2 * ((size_t)1 << p.ab[r]) + 4 * (size_t)p.step_depth[r];
    }
    p.query_stride = q;
    p.final_len = 1u << (lg - d->rate_bits);
    p.o_queries = (size_t)p.nred * p.capn * 4;
    p.o_final = p.o_queries + q * p.nq;
    p.o_pow = p.o_final + 2 * (size_t)p.final_len;
    p.total = p.o_pow + 1;
    for (u32 b = 0; b < p.npts; b++) {
        const glp_fri_point &pt = d->points[b];
        p.first[b] = (u32)p.nopen; p.len[b] = 0; p.nranges[b] = pt.num_ranges;
        for (u32 r = 0; r < pt.num_ranges; r++) {
            const glp_fri_range &rg = pt.ranges[r];
            p.prog.push_back(leaf_off[rg.oracle]); p.prog.push_back(rg.col_begin); p.prog.push_back(rg.num_cols);
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

    struct Scratch { glp_ctx *c; std::vector<void *> p; ~Scratch() { (void)hipStreamSynchronize(c->stream); for (void *q : p) c->release(q); } } sc{c, {}};
    auto get = [&](void **ptr, size_t bytes) -> int { int r = c->alloc(ptr, bytes); if (r == GLP_OK) sc.p.push_back(*ptr); return r; };
    u64 *dev_proofs = nullptr, *dev_hv = nullptr, *dev_open = nullptr;
    u32 *dev_status = nullptr;
    GLP_TRY(get((void **)&dev_proofs, (size_t)K * p.total * 8));
    GLP_TRY(get((void **)&dev_hv, hv.size() * 8));
    GLP_TRY(get((void **)&dev_status, (size_t)K * nq * 4));
    if (stepped) GLP_TRY(get((void **)&dev_open, (size_t)K * p.nopen * 16));
    // the proofs (and, stepped, the openings) go up on a thread of their own while the host half runs
    hipError_t up_err = hipSuccess;
    std::thread uploader([&] {
        up_err = hipSetDevice(c->device);
        if (up_err == hipSuccess) up_err = hipMemcpyAsync(dev_proofs, proofs, (size_t)K * p.total * 8, hipMemcpyHostToDevice, c->stream);
        if (up_err == hipSuccess && stepped) up_err = hipMemcpyAsync(dev_open, openings, (size_t)K * p.nopen * 16, hipMemcpyHostToDevice, c->stream);
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
    uploader.join();
    if (up_err != hipSuccess) return set_error(GLP_ERR_HIP, "upload of the proofs: %s", hipGetErrorString(up_err));
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
    {
        StageScope st(c, "fri_verify_queries", 8.0 * K * p.total);
        const unsigned nblocks = (unsigned)(((size_t)K * nq + 15) / 16);
        if (p.hasher == GLP_HASH_KECCAK25) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fri_verify_queries<GLP_HASH_KECCAK25>), dim3(nblocks), dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fri_verify_queries<GLP_HASH_POSEIDON>), dim3(nblocks), dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
    }
    std::vector<u32> hs((size_t)K * nq);
    GLP_HIP(hipMemcpyAsync(hs.data(), dev_status, hs.size() * 4, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    for (u32 k = 0; k < K; k++) {
        for (u32 q = 0; q < nq && why[k].empty(); q++)
            if (hs[(size_t)k * nq + q]) why[k] = fv_query_reason(q, hs[(size_t)k * nq + q]);
        status_out[k] = why[k].empty() ? GLP_OK : GLP_ERR_PROVE;
        if (reasons_out) {
            char *o = reasons_out + (size_t)k * GLP_REASON_LEN;
            memset(o, 0, GLP_REASON_LEN);
            strncpy(o, why[k].c_str(), GLP_REASON_LEN - 1);
        }
    }
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
