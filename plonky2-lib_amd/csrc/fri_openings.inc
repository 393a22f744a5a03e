// fri_openings.inc -- glp_fri_*: the openings and the FRI proofs of caller-held PolynomialBatches (plonky2 fri/oracle.rs
// `PolynomialBatch::prove_openings` and the `eval` calls of plonk/prover.rs), for any FriInstanceInfo: up to GLP_FRI_MAX_ORACLES
// oracles, up to GLP_FRI_MAX_POINTS points, each naming column ranges of the oracles.  Included by prover.hip after the session.
//
// A handle holds K >= 1 proofs of ONE instance that advance in lock step.  glp_fri_begin / glp_fri_prove make it with K = 1 at the
// description's points; glp_fri_begin_many / glp_fri_prove_many with the caller's K and points [K][num_points][2], for circuits
// outside the gate library that are small enough to be bound by launch and host latency when proved one by one (what
// glp_prove_batch is to glp_prove).  An oracle is either per proof (glp_batch::K == K, arrays [K][...]) or shared by all proofs
// (K == 1 under K > 1, stride 0); every proof has its own opening points, alpha, betas, witness and query indices.
//
// Every step is a fixed number of launches over all K proofs and one copy to or from the host.  The device code of its own is the
// combination, k_fri_table + k_fri_combine_many(_small) (fri_kernels.inc), the generic form of k_final_values(_small), and
// k_fri_open_finish.  Everything else is what the batch prover drives the same way: k_zeta_table / k_open_dot on a coefficient
// pointer advanced to the range, fri_values_to_coeffs, stage_fri_commit / stage_fri_fold, queries_oracle / queries_layers,
// pow_search / pow_search_batch.  The geometry those read comes from fri_geo instead of a circuit.
#include <map>
#include "fri_shape.h"

namespace {
ProveGeo fri_geo(const glp_batch *b, const u32 *arity_bits, u32 nq, u32 K) {
    ProveGeo g;
    memset(&g, 0, sizeof(g));
    g.K = K;
    g.lg = b->lg; g.rb = b->rate_bits; g.hasher = b->hasher; g.cap_height = b->cap_height;
    g.n = (size_t)1 << g.lg; g.N = g.n << g.rb;
    g.capn = 1u << b->cap_height;
    g.arity_bits = arity_bits; g.nq = nq;
    return g;
}
struct FriPointPlan {
    std::vector<glp_fri_range> ranges;
    u32 len = 0;               // polynomials named
    size_t first = 0;          // index of its first opening (and of its first alpha power)
    u32 table = 0;             // the earliest point that equals this one for every proof: one zeta table per distinct point
};
}  // namespace

struct glp_fri {
    glp_ctx *c;
    std::vector<const glp_batch *> ob;
    std::vector<FriPointPlan> pts;
    u32 arity_bits[16] = {0};
    u32 nred = 0, pow_bits = 0;
    ProveGeo g;                        // g.K proofs, no circuit; arity_bits points into this object
    Scratch tmp;
    size_t nopen = 0;                  // openings of one proof, points in order
    FriState fri;
    bool layer_open = false;
    size_t o_queries = 0, o_final = 0, o_pow = 0, total = 0, query_stride = 0;      // word offsets inside one FriProof (the caps start at 0)
    u32 final_len = 0;
    std::vector<u64> words;            // [K][total]: the FriProofs being assembled
    std::vector<u64> cap;              // [K][capn][4]: the caps of the last layer committed
    enum Stage { S_NEW, S_OPEN, S_FRI, S_FINAL, S_DONE } stage = S_NEW;
    const bool many;                   // made by a many entry point: decides which queries call it takes and which proof-of-work search fri_prove runs
    std::vector<u64> zs;               // [K][points][2]: every proof's own points
    u64 *dev_zs = nullptr, *dev_open = nullptr;        // zs on the device; the finished openings [K][nopen][2]

    // K proofs, proof k at points[k][num_points][2]
    glp_fri(glp_ctx *ctx, const glp_fri_desc &d, u32 K, const u64 *points, bool many_) : c(ctx), tmp(ctx), many(many_) {
        ob.assign(d.oracles, d.oracles + d.num_oracles);
        nred = d.num_reductions; pow_bits = d.proof_of_work_bits;
        for (u32 i = 0; i < nred; i++) arity_bits[i] = d.reduction_arity_bits[i];
        g = fri_geo(ob[0], arity_bits, d.num_query_rounds, K);
        zs.assign(points, points + (size_t)K * d.num_points * 2);
        // two points share a zeta table when they are equal for every proof
        auto same_point = [&](u32 e, u32 b) {
            for (u32 k = 0; k < K; k++) {
                const u64 *ze = &zs[((size_t)k * d.num_points + e) * 2], *zb = &zs[((size_t)k * d.num_points + b) * 2];
                if (ze[0] != zb[0] || ze[1] != zb[1]) return false;
            }
            return true;
        };
        for (u32 b = 0; b < d.num_points; b++) {
            FriPointPlan p;
            p.ranges.assign(d.points[b].ranges, d.points[b].ranges + d.points[b].num_ranges);
            for (const glp_fri_range &r : p.ranges) p.len += r.num_cols;
            p.first = nopen; nopen += p.len;
            p.table = b;
            for (u32 e = 0; e < b; e++) if (same_point(e, b)) { p.table = e; break; }
            pts.push_back(p);
        }
        u32 leaf_len[GLP_FRI_MAX_ORACLES];
        for (size_t o = 0; o < ob.size(); o++) leaf_len[o] = ob[o]->ncols + ob[o]->salt;
        const FriProofLayout f = fri_proof_layout((u32)(g.lg + g.rb), (u32)g.rb, (u32)g.cap_height, leaf_len, (u32)ob.size(), arity_bits, nred, g.nq);
        query_stride = f.query_stride; final_len = f.final_len;
        o_queries = f.queries; o_final = f.final_poly; o_pow = f.pow; total = f.total;
        words.assign((size_t)K * total, 0);
    }
    glp_fri(const glp_fri &) = delete;

    bool shared(const glp_batch *b) const { return b->K != g.K; }        // K == 1 under K > 1 proofs
    u64 *proof_words(size_t k) { return words.data() + k * total; }

    // K7 for every (proof, point, polynomial) -> openings_out [K][nopen][2]: one zeta table per distinct point, one dot-product launch per range
    int open(u64 *openings_out) {
        GLP_REQUIRE(stage == S_NEW, "glp_fri_open: already opened");
        const size_t n = g.n, npts = pts.size();
        const u32 K = g.K, nob = open_blocks(n);
        StageScope st(c, "fri.openings", 8.0 * n * nopen * K);
        u64 *partial;
        GLP_TRY(tmp.words(&partial, (size_t)K * nopen * nob * 2));
        GLP_TRY(tmp.words(&dev_zs, zs.size()));
        GLP_TRY(h2d(c, dev_zs, zs.data(), zs.size() * 8));
        std::vector<u64 *> zt(npts, nullptr);
        for (size_t b = 0; b < npts; b++) {
            const FriPointPlan &p = pts[b];
            if (p.table != b) zt[b] = zt[p.table];
            else {
                GLP_TRY(tmp.words(&zt[b], (size_t)K * 2 * n));
                ZTArgs za;
                za.zt = zt[b]; za.lg = (u32)g.lg;
                if (K == 1) {       // one point: its squarings are made here once and ride in the kernel arguments, not lg per lane on the device
                    za.zeta_b = nullptr; za.zeta_stride = 0;
                    ext2 s = e_make(zs[2 * b], zs[2 * b + 1]);
                    for (int k = 0; k < 24; k++) { za.zp2[k] = s; s = e_sqr(s); }
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_zeta_table<false>), dim3(nblk(n)), dim3(256), 0, c->stream, za);
                } else {
                    za.zeta_b = dev_zs + 2 * b; za.zeta_stride = 2 * npts;
                    for (int k = 0; k < 24; k++) za.zp2[k] = e_from(0);
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_zeta_table<true>), dim3(nblk(n), K), dim3(256), 0, c->stream, za);
                }
                GLP_HIP(hipGetLastError());
            }
            size_t pos = p.first;
            for (const glp_fri_range &r : p.ranges) {
                const glp_batch *o = ob[r.oracle];
                for (u32 c0 = 0; c0 < r.num_cols; c0 += GRID_YZ_MAX) {        // the column rides in grid.y
                    const u32 cnt = std::min(GRID_YZ_MAX, r.num_cols - c0);
                    hipLaunchKernelGGL(k_open_dot, dim3(nob, cnt, K), dim3(256), 0, c->stream, o->coeffs + (size_t)(r.col_begin + c0) * n, zt[b],
                                       partial + 2 * (size_t)nob * pos, (u32)g.lg, shared(o) ? (size_t)0 : (size_t)o->ncols * n, 2 * n,
                                       nopen * nob * 2);
                    GLP_HIP(hipGetLastError());
                    pos += cnt;
                }
            }
        }
        GLP_TRY(tmp.words(&dev_open, (size_t)K * nopen * 2));
        hipLaunchKernelGGL(k_fri_open_finish, dim3(nblk((size_t)K * nopen)), dim3(256), 0, c->stream, partial, dev_open, (size_t)K * nopen, nob);
        GLP_HIP(hipGetLastError());
        GLP_TRY(d2h(c, openings_out, dev_open, (size_t)K * nopen * 16));
        stage = S_OPEN;
        return GLP_OK;
    }

    // K8 -> the K FRI polynomials' coefficients, the commit phase starts from them.  alphas [K][2]
    int combine(const u64 *alphas) {
        GLP_REQUIRE(stage == S_OPEN, "glp_fri_combine: call after glp_fri_open");
        GLP_REQUIRE(alphas, "alpha is null");
        const u32 K = g.K;
        for (u32 k = 0; k < K; k++) GLP_REQUIRE(alphas[2 * k] < P && alphas[2 * k + 1] < P, "alpha[%u] is not canonical", k);
        StageScope st(c, "fri.combine", 8.0 * g.n * nopen * K);
        // the column program: one for all proofs
        std::vector<FCColM> prog;
        std::map<std::pair<u32, u32>, std::vector<u32>> where;      // (oracle, column) -> its program entries (more than one only if a point names it twice)
        FTArgs ta;
        memset(&ta, 0, sizeof(ta));
        for (size_t b = 0; b < pts.size(); b++) {
            const FriPointPlan &p = pts[b];
            size_t j = p.first;
            for (const glp_fri_range &r : p.ranges) {
                const glp_batch *o = ob[r.oracle];
                for (u32 col = r.col_begin; col < r.col_begin + r.num_cols; col++, j++) {
                    std::vector<u32> &es = where[{r.oracle, col}];
                    u32 e = ~0u;
                    for (u32 cand : es) if (prog[cand].ap[b] == FC_ABSENT) { e = cand; break; }
                    if (e == ~0u) {
                        FCColM fc;
                        fc.plane = o->lde + (size_t)col * g.N;
                        fc.stride = shared(o) ? 0 : (size_t)(o->ncols + o->salt) * g.N;
                        for (u32 k = 0; k < GLP_FRI_MAX_POINTS; k++) fc.ap[k] = FC_ABSENT;
                        e = (u32)prog.size();
                        prog.push_back(fc);
                        es.push_back(e);
                    }
                    prog[e].ap[b] = (u32)j;
                }
            }
            ta.first[b] = (u32)p.first; ta.len[b] = p.len;
        }
        static_assert(sizeof(FCColM) % sizeof(u64) == 0, "FCColM is uploaded as words");
        // the program and the alphas go up in one copy: every upload is a host round trip inside the stage
        u64 *dev_prog, *dev_ap, *dev_pp, *fv, *fcoef;
        const size_t prog_words = prog.size() * sizeof(FCColM) / sizeof(u64);
        std::vector<u64> up(prog_words + (size_t)K * 2);
        memcpy(up.data(), prog.data(), prog_words * 8);
        memcpy(up.data() + prog_words, alphas, (size_t)K * 16);
        GLP_TRY(tmp.words(&dev_prog, up.size()));
        GLP_TRY(h2d(c, dev_prog, up.data(), up.size() * 8));
        const u64 *dev_alpha = dev_prog + prog_words;
        GLP_TRY(tmp.words(&dev_ap, (size_t)K * 2 * nopen));
        GLP_TRY(tmp.words(&dev_pp, (size_t)K * FCM_PP_WORDS));
        GLP_TRY(tmp.words(&fv, (size_t)K * 2 * g.n));
        GLP_TRY(tmp.words(&fcoef, (size_t)K * 2 * g.n));
        ta.alpha = dev_alpha; ta.open = dev_open; ta.z = dev_zs; ta.apow = dev_ap; ta.pp = dev_pp; ta.nopen = nopen;
        hipLaunchKernelGGL(k_fri_table, dim3((unsigned)pts.size(), K), dim3(256), 0, c->stream, ta);
        GLP_HIP(hipGetLastError());
        FCMArgs a;
        memset(&a, 0, sizeof(a));
        a.prog = (const FCColM *)dev_prog; a.nprog = (u32)prog.size(); a.npoints = (u32)pts.size();
        a.apow = dev_ap; a.pp = dev_pp; a.out = fv; a.nopen = nopen;
        a.w_n = root_of_unity(g.lg); a.g = GEN; a.lg = (u32)g.lg;
        if (g.lg >= 2 && g.lg <= 7) hipLaunchKernelGGL(k_fri_combine_many_small, dim3(1, K), dim3(256), 0, c->stream, a);      // 4..128 points: 256 / n lanes per point
        else hipLaunchKernelGGL(k_fri_combine_many, dim3(nblk(g.n), K), dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
        GLP_TRY(fri_values_to_coeffs(c, g, fv, fcoef));
        fri.start(fcoef, g.lg);
        stage = S_FRI;
        return GLP_OK;
    }

    // one layer of all K proofs -> cap [K][capn][4], into the proofs and cap_out (may be null)
    int commit(u64 *cap_out) {
        GLP_REQUIRE(stage == S_FRI && !layer_open && fri.layers.size() < nred, "glp_fri_commit: no layer left or beta pending");
        StageScope st(c, "fri.commit", 0.0);
        const size_t r = fri.layers.size(), capw = (size_t)g.capn * 4;
        GLP_TRY(stage_fri_commit(c, g, tmp, fri));
        const FriLayer &ly = fri.layers.back();
        GLP_TRY(caps_to_host(c, ly.dig, ly.ndig * 4, merkle_cap_offset(((size_t)1 << ly.lgL) >> ly.ab, g.cap_height), g.capn, g.K, cap));
        for (u32 k = 0; k < g.K; k++) memcpy(proof_words(k) + r * capw, &cap[k * capw], capw * 8);
        if (cap_out) memcpy(cap_out, cap.data(), g.K * capw * 8);
        layer_open = true;
        return GLP_OK;
    }
    // betas [K][2]
    int fold(const u64 *betas) {
        GLP_REQUIRE(stage == S_FRI && layer_open, "glp_fri_fold: call after glp_fri_commit");
        GLP_REQUIRE(betas, "beta is null");
        const u32 K = g.K;
        for (u32 k = 0; k < K; k++) GLP_REQUIRE(betas[2 * k] < P && betas[2 * k + 1] < P, "beta[%u] is not canonical", k);
        StageScope st(c, "fri.fold", 0.0);
        u64 *dev_betas = nullptr;                               // one beta rides in the kernel arguments: no upload per layer
        if (K > 1) {
            GLP_TRY(tmp.words(&dev_betas, (size_t)K * 2));
            GLP_TRY(h2d(c, dev_betas, betas, (size_t)K * 16));
        }
        GLP_TRY(stage_fri_fold(c, g, tmp, fri, K > 1 ? e_from(0) : e_make(betas[0], betas[1]), dev_betas));      // k_fri_fold reads dev_betas when set
        layer_open = false;
        return GLP_OK;
    }
    // the K final polynomials (natural coefficient order) -> the proofs and coeffs_out [K][final_len][2] (may be null)
    int final_poly(u64 *coeffs_out) {
        GLP_REQUIRE(stage == S_FRI && !layer_open && fri.layers.size() == nred, "glp_fri_final_poly: reductions not finished");
        const size_t fl = (size_t)1 << fri.lgcur;
        const u32 K = g.K;
        std::vector<u64> h((size_t)K * 2 * fl);
        GLP_TRY(d2h(c, h.data(), fri.cur, h.size() * 8));
        for (u32 k = 0; k < K; k++) {
            u64 *pf = proof_words(k) + o_final;
            for (size_t p = 0; p < fl; p++) {
                const size_t kk = bitrev32((u32)p, fri.lgcur);
                pf[2 * kk] = h[(size_t)k * 2 * fl + p];
                pf[2 * kk + 1] = h[(size_t)k * 2 * fl + fl + p];
            }
            if (coeffs_out) memcpy(coeffs_out + (size_t)k * 2 * fl, pf, fl * 16);
        }
        stage = S_FINAL;
        return GLP_OK;
    }
    // pow_witnesses [K], indices [K][nq]: every gather writes into a device image of the K query sections, one strided copy brings them back
    int queries(const u64 *pow_witnesses, const u64 *indices) {
        GLP_REQUIRE(stage == S_FINAL, "glp_fri_queries: call after glp_fri_final_poly");
        const u32 K = g.K, nq = g.nq;
        for (u32 k = 0; k < K; k++)
            for (u32 q = 0; q < nq; q++)
                GLP_REQUIRE(indices[(size_t)k * nq + q] < (u64)g.N, "indices[%u][%u] = %llu outside the LDE domain", k, q,
                            (unsigned long long)indices[(size_t)k * nq + q]);
        for (u32 k = 0; k < K; k++)          // a field element that lands in the proof
            GLP_REQUIRE(pow_witnesses[k] < P, "glp_fri_queries: pow_witnesses[%u] = 0x%016llx is not a canonical field element (>= p)", k,
                        (unsigned long long)pow_witnesses[k]);
        for (u32 k = 0; k < K; k++) proof_words(k)[o_pow] = pow_witnesses[k];
        StageScope st(c, "fri.queries", 0.0);
        u64 *dev_idx, *dev_q;
        const size_t qsec = (size_t)nq * query_stride;
        GLP_TRY(tmp.words(&dev_idx, (size_t)K * nq));
        GLP_TRY(tmp.words(&dev_q, (size_t)K * qsec));
        GLP_TRY(h2d(c, dev_idx, indices, (size_t)K * nq * 8));
        size_t off = 0;
        for (const glp_batch *b : ob) GLP_TRY(queries_oracle(c, g, b, shared(b), dev_idx, dev_q, query_stride, qsec, off));
        GLP_TRY(queries_layers(c, g, fri.layers, dev_idx, dev_q, query_stride, qsec, off));
        if (off != query_stride) return set_error(GLP_ERR_ARG, "internal: query record layout mismatch");
        GLP_HIP(hipMemcpy2DAsync(words.data() + o_queries, total * 8, dev_q, qsec * 8, qsec * 8, K, hipMemcpyDeviceToHost, c->stream));
        GLP_HIP(hipStreamSynchronize(c->stream));
        stage = S_DONE;
        return GLP_OK;
    }
};

namespace {
// the [1][num_points][2] array of a one-proof description's points (left empty where fri_check refuses the counts before it reads the array)
std::vector<u64> fri_desc_points(const glp_fri_desc *d) {
    std::vector<u64> z;
    if (d->points && d->num_points <= GLP_FRI_MAX_POINTS)
        for (u32 p = 0; p < d->num_points; p++) { z.push_back(d->points[p].point[0]); z.push_back(d->points[p].point[1]); }
    return z;
}
int fri_many_args(u32 num_proofs, const u64 *points) {
    GLP_REQUIRE(num_proofs >= 1 && num_proofs <= 4096, "num_proofs = %u outside 1..4096", num_proofs);
    GLP_REQUIRE(points, "points (the per-proof array [num_proofs][num_points][2]) is null");
    return GLP_OK;
}
// K proofs, proof k at points[k][num_points][2].  many: the caller is glp_fri_begin_many / glp_fri_prove_many, which take many-proof batches
int fri_check(glp_ctx *c, const glp_fri_desc *d, u32 K, const u64 *points, bool many) {
    GLP_TRY(fri_shape_counts(d->num_oracles, d->oracles, d->num_points, d->points));
    const glp_batch *b0 = d->oracles[0];
    bool per_proof = false;
    for (u32 i = 0; i < d->num_oracles; i++) {
        const glp_batch *b = d->oracles[i];
        GLP_REQUIRE(b, "oracles[%u] is null", i);
        if (!many && b->K != 1)
            return set_error(GLP_ERR_UNSUPPORTED, "oracles[%u] is a many-proof batch (K = %u): glp_fri_begin_many proves those", i, b->K);
        GLP_REQUIRE(b->K == 1 || b->K == K, "oracles[%u]: K = %u, neither num_proofs = %u (an oracle per proof) nor 1 (one oracle shared by all proofs)", i,
                    b->K, K);
        per_proof |= b->K == K;
        GLP_REQUIRE(b->ctx == c, "oracles[%u] belongs to another ctx", i);
        GLP_REQUIRE(b->lg == b0->lg, "oracles[%u]: log_n = %d, oracles[0] has %d", i, b->lg, b0->lg);
        GLP_REQUIRE(b->rate_bits == b0->rate_bits, "oracles[%u]: rate_bits = %d, oracles[0] has %d", i, b->rate_bits, b0->rate_bits);
        GLP_REQUIRE(b->cap_height == b0->cap_height, "oracles[%u]: cap_height = %d, oracles[0] has %d", i, b->cap_height, b0->cap_height);
        GLP_REQUIRE(b->hasher == b0->hasher, "oracles[%u]: hasher = %d, oracles[0] has %d", i, b->hasher, b0->hasher);
    }
    GLP_REQUIRE(per_proof, "oracles: every one is shared (K = 1), none has K = num_proofs = %u", K);
    const u32 lg = (u32)b0->lg;
    const u64 gn = pow(GEN, (u64)1 << lg);
    u32 ncols[GLP_FRI_MAX_ORACLES];
    for (u32 i = 0; i < d->num_oracles; i++) ncols[i] = d->oracles[i]->ncols;
    // the rules a verifier without batches checks too (fri_shape.h); the points are checked below, in the array
    GLP_TRY(fri_shape_rules(ncols, d->num_oracles, lg, (u32)b0->rate_bits, (u32)b0->cap_height, d->num_points, d->points, false, d->num_reductions,
                            d->reduction_arity_bits, d->proof_of_work_bits, d->num_query_rounds));
    for (u32 k = 0; k < K; k++)
        for (u32 p = 0; p < d->num_points; p++) {
            const u64 *z = points + ((size_t)k * d->num_points + p) * 2;
            GLP_REQUIRE(z[0] < P && z[1] < P, "points[%u][%u] (proof %u) is not canonical", k, p, k);
            // x - z must be invertible on coset plane 0 = g H: z = a + 0 X with (a / g)^n = 1 is a point of it
            if (z[1] == 0 && pow(z[0], (u64)1 << lg) == gn)
                return set_error(GLP_ERR_PROVE, "points[%u][%u] (proof %u) lies on the coset g H of the commitments", k, p, k);
        }
    return GLP_OK;
}
// K sponges, each with the same number of pending inputs -> the smallest witness of each
int pow_search_many(glp_ctx *c, int hasher, const u64 *states, const u64 *pending, u32 npending, u32 bits, u32 K, u64 *witnesses) {
    StageScope stg(c, "fri_pow", 0.0);
    std::vector<u64> pst(states, states + (size_t)K * 12), best;
    for (u32 k = 0; k < K; k++)
        for (u32 i = 0; i < npending; i++) pst[(size_t)k * 12 + i] = pending[(size_t)k * npending + i];
    const std::vector<u32> ppos(K, npending);
    Scratch tmp(c);
    GLP_TRY(pow_search_batch(c, tmp, hasher, pst, ppos, bits, best));
    for (u32 k = 0; k < K; k++) {
        if (best[k] == ~0ull) return set_error(GLP_ERR_PROVE, "Proof of work failed. This is highly unlikely! (proof %u)", k);
        witnesses[k] = best[k];
    }
    return GLP_OK;
}
// glp_fri_prove and glp_fri_prove_many: the stepped sequence of K proofs driven by K of the library's transcripts on the context's host
// threads, one proof inline (fri/prover.rs `fri_proof` order)
int fri_prove(glp_ctx *c, const glp_fri_desc *desc, u32 K, const u64 *points, bool many, const u64 *sponge_states, const u64 *pending_inputs,
              u32 num_pending, u64 *openings_out, u64 *proofs_out) {
    GLP_REQUIRE(num_pending < 8, "%u pending inputs (the rate is 8)", num_pending);
    GLP_TRY(sponge_args_check(sponge_states, pending_inputs, num_pending, K, many));
    GLP_TRY(fri_check(c, desc, K, points, many));
    GLP_TRY(bind(c));
    glp_fri f(c, *desc, K, points, many);
    const u32 capn = f.g.capn, nq = f.g.nq;
    const int hasher = f.g.hasher;
    std::vector<Challenger> ch(K, Challenger(hasher));
    std::vector<u64> chal((size_t)K * 2);
    HostPool &pool = ctx_host_pool(c);       // runs inline below two proofs
    pool.run(K, [&](size_t k) {
        Challenger &t = ch[k];
        memcpy(t.st, sponge_states + k * 12, 96);
        for (u32 i = 0; i < num_pending; i++) t.in[i] = pending_inputs[k * num_pending + i];
        t.nin = (int)num_pending;
        // the caller has just observed the openings: with nothing pending its last observation filled the rate and permuted, which
        // refills the output buffer from the state (plonky2's `duplexing`); with inputs pending the output buffer is empty
        if (num_pending == 0) { memcpy(t.out, t.st, 64); t.nout = 8; }
    });
    GLP_TRY(f.open(openings_out));
    pool.run(K, [&](size_t k) { const ext2 x = ch[k].get_ext(); chal[2 * k] = x.a; chal[2 * k + 1] = x.b; });
    GLP_TRY(f.combine(chal.data()));
    for (u32 r = 0; r < f.nred; r++) {
        GLP_TRY(f.commit(nullptr));
        pool.run(K, [&](size_t k) {
            ch[k].observe_hashes(&f.cap[k * capn * 4], capn);
            const ext2 x = ch[k].get_ext();
            chal[2 * k] = x.a; chal[2 * k + 1] = x.b;
        });
        GLP_TRY(f.fold(chal.data()));
    }
    GLP_TRY(f.final_poly(nullptr));
    std::vector<u64> pst((size_t)K * 12), best(K);
    std::vector<u32> ppos(K);
    pool.run(K, [&](size_t k) {
        ch[k].observe(f.proof_words(k) + f.o_final, 2 * (size_t)f.final_len);
        memcpy(&pst[k * 12], ch[k].st, 96);
        for (int i = 0; i < ch[k].nin; i++) pst[k * 12 + i] = ch[k].in[i];
        ppos[k] = (u32)ch[k].nin;
    });
    // the one step that knows its entry point: glp_fri_prove searches with k_pow in host-stepped chunks, glp_fri_prove_many with one
    // batch search for all K.  Both return the smallest witness
    if (!many) GLP_TRY(pow_search(c, ch[0].st, ch[0].in, ppos[0], f.pow_bits, &best[0], hasher));
    else {
        for (u32 k = 0; k < K; k++) GLP_REQUIRE(ppos[k] < 8, "proof of work: %u pending inputs (the rate is 8)", ppos[k]);
        StageScope stg(c, "fri_pow", 0.0);
        GLP_TRY(pow_search_batch(c, f.tmp, hasher, pst, ppos, f.pow_bits, best));
    }
    std::vector<u64> xi((size_t)K * nq);
    std::vector<int> err(K, 0);
    pool.run(K, [&](size_t k) {
        if (best[k] == ~0ull) { err[k] = 1; return; }
        ch[k].observe(&best[k], 1);
        const u64 resp = ch[k].get();
        if (f.pow_bits && (resp >> (64 - f.pow_bits)) != 0) { err[k] = 2; return; }
        for (u32 q = 0; q < nq; q++) xi[k * nq + q] = ch[k].get() % (u64)f.g.N;
    });
    for (u32 k = 0; k < K; k++) {
        if (err[k] == 1) return set_error(GLP_ERR_PROVE, "Proof of work failed. This is highly unlikely! (proof %u)", k);
        if (err[k] == 2) return set_error(GLP_ERR_PROVE, "proof-of-work response check failed (proof %u)", k);
    }
    GLP_TRY(f.queries(best.data(), xi.data()));
    memcpy(proofs_out, f.words.data(), (size_t)K * f.total * 8);
    return GLP_OK;
}
}  // namespace

extern "C" {
int glp_session_oracle(glp_session *s, uint32_t index, const glp_batch **out) {
    GLP_REQUIRE(s && out, "null argument");
    *out = nullptr;
    GLP_REQUIRE(index < 4, "glp_session_oracle: index %u (0..3: constants_sigmas, wires, zs_partial_products, quotient)", index);
    const glp_batch *b = index == 0 ? s->cc->cs : index == 1 ? s->wb.b : index == 2 ? s->zb.b : s->qb.b;
    GLP_REQUIRE(b, "glp_session_oracle: oracle %u is not committed yet", index);
    *out = b;
    return GLP_OK;
}

int glp_fri_begin(glp_ctx *c, const glp_fri_desc *desc, glp_fri **out) {
    GLP_REQUIRE(c && desc && out, "null argument");
    *out = nullptr;
    const std::vector<u64> z = fri_desc_points(desc);
    GLP_TRY(fri_check(c, desc, 1, z.data(), false));
    GLP_TRY(bind(c));
    *out = new glp_fri(c, *desc, 1, z.data(), false);
    return GLP_OK;
}
int glp_fri_begin_many(glp_ctx *c, const glp_fri_desc *desc, uint32_t num_proofs, const uint64_t *points, glp_fri **out) {
    GLP_REQUIRE(c && desc && out, "null argument");
    *out = nullptr;
    GLP_TRY(fri_many_args(num_proofs, points));
    GLP_TRY(fri_check(c, desc, num_proofs, points, true));
    GLP_TRY(bind(c));
    *out = new glp_fri(c, *desc, num_proofs, points, true);
    return GLP_OK;
}
#define GLP_FRI_ENTER(F)                          \
    GLP_REQUIRE((F) != nullptr, "null glp_fri");  \
    GLP_TRY(bind((F)->c))
uint32_t glp_fri_num_proofs(const glp_fri *f) { return f ? f->g.K : 0; }
size_t glp_fri_num_openings(const glp_fri *f) { return f ? f->nopen : 0; }
size_t glp_fri_final_poly_len(const glp_fri *f) { return f ? f->final_len : 0; }
size_t glp_fri_proof_words(const glp_fri *f) { return f ? f->total : 0; }
// the steps take [K] of what the header declares for one proof: openings, alpha, cap, beta, coefficients
int glp_fri_open(glp_fri *f, uint64_t *openings_out) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(openings_out, "null argument");
    return f->open(openings_out);
}
int glp_fri_combine(glp_fri *f, const uint64_t alpha[2]) {
    GLP_FRI_ENTER(f);
    return f->combine(alpha);
}
int glp_fri_commit(glp_fri *f, uint64_t *cap_out) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(cap_out, "null argument");
    return f->commit(cap_out);
}
int glp_fri_fold(glp_fri *f, const uint64_t beta[2]) {
    GLP_FRI_ENTER(f);
    return f->fold(beta);
}
int glp_fri_final_poly(glp_fri *f, uint64_t *coeffs_out) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(coeffs_out, "null argument");
    return f->final_poly(coeffs_out);
}
int glp_fri_queries(glp_fri *f, uint64_t pow_witness, const uint64_t *indices, uint32_t num_indices) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(indices, "null argument");
    GLP_REQUIRE(!f->many, "glp_fri_queries: a many-proof handle takes one witness per proof: glp_fri_queries_many");
    GLP_REQUIRE(num_indices == f->g.nq, "glp_fri_queries: %u indices, the instance has %u query rounds", num_indices, f->g.nq);
    return f->queries(&pow_witness, indices);
}
int glp_fri_queries_many(glp_fri *f, const uint64_t *pow_witnesses, const uint64_t *indices) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(pow_witnesses && indices, "null argument");
    GLP_REQUIRE(f->many, "glp_fri_queries_many: the handle comes from glp_fri_begin: glp_fri_queries");
    return f->queries(pow_witnesses, indices);
}
int glp_fri_proof(glp_fri *f, uint64_t *proof_out) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(proof_out, "null argument");
    GLP_REQUIRE(f->stage == glp_fri::S_DONE, "the proof is not finished (call glp_fri_queries first)");
    memcpy(proof_out, f->words.data(), (size_t)f->g.K * f->total * 8);
    return GLP_OK;
}
void glp_fri_end(glp_fri *f) {
    if (!f) return;
    (void)hipSetDevice(f->c->device);
    delete f;
}
int glp_pow_search_many(glp_ctx *c, uint32_t hasher, uint32_t num_proofs, const uint64_t *sponge_states, const uint64_t *pending_inputs,
                        uint32_t num_pending, uint32_t bits, uint64_t *witnesses_out) {
    GLP_REQUIRE(c && sponge_states && witnesses_out && (pending_inputs || num_pending == 0), "null argument");
    GLP_REQUIRE(num_proofs >= 1 && num_proofs <= 4096, "num_proofs = %u outside 1..4096", num_proofs);
    GLP_REQUIRE(num_pending < 8, "proof of work: %u pending inputs (the rate is 8)", num_pending);
    GLP_REQUIRE(bits <= POW_MAX_BITS, "proof_of_work_bits=%u: this build searches at most 2^40 candidates and accepts up to %u bits", bits,
                POW_MAX_BITS);
    if (hasher != GLP_HASH_POSEIDON && hasher != GLP_HASH_KECCAK25) return set_error(GLP_ERR_UNSUPPORTED, "hasher %u is not one of GLP_HASH_*", hasher);
    GLP_TRY(sponge_args_check(sponge_states, pending_inputs, num_pending, num_proofs, true));
    GLP_TRY(bind(c));
    return pow_search_many(c, (int)hasher, sponge_states, pending_inputs, num_pending, bits, num_proofs, witnesses_out);
}
int glp_fri_prove(glp_ctx *c, const glp_fri_desc *desc, const uint64_t sponge_state[12], const uint64_t *pending_inputs, uint32_t num_pending,
                  uint64_t *openings_out, uint64_t *proof_out) {
    GLP_REQUIRE(c && desc && sponge_state && openings_out && proof_out && (pending_inputs || num_pending == 0), "null argument");
    const std::vector<u64> z = fri_desc_points(desc);
    return fri_prove(c, desc, 1, z.data(), false, sponge_state, pending_inputs, num_pending, openings_out, proof_out);
}
int glp_fri_prove_many(glp_ctx *c, const glp_fri_desc *desc, uint32_t num_proofs, const uint64_t *points, const uint64_t *sponge_states,
                       const uint64_t *pending_inputs, uint32_t num_pending, uint64_t *openings_out, uint64_t *proofs_out) {
    GLP_REQUIRE(c && desc && sponge_states && openings_out && proofs_out && (pending_inputs || num_pending == 0), "null argument");
    GLP_TRY(fri_many_args(num_proofs, points));
    return fri_prove(c, desc, num_proofs, points, true, sponge_states, pending_inputs, num_pending, openings_out, proofs_out);
}
}  // extern "C"
