// fri_openings.inc -- glp_fri_*: the openings and the FRI proof of caller-held PolynomialBatches (plonky2 fri/oracle.rs
// `PolynomialBatch::prove_openings` and the `eval` calls of plonk/prover.rs), for any FriInstanceInfo: up to GLP_FRI_MAX_ORACLES
// oracles, up to GLP_FRI_MAX_POINTS points, each naming column ranges of the oracles.  Included by prover.hip after the session.
//
// The one piece of device code of its own is k_fri_combine (fri_kernels.inc), the generic form of k_final_values.  Everything
// else is the session's: k_zeta_table / k_open_dot on a coefficient pointer advanced to the range, fri_values_to_coeffs,
// stage_fri_commit / stage_fri_fold, queries_oracle / queries_layers, pow_search.  The geometry those read comes from fri_geo
// instead of a circuit.
// The many-proof form (glp_fri_begin_many: K proofs of one instance in lock step) shares the handle, the checks and the step entry
// points; its steps are the functions of fri_many.inc.
#include <map>
#include "fri_shape.h"

namespace {
ProveGeo fri_geo(const glp_batch *b, const u32 *arity_bits, u32 nq) {
    ProveGeo g;
    memset(&g, 0, sizeof(g));
    g.K = 1;
    g.lg = b->lg; g.rb = b->rate_bits; g.hasher = b->hasher; g.cap_height = b->cap_height;
    g.n = (size_t)1 << g.lg; g.N = g.n << g.rb;
    g.capn = 1u << b->cap_height;
    g.arity_bits = arity_bits; g.nq = nq;
    return g;
}
struct FriPointPlan {
    ext2 z;
    std::vector<glp_fri_range> ranges;
    u32 len = 0;               // polynomials named
    size_t first = 0;          // index of its first opening (and of its first alpha power)
    u32 table = 0;             // the earliest point with the same z: one zeta table per distinct point
};
}  // namespace

struct glp_fri {
    glp_ctx *c;
    std::vector<const glp_batch *> ob;
    std::vector<FriPointPlan> pts;
    u32 arity_bits[16] = {0};
    u32 nred = 0, pow_bits = 0;
    ProveGeo g;                        // K = 1, no circuit; arity_bits points into this object
    Tmp tmp;
    size_t nopen = 0;
    std::vector<ext2> open;            // every opening, points in order
    FriState fri;
    bool layer_open = false;
    size_t o_queries = 0, o_final = 0, o_pow = 0, total = 0, query_stride = 0;      // word offsets inside the FriProof (the caps start at 0)
    u32 final_len = 0;
    std::vector<u64> words;            // the FriProof being assembled
    std::vector<u64> cap;
    enum Stage { S_NEW, S_OPEN, S_FRI, S_FINAL, S_DONE } stage = S_NEW;
    // the many-proof form (fri_many.inc): g.K proofs, `words` and `cap` hold [K] of what they hold for one proof
    bool many = false;
    std::vector<u64> zs;               // [K][points][2]: every proof's own points (FriPointPlan::z is proof 0's)
    u64 *dev_zs = nullptr, *dev_open = nullptr;        // zs on the device; the finished openings [K][nopen][2]

    // points_many == nullptr: one proof at the description's points; else K proofs, proof k at points_many[k][num_points][2]
    glp_fri(glp_ctx *ctx, const glp_fri_desc &d, u32 K = 1, const u64 *points_many = nullptr) : c(ctx), tmp(ctx), many(points_many != nullptr) {
        ob.assign(d.oracles, d.oracles + d.num_oracles);
        nred = d.num_reductions; pow_bits = d.proof_of_work_bits;
        for (u32 i = 0; i < nred; i++) arity_bits[i] = d.reduction_arity_bits[i];
        g = fri_geo(ob[0], arity_bits, d.num_query_rounds);
        g.K = K;
        if (many) zs.assign(points_many, points_many + (size_t)K * d.num_points * 2);
        // two points share a zeta table when they are equal for every proof
        auto same_point = [&](u32 e, u32 b) {
            if (!many) return e_eq(pts[e].z, e_make(d.points[b].point[0], d.points[b].point[1]));
            for (u32 k = 0; k < K; k++) {
                const u64 *ze = &zs[((size_t)k * d.num_points + e) * 2], *zb = &zs[((size_t)k * d.num_points + b) * 2];
                if (ze[0] != zb[0] || ze[1] != zb[1]) return false;
            }
            return true;
        };
        for (u32 b = 0; b < d.num_points; b++) {
            FriPointPlan p;
            p.z = many ? e_make(zs[2 * b], zs[2 * b + 1]) : e_make(d.points[b].point[0], d.points[b].point[1]);
            p.ranges.assign(d.points[b].ranges, d.points[b].ranges + d.points[b].num_ranges);
            for (const glp_fri_range &r : p.ranges) p.len += r.num_cols;
            p.first = nopen; nopen += p.len;
            p.table = b;
            for (u32 e = 0; e < b; e++) if (same_point(e, b)) { p.table = e; break; }
            pts.push_back(p);
        }
        const u32 lgN = (u32)(g.lg + g.rb), depth0 = lgN - (u32)g.cap_height;
        size_t q = 0;
        for (const glp_batch *b : ob) q += b->ncols + b->salt + 4 * (size_t)depth0;
        u32 lg = lgN;
        for (u32 i = 0; i < nred; i++) { lg -= arity_bits[i]; q += 2 * ((size_t)1 << arity_bits[i]) + 4 * (size_t)(lg - (u32)g.cap_height); }
        query_stride = q;
        final_len = 1u << (lg - (u32)g.rb);
        o_queries = (size_t)nred * g.capn * 4;
        o_final = o_queries + q * g.nq;
        o_pow = o_final + 2 * (size_t)final_len;
        total = o_pow + 1;
        words.assign((size_t)K * total, 0);
    }
    glp_fri(const glp_fri &) = delete;

    // K7 for every (point, polynomial): one zeta table per distinct point, one dot-product launch per range
    int open_all() {
        GLP_REQUIRE(stage == S_NEW, "glp_fri_open: already opened");
        StageScope st(c, "fri.openings", 8.0 * g.n * nopen);
        const size_t n = g.n;
        const u32 nob = open_blocks(n);
        u64 *partial;
        GLP_TRY(tmp.get(&partial, nopen * nob * 2));
        std::vector<u64 *> zt(pts.size(), nullptr);
        for (size_t b = 0; b < pts.size(); b++) {
            const FriPointPlan &p = pts[b];
            if (p.table != b) zt[b] = zt[p.table];
            else {
                GLP_TRY(tmp.get(&zt[b], 2 * n));
                ZTArgs za;
                za.zt = zt[b]; za.lg = (u32)g.lg; za.zeta_b = nullptr; za.zeta_stride = 0;
                ext2 s = p.z;
                for (int k = 0; k < 24; k++) { za.zp2[k] = s; s = e_sqr(s); }
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_zeta_table<false>), dim3(nblk(n)), dim3(256), 0, c->stream, za);
                GLP_HIP(hipGetLastError());
            }
            size_t pos = p.first;
            for (const glp_fri_range &r : p.ranges)
                for (u32 c0 = 0; c0 < r.num_cols; c0 += 65535) {      // grid.y holds 65535 columns
                    const u32 cnt = std::min<u32>(65535, r.num_cols - c0);
                    hipLaunchKernelGGL(k_open_dot, dim3(nob, cnt, 1), dim3(256), 0, c->stream, ob[r.oracle]->coeffs + (size_t)(r.col_begin + c0) * n,
                                       zt[b], partial + 2 * (size_t)nob * pos, (u32)g.lg, (size_t)0, (size_t)0, (size_t)0);
                    GLP_HIP(hipGetLastError());
                    pos += cnt;
                }
        }
        std::vector<u64> hp(nopen * nob * 2);
        GLP_TRY(d2h(c, hp.data(), partial, hp.size() * 8));
        open_batch_finish(hp.data(), (u32)nopen, nob, open);
        stage = S_OPEN;
        return GLP_OK;
    }
    // K8 -> the FRI polynomial's coefficients, the commit phase starts from them
    int combine(ext2 alpha) {
        GLP_REQUIRE(stage == S_OPEN, "glp_fri_combine: call after glp_fri_open");
        u64 *fcoef;
        GLP_TRY(tmp.get(&fcoef, 2 * g.n));
        GLP_TRY(combine_into(alpha, fcoef));
        fri.start(fcoef, g.lg);
        stage = S_FRI;
        return GLP_OK;
    }
    // the column program and the alpha-power table of this instance, k_fri_combine, values -> coefficients (fcoef [2][n])
    int combine_into(ext2 alpha, u64 *fcoef) {
        StageScope st(c, "fri.combine", 8.0 * g.n * nopen);
        std::vector<FCCol> prog;
        std::map<std::pair<u32, u32>, std::vector<u32>> where;      // (oracle, column) -> its program entries (more than one only if a point names it twice)
        std::vector<u64> ap(2 * nopen);
        FCArgs a;
        memset(&a, 0, sizeof(a));
        for (size_t b = 0; b < pts.size(); b++) {
            const FriPointPlan &p = pts[b];
            ext2 x = e_from(1), red = e_from(0);
            size_t j = p.first;
            for (const glp_fri_range &r : p.ranges)
                for (u32 col = r.col_begin; col < r.col_begin + r.num_cols; col++, j++) {
                    ap[2 * j] = x.a; ap[2 * j + 1] = x.b;
                    red = e_add(red, e_mul(x, open[j]));
                    x = e_mul(x, alpha);
                    std::vector<u32> &es = where[{r.oracle, col}];
                    u32 e = ~0u;
                    for (u32 cand : es) if (prog[cand].ap[b] == FC_ABSENT) { e = cand; break; }
                    if (e == ~0u) {
                        FCCol fc;
                        fc.plane = ob[r.oracle]->lde + (size_t)col * g.N;
                        for (u32 k = 0; k < GLP_FRI_MAX_POINTS; k++) fc.ap[k] = FC_ABSENT;
                        e = (u32)prog.size();
                        prog.push_back(fc);
                        es.push_back(e);
                    }
                    prog[e].ap[b] = (u32)j;
                }
            a.red[b] = red; a.z[b] = p.z; a.shift[b] = x;       // x = alpha^(len_b)
        }
        static_assert(sizeof(FCCol) % sizeof(u64) == 0, "FCCol is uploaded as words");
        u64 *dev_prog, *dev_ap, *fv;
        const size_t prog_words = prog.size() * sizeof(FCCol) / sizeof(u64);
        GLP_TRY(tmp.get(&dev_prog, prog_words));
        GLP_TRY(h2d(c, dev_prog, prog.data(), prog_words * 8));
        GLP_TRY(tmp.get(&dev_ap, ap.size()));
        GLP_TRY(h2d(c, dev_ap, ap.data(), ap.size() * 8));
        GLP_TRY(tmp.get(&fv, 2 * g.n));
        a.prog = (const FCCol *)dev_prog; a.nprog = (u32)prog.size(); a.npoints = (u32)pts.size();
        a.apow = dev_ap; a.out = fv;
        a.w_n = root_of_unity(g.lg); a.g = GEN; a.lg = (u32)g.lg;
        hipLaunchKernelGGL(k_fri_combine, dim3(nblk(g.n)), dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
        return fri_values_to_coeffs(c, g, fv, fcoef);
    }
    int commit_layer() {
        GLP_REQUIRE(stage == S_FRI && !layer_open && fri.layers.size() < nred, "glp_fri_commit: no layer left or beta pending");
        StageScope st(c, "fri.commit", 0.0);
        const size_t r = fri.layers.size();
        GLP_TRY(stage_fri_commit(c, g, tmp, fri));
        cap.resize((size_t)g.capn * 4);
        GLP_TRY(d2h(c, cap.data(), fri_layer_cap(g, fri.layers.back()), (size_t)g.capn * 32));
        memcpy(words.data() + r * g.capn * 4, cap.data(), (size_t)g.capn * 32);
        layer_open = true;
        return GLP_OK;
    }
    int fold(ext2 beta) {
        GLP_REQUIRE(stage == S_FRI && layer_open, "glp_fri_fold: call after glp_fri_commit");
        StageScope st(c, "fri.commit", 0.0);
        GLP_TRY(stage_fri_fold(c, g, tmp, fri, beta, nullptr));
        layer_open = false;
        return GLP_OK;
    }
    // final polynomial (natural coefficient order) -> proof
    int final_poly() {
        GLP_REQUIRE(stage == S_FRI && !layer_open && fri.layers.size() == nred, "glp_fri_final_poly: reductions not finished");
        const size_t fl = (size_t)1 << fri.lgcur;
        std::vector<u64> h(2 * fl);
        GLP_TRY(d2h(c, h.data(), fri.cur, h.size() * 8));
        for (size_t p = 0; p < fl; p++) {
            const size_t k = bitrev32((u32)p, fri.lgcur);
            words[o_final + 2 * k] = h[p];
            words[o_final + 2 * k + 1] = h[fl + p];
        }
        stage = S_FINAL;
        return GLP_OK;
    }
    int queries(u64 pow_witness, const u64 *indices, u32 nq) {
        GLP_REQUIRE(stage == S_FINAL, "glp_fri_queries: call after glp_fri_final_poly");
        GLP_REQUIRE(nq == g.nq, "glp_fri_queries: %u indices, the instance has %u query rounds", nq, g.nq);
        for (u32 q = 0; q < nq; q++) GLP_REQUIRE(indices[q] < (u64)g.N, "query index %llu outside the LDE domain", (unsigned long long)indices[q]);
        words[o_pow] = pow_witness;
        StageScope st(c, "fri.queries", 0.0);
        u64 *dev_idx, *dev_q;
        const size_t qsec = (size_t)nq * query_stride;
        GLP_TRY(tmp.get(&dev_idx, nq));
        GLP_TRY(tmp.get(&dev_q, qsec));
        GLP_TRY(h2d(c, dev_idx, indices, (size_t)nq * 8));
        size_t off = 0;
        for (const glp_batch *b : ob) GLP_TRY(queries_oracle(c, g, b, true, dev_idx, dev_q, query_stride, qsec, off));
        GLP_TRY(queries_layers(c, g, fri.layers, dev_idx, dev_q, query_stride, qsec, off));
        if (off != query_stride) return set_error(GLP_ERR_ARG, "internal: query record layout mismatch");
        GLP_TRY(d2h(c, words.data() + o_queries, dev_q, qsec * 8));
        stage = S_DONE;
        return GLP_OK;
    }
};

namespace {
// num_proofs == 0: glp_fri_begin / glp_fri_prove (one proof at the description's points); else the many form at points_many[num_proofs][num_points][2]
int fri_check(glp_ctx *c, const glp_fri_desc *d, u32 num_proofs = 0, const u64 *points_many = nullptr) {
    GLP_TRY(fri_shape_counts(d->num_oracles, d->oracles, d->num_points, d->points));
    const glp_batch *b0 = d->oracles[0];
    for (u32 i = 0; i < d->num_oracles; i++) {
        const glp_batch *b = d->oracles[i];
        GLP_REQUIRE(b, "oracles[%u] is null", i);
        if (!num_proofs && b->K != 1)
            return set_error(GLP_ERR_UNSUPPORTED, "oracles[%u] is a many-proof batch (K = %u): glp_fri_begin_many proves those", i, b->K);
        GLP_REQUIRE(!num_proofs || b->K == 1 || b->K == num_proofs,
                    "oracles[%u]: K = %u, neither num_proofs = %u (an oracle per proof) nor 1 (one oracle shared by all proofs)", i, b->K, num_proofs);
        GLP_REQUIRE(b->ctx == c, "oracles[%u] belongs to another ctx", i);
        GLP_REQUIRE(b->lg == b0->lg, "oracles[%u]: log_n = %d, oracles[0] has %d", i, b->lg, b0->lg);
        GLP_REQUIRE(b->rate_bits == b0->rate_bits, "oracles[%u]: rate_bits = %d, oracles[0] has %d", i, b->rate_bits, b0->rate_bits);
        GLP_REQUIRE(b->cap_height == b0->cap_height, "oracles[%u]: cap_height = %d, oracles[0] has %d", i, b->cap_height, b0->cap_height);
        GLP_REQUIRE(b->hasher == b0->hasher, "oracles[%u]: hasher = %d, oracles[0] has %d", i, b->hasher, b0->hasher);
    }
    if (num_proofs > 1) {
        bool per_proof = false;
        for (u32 i = 0; i < d->num_oracles; i++) per_proof |= d->oracles[i]->K == num_proofs;
        GLP_REQUIRE(per_proof, "oracles: every one is shared (K = 1), none has K = num_proofs = %u", num_proofs);
    }
    const u32 lg = (u32)b0->lg;
    const u64 gn = pow(GEN, (u64)1 << lg);
    u32 ncols[GLP_FRI_MAX_ORACLES];
    for (u32 i = 0; i < d->num_oracles; i++) ncols[i] = d->oracles[i]->ncols;
    // the rules a verifier without batches checks too (fri_shape.h)
    GLP_TRY(fri_shape_rules(ncols, d->num_oracles, lg, (u32)b0->rate_bits, (u32)b0->cap_height, d->num_points, d->points, !num_proofs, d->num_reductions,
                            d->reduction_arity_bits, d->proof_of_work_bits, d->num_query_rounds));
    // x - z must be invertible on coset plane 0 = g H: z = a + 0 X with (a / g)^n = 1 is a point of it
    for (u32 p = 0; p < d->num_points && !num_proofs; p++)
        if (d->points[p].point[1] == 0 && pow(d->points[p].point[0], (u64)1 << lg) == gn)
            return set_error(GLP_ERR_PROVE, "points[%u] lies on the coset g H of the commitments", p);
    for (u32 k = 0; k < num_proofs; k++)
        for (u32 p = 0; p < d->num_points; p++) {
            const u64 *z = points_many + ((size_t)k * d->num_points + p) * 2;
            GLP_REQUIRE(z[0] < P && z[1] < P, "points[%u][%u] (proof %u) is not canonical", k, p, k);
            if (z[1] == 0 && pow(z[0], (u64)1 << lg) == gn)
                return set_error(GLP_ERR_PROVE, "points[%u][%u] (proof %u) lies on the coset g H of the commitments", k, p, k);
        }
    return GLP_OK;
}
}  // namespace
#include "fri_many.inc"

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
    GLP_TRY(fri_check(c, desc));
    GLP_TRY(bind(c));
    *out = new glp_fri(c, *desc);
    return GLP_OK;
}
#define GLP_FRI_ENTER(F)                          \
    GLP_REQUIRE((F) != nullptr, "null glp_fri");  \
    GLP_TRY(bind((F)->c))
size_t glp_fri_num_openings(const glp_fri *f) { return f ? f->nopen : 0; }
size_t glp_fri_final_poly_len(const glp_fri *f) { return f ? f->final_len : 0; }
size_t glp_fri_proof_words(const glp_fri *f) { return f ? f->total : 0; }
int glp_fri_open(glp_fri *f, uint64_t *openings_out) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(openings_out, "null argument");
    if (f->many) return fri_many_open(*f, openings_out);
    GLP_TRY(f->open_all());
    for (size_t k = 0; k < f->nopen; k++) { openings_out[2 * k] = f->open[k].a; openings_out[2 * k + 1] = f->open[k].b; }
    return GLP_OK;
}
int glp_fri_combine(glp_fri *f, const uint64_t alpha[2]) {
    GLP_FRI_ENTER(f);
    if (f->many) return fri_many_combine(*f, alpha);
    GLP_REQUIRE(alpha && alpha[0] < P && alpha[1] < P, "alpha is null or not canonical");
    return f->combine(e_make(alpha[0], alpha[1]));
}
int glp_fri_commit(glp_fri *f, uint64_t *cap_out) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(cap_out, "null argument");
    GLP_TRY(f->many ? fri_many_commit(*f) : f->commit_layer());
    memcpy(cap_out, f->cap.data(), (size_t)f->g.K * f->g.capn * 32);
    return GLP_OK;
}
int glp_fri_fold(glp_fri *f, const uint64_t beta[2]) {
    GLP_FRI_ENTER(f);
    if (f->many) return fri_many_fold(*f, beta);
    GLP_REQUIRE(beta && beta[0] < P && beta[1] < P, "beta is null or not canonical");
    return f->fold(e_make(beta[0], beta[1]));
}
int glp_fri_final_poly(glp_fri *f, uint64_t *coeffs_out) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(coeffs_out, "null argument");
    if (f->many) return fri_many_final_poly(*f, coeffs_out);
    GLP_TRY(f->final_poly());
    memcpy(coeffs_out, f->words.data() + f->o_final, (size_t)f->final_len * 16);
    return GLP_OK;
}
int glp_fri_queries(glp_fri *f, uint64_t pow_witness, const uint64_t *indices, uint32_t num_indices) {
    GLP_FRI_ENTER(f);
    GLP_REQUIRE(indices, "null argument");
    GLP_REQUIRE(!f->many, "glp_fri_queries: a many-proof handle takes one witness per proof: glp_fri_queries_many");
    return f->queries(pow_witness, indices, num_indices);
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
// the stepped sequence driven by the library's transcript (fri/prover.rs `fri_proof` order)
int glp_fri_prove(glp_ctx *c, const glp_fri_desc *desc, const uint64_t sponge_state[12], const uint64_t *pending_inputs, uint32_t num_pending,
                  uint64_t *openings_out, uint64_t *proof_out) {
    GLP_REQUIRE(c && desc && sponge_state && openings_out && proof_out && (pending_inputs || num_pending == 0), "null argument");
    GLP_REQUIRE(num_pending < 8, "%u pending inputs (the rate is 8)", num_pending);
    GLP_TRY(fri_check(c, desc));
    GLP_TRY(bind(c));
    glp_fri f(c, *desc);
    Challenger ch(f.g.hasher);
    memcpy(ch.st, sponge_state, 96);
    for (u32 i = 0; i < num_pending; i++) ch.in[i] = pending_inputs[i];
    ch.nin = (int)num_pending;
    // the caller has just observed the openings: with nothing pending its last observation filled the rate and permuted, which
    // refills the output buffer from the state (plonky2's `duplexing`); with inputs pending the output buffer is empty
    if (num_pending == 0) { memcpy(ch.out, ch.st, 64); ch.nout = 8; }
    GLP_TRY(f.open_all());
    for (size_t k = 0; k < f.nopen; k++) { openings_out[2 * k] = f.open[k].a; openings_out[2 * k + 1] = f.open[k].b; }
    GLP_TRY(f.combine(ch.get_ext()));
    for (u32 r = 0; r < f.nred; r++) {
        GLP_TRY(f.commit_layer());
        ch.observe_hashes(f.cap.data(), f.g.capn);
        GLP_TRY(f.fold(ch.get_ext()));
    }
    GLP_TRY(f.final_poly());
    ch.observe(f.words.data() + f.o_final, 2 * (size_t)f.final_len);
    u64 found;
    GLP_TRY(pow_search(c, ch.st, ch.in, (u32)ch.nin, f.pow_bits, &found, f.g.hasher));
    ch.observe(&found, 1);
    const u64 resp = ch.get();
    if (f.pow_bits && (resp >> (64 - f.pow_bits)) != 0) return set_error(GLP_ERR_PROVE, "proof-of-work response check failed");
    std::vector<u64> xi(f.g.nq);
    for (u32 q = 0; q < f.g.nq; q++) xi[q] = ch.get() % (u64)f.g.N;
    GLP_TRY(f.queries(found, xi.data(), f.g.nq));
    memcpy(proof_out, f.words.data(), f.total * 8);
    return GLP_OK;
}
}  // extern "C"
