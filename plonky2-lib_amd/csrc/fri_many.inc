// fri_many.inc -- the many-proof form of glp_fri_*: K proofs of ONE FriInstanceInfo in lock step, for circuits outside the gate library
// that are small enough to be bound by launch and host latency when proved one by one (what glp_prove_batch is to glp_prove).
// Included by fri_openings.inc between glp_fri and its C entry points.
//
// Every step is a fixed number of launches over all K proofs and one copy to or from the host: an oracle is either per proof
// (glp_batch::K == K, arrays [K][...]) or shared by all proofs (K == 1, stride 0), every proof has its own opening points, alpha,
// betas, witness and query indices.  The steps of one proof's glp_fri map onto: k_zeta_table<true> / k_open_dot with a proof
// dimension + k_fri_open_finish; k_fri_table + k_fri_combine_many(_small); stage_fri_commit / stage_fri_fold, queries_oracle /
// queries_layers and pow_search_batch, which the batch prover already drives with K > 1.
namespace {

inline bool fri_shared(const glp_fri &f, const glp_batch *b) { return b->K != f.g.K; }      // K == 1 under K > 1 proofs
inline u64 *fri_words(glp_fri &f, u32 k) { return f.words.data() + (size_t)k * f.total; }

// K7 for every (proof, point, polynomial) -> openings_out [K][nopen][2]
int fri_many_open(glp_fri &f, u64 *openings_out) {
    GLP_REQUIRE(f.stage == glp_fri::S_NEW, "glp_fri_open: already opened");
    glp_ctx *c = f.c;
    const ProveGeo &g = f.g;
    const size_t n = g.n, nopen = f.nopen, npts = f.pts.size();
    const u32 K = g.K, nob = open_blocks(n);
    StageScope st(c, "fri.openings", 8.0 * n * nopen * K);
    u64 *partial;
    GLP_TRY(f.tmp.get(&partial, (size_t)K * nopen * nob * 2));
    GLP_TRY(f.tmp.get(&f.dev_zs, f.zs.size()));
    GLP_TRY(h2d(c, f.dev_zs, f.zs.data(), f.zs.size() * 8));
    std::vector<u64 *> zt(npts, nullptr);
    for (size_t b = 0; b < npts; b++) {
        const FriPointPlan &p = f.pts[b];
        if (p.table != b) zt[b] = zt[p.table];
        else {
            GLP_TRY(f.tmp.get(&zt[b], (size_t)K * 2 * n));
            ZTArgs za;
            za.zt = zt[b]; za.lg = (u32)g.lg; za.zeta_b = f.dev_zs + 2 * b; za.zeta_stride = 2 * npts;
            for (int k = 0; k < 24; k++) za.zp2[k] = e_from(0);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_zeta_table<true>), dim3(nblk(n), K), dim3(256), 0, c->stream, za);
            GLP_HIP(hipGetLastError());
        }
        size_t pos = p.first;
        for (const glp_fri_range &r : p.ranges) {
            const glp_batch *ob = f.ob[r.oracle];
            for (u32 c0 = 0; c0 < r.num_cols; c0 += 65535) {      // grid.y holds 65535 columns
                const u32 cnt = std::min<u32>(65535, r.num_cols - c0);
                hipLaunchKernelGGL(k_open_dot, dim3(nob, cnt, K), dim3(256), 0, c->stream, ob->coeffs + (size_t)(r.col_begin + c0) * n, zt[b],
                                   partial + 2 * (size_t)nob * pos, (u32)g.lg, fri_shared(f, ob) ? (size_t)0 : (size_t)ob->ncols * n, 2 * n,
                                   nopen * nob * 2);
                GLP_HIP(hipGetLastError());
                pos += cnt;
            }
        }
    }
    GLP_TRY(f.tmp.get(&f.dev_open, (size_t)K * nopen * 2));
    hipLaunchKernelGGL(k_fri_open_finish, dim3(nblk((size_t)K * nopen)), dim3(256), 0, c->stream, partial, f.dev_open, (size_t)K * nopen, nob);
    GLP_HIP(hipGetLastError());
    GLP_TRY(d2h(c, openings_out, f.dev_open, (size_t)K * nopen * 16));
    f.stage = glp_fri::S_OPEN;
    return GLP_OK;
}

// K8 -> the K FRI polynomials' coefficients.  alphas [K][2]
int fri_many_combine(glp_fri &f, const u64 *alphas) {
    GLP_REQUIRE(f.stage == glp_fri::S_OPEN, "glp_fri_combine: call after glp_fri_open");
    GLP_REQUIRE(alphas, "alpha is null");
    glp_ctx *c = f.c;
    const ProveGeo &g = f.g;
    const u32 K = g.K;
    for (u32 k = 0; k < K; k++) GLP_REQUIRE(alphas[2 * k] < P && alphas[2 * k + 1] < P, "alpha[%u] is not canonical", k);
    StageScope st(c, "fri.combine", 8.0 * g.n * f.nopen * K);
    // the column program: one for all proofs
    std::vector<FCColM> prog;
    std::map<std::pair<u32, u32>, std::vector<u32>> where;      // (oracle, column) -> its program entries (more than one only if a point names it twice)
    FTArgs ta;
    memset(&ta, 0, sizeof(ta));
    for (size_t b = 0; b < f.pts.size(); b++) {
        const FriPointPlan &p = f.pts[b];
        size_t j = p.first;
        for (const glp_fri_range &r : p.ranges) {
            const glp_batch *ob = f.ob[r.oracle];
            for (u32 col = r.col_begin; col < r.col_begin + r.num_cols; col++, j++) {
                std::vector<u32> &es = where[{r.oracle, col}];
                u32 e = ~0u;
                for (u32 cand : es) if (prog[cand].ap[b] == FC_ABSENT) { e = cand; break; }
                if (e == ~0u) {
                    FCColM fc;
                    fc.plane = ob->lde + (size_t)col * g.N;
                    fc.stride = fri_shared(f, ob) ? 0 : (size_t)(ob->ncols + ob->salt) * g.N;
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
    u64 *dev_prog, *dev_alpha, *dev_ap, *dev_pp, *fv, *fcoef;
    const size_t prog_words = prog.size() * sizeof(FCColM) / sizeof(u64);
    GLP_TRY(f.tmp.get(&dev_prog, prog_words));
    GLP_TRY(h2d(c, dev_prog, prog.data(), prog_words * 8));
    GLP_TRY(f.tmp.get(&dev_alpha, (size_t)K * 2));
    GLP_TRY(h2d(c, dev_alpha, alphas, (size_t)K * 16));
    GLP_TRY(f.tmp.get(&dev_ap, (size_t)K * 2 * f.nopen));
    GLP_TRY(f.tmp.get(&dev_pp, (size_t)K * FCM_PP_WORDS));
    GLP_TRY(f.tmp.get(&fv, (size_t)K * 2 * g.n));
    GLP_TRY(f.tmp.get(&fcoef, (size_t)K * 2 * g.n));
    ta.alpha = dev_alpha; ta.open = f.dev_open; ta.z = f.dev_zs; ta.apow = dev_ap; ta.pp = dev_pp; ta.nopen = f.nopen;
    hipLaunchKernelGGL(k_fri_table, dim3((unsigned)f.pts.size(), K), dim3(256), 0, c->stream, ta);
    GLP_HIP(hipGetLastError());
    FCMArgs a;
    memset(&a, 0, sizeof(a));
    a.prog = (const FCColM *)dev_prog; a.nprog = (u32)prog.size(); a.npoints = (u32)f.pts.size();
    a.apow = dev_ap; a.pp = dev_pp; a.out = fv; a.nopen = f.nopen;
    a.w_n = root_of_unity(g.lg); a.g = GEN; a.lg = (u32)g.lg;
    if (g.lg >= 2 && g.lg <= 7) hipLaunchKernelGGL(k_fri_combine_many_small, dim3(1, K), dim3(256), 0, c->stream, a);      // 4..128 points: 256 / n lanes per point
    else hipLaunchKernelGGL(k_fri_combine_many, dim3(nblk(g.n), K), dim3(256), 0, c->stream, a);
    GLP_HIP(hipGetLastError());
    GLP_TRY(fri_values_to_coeffs(c, g, fv, fcoef));
    f.fri.start(fcoef, g.lg);
    f.stage = glp_fri::S_FRI;
    return GLP_OK;
}

// one layer of all K proofs -> f.cap [K][capn][4], and into the proofs
int fri_many_commit(glp_fri &f) {
    GLP_REQUIRE(f.stage == glp_fri::S_FRI && !f.layer_open && f.fri.layers.size() < f.nred, "glp_fri_commit: no layer left or beta pending");
    glp_ctx *c = f.c;
    const ProveGeo &g = f.g;
    StageScope st(c, "fri.commit", 0.0);
    const size_t r = f.fri.layers.size(), capw = (size_t)g.capn * 4;
    GLP_TRY(stage_fri_commit(c, g, f.tmp, f.fri));
    const FriLayer &ly = f.fri.layers.back();
    GLP_TRY(caps_to_host(c, ly.dig, ly.ndig * 4, merkle_cap_offset(((size_t)1 << ly.lgL) >> ly.ab, g.cap_height), g.capn, g.K, f.cap));
    for (u32 k = 0; k < g.K; k++) memcpy(fri_words(f, k) + r * capw, &f.cap[k * capw], capw * 8);
    f.layer_open = true;
    return GLP_OK;
}
// betas [K][2]
int fri_many_fold(glp_fri &f, const u64 *betas) {
    GLP_REQUIRE(f.stage == glp_fri::S_FRI && f.layer_open, "glp_fri_fold: call after glp_fri_commit");
    GLP_REQUIRE(betas, "beta is null");
    glp_ctx *c = f.c;
    const u32 K = f.g.K;
    for (u32 k = 0; k < K; k++) GLP_REQUIRE(betas[2 * k] < P && betas[2 * k + 1] < P, "beta[%u] is not canonical", k);
    StageScope st(c, "fri.fold", 0.0);
    u64 *dev_betas;
    GLP_TRY(f.tmp.get(&dev_betas, (size_t)K * 2));
    GLP_TRY(h2d(c, dev_betas, betas, (size_t)K * 16));
    GLP_TRY(stage_fri_fold(c, f.g, f.tmp, f.fri, e_from(0), dev_betas));
    f.layer_open = false;
    return GLP_OK;
}
// the K final polynomials (natural coefficient order) -> the proofs and coeffs_out [K][final_len][2]
int fri_many_final_poly(glp_fri &f, u64 *coeffs_out) {
    GLP_REQUIRE(f.stage == glp_fri::S_FRI && !f.layer_open && f.fri.layers.size() == f.nred, "glp_fri_final_poly: reductions not finished");
    const size_t fl = (size_t)1 << f.fri.lgcur;
    const u32 K = f.g.K;
    std::vector<u64> h((size_t)K * 2 * fl);
    GLP_TRY(d2h(f.c, h.data(), f.fri.cur, h.size() * 8));
    for (u32 k = 0; k < K; k++) {
        u64 *pf = fri_words(f, k) + f.o_final;
        for (size_t p = 0; p < fl; p++) {
            const size_t kk = bitrev32((u32)p, f.fri.lgcur);
            pf[2 * kk] = h[(size_t)k * 2 * fl + p];
            pf[2 * kk + 1] = h[(size_t)k * 2 * fl + fl + p];
        }
        if (coeffs_out) memcpy(coeffs_out + (size_t)k * 2 * fl, pf, fl * 16);
    }
    f.stage = glp_fri::S_FINAL;
    return GLP_OK;
}
// pow_witnesses [K], indices [K][nq]: every gather writes into a device image of the K query sections, one strided copy brings them back
int fri_many_queries(glp_fri &f, const u64 *pow_witnesses, const u64 *indices) {
    GLP_REQUIRE(f.stage == glp_fri::S_FINAL, "glp_fri_queries_many: call after glp_fri_final_poly");
    glp_ctx *c = f.c;
    const ProveGeo &g = f.g;
    const u32 K = g.K, nq = g.nq;
    for (u32 k = 0; k < K; k++)
        for (u32 q = 0; q < nq; q++)
            GLP_REQUIRE(indices[(size_t)k * nq + q] < (u64)g.N, "indices[%u][%u] = %llu outside the LDE domain", k, q,
                        (unsigned long long)indices[(size_t)k * nq + q]);
    for (u32 k = 0; k < K; k++) fri_words(f, k)[f.o_pow] = pow_witnesses[k];
    StageScope st(c, "fri.queries", 0.0);
    u64 *dev_idx, *dev_q;
    const size_t qsec = (size_t)nq * f.query_stride;
    GLP_TRY(f.tmp.get(&dev_idx, (size_t)K * nq));
    GLP_TRY(f.tmp.get(&dev_q, (size_t)K * qsec));
    GLP_TRY(h2d(c, dev_idx, indices, (size_t)K * nq * 8));
    size_t off = 0;
    for (const glp_batch *b : f.ob) GLP_TRY(queries_oracle(c, g, b, fri_shared(f, b), dev_idx, dev_q, f.query_stride, qsec, off));
    GLP_TRY(queries_layers(c, g, f.fri.layers, dev_idx, dev_q, f.query_stride, qsec, off));
    if (off != f.query_stride) return set_error(GLP_ERR_ARG, "internal: query record layout mismatch");
    GLP_HIP(hipMemcpy2DAsync(f.words.data() + f.o_queries, f.total * 8, dev_q, qsec * 8, qsec * 8, K, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    f.stage = glp_fri::S_DONE;
    return GLP_OK;
}

int fri_many_args(u32 num_proofs, const u64 *points) {
    GLP_REQUIRE(num_proofs >= 1 && num_proofs <= 4096, "num_proofs = %u outside 1..4096", num_proofs);
    GLP_REQUIRE(points, "points (the per-proof array [num_proofs][num_points][2]) is null");
    return GLP_OK;
}
// K sponges, each with the same number of pending inputs -> the smallest witness of each
int pow_search_many(glp_ctx *c, int hasher, const u64 *states, const u64 *pending, u32 npending, u32 bits, u32 K, u64 *witnesses) {
    StageScope stg(c, "fri_pow", 0.0);
    std::vector<u64> pst(states, states + (size_t)K * 12), best;
    for (u32 k = 0; k < K; k++)
        for (u32 i = 0; i < npending; i++) pst[(size_t)k * 12 + i] = pending[(size_t)k * npending + i];
    const std::vector<u32> ppos(K, npending);
    Tmp tmp(c);
    GLP_TRY(pow_search_batch(c, tmp, hasher, pst, ppos, bits, best));
    for (u32 k = 0; k < K; k++) {
        if (best[k] == ~0ull) return set_error(GLP_ERR_PROVE, "Proof of work failed. This is highly unlikely! (proof %u)", k);
        witnesses[k] = best[k];
    }
    return GLP_OK;
}
}  // namespace

extern "C" {
int glp_fri_begin_many(glp_ctx *c, const glp_fri_desc *desc, uint32_t num_proofs, const uint64_t *points, glp_fri **out) {
    GLP_REQUIRE(c && desc && out, "null argument");
    *out = nullptr;
    GLP_TRY(fri_many_args(num_proofs, points));
    GLP_TRY(fri_check(c, desc, num_proofs, points));
    GLP_TRY(bind(c));
    *out = new glp_fri(c, *desc, num_proofs, points);
    return GLP_OK;
}
uint32_t glp_fri_num_proofs(const glp_fri *f) { return f ? f->g.K : 0; }
int glp_fri_queries_many(glp_fri *f, const uint64_t *pow_witnesses, const uint64_t *indices) {
    GLP_REQUIRE(f != nullptr, "null glp_fri");
    GLP_TRY(bind(f->c));
    GLP_REQUIRE(pow_witnesses && indices, "null argument");
    GLP_REQUIRE(f->many, "glp_fri_queries_many: the handle comes from glp_fri_begin: glp_fri_queries");
    return fri_many_queries(*f, pow_witnesses, indices);
}
int glp_pow_search_many(glp_ctx *c, uint32_t hasher, uint32_t num_proofs, const uint64_t *sponge_states, const uint64_t *pending_inputs,
                        uint32_t num_pending, uint32_t bits, uint64_t *witnesses_out) {
    GLP_REQUIRE(c && sponge_states && witnesses_out && (pending_inputs || num_pending == 0), "null argument");
    GLP_REQUIRE(num_proofs >= 1 && num_proofs <= 4096, "num_proofs = %u outside 1..4096", num_proofs);
    GLP_REQUIRE(num_pending < 8, "proof of work: %u pending inputs (the rate is 8)", num_pending);
    GLP_REQUIRE(bits <= POW_MAX_BITS, "proof_of_work_bits=%u: this build searches at most 2^40 candidates and accepts up to %u bits", bits,
                POW_MAX_BITS);
    if (hasher != GLP_HASH_POSEIDON && hasher != GLP_HASH_KECCAK25) return set_error(GLP_ERR_UNSUPPORTED, "hasher %u is not one of GLP_HASH_*", hasher);
    GLP_TRY(bind(c));
    return pow_search_many(c, (int)hasher, sponge_states, pending_inputs, num_pending, bits, num_proofs, witnesses_out);
}
// the stepped sequence of K proofs driven by K of the library's transcripts on the context's host threads (fri/prover.rs `fri_proof` order)
int glp_fri_prove_many(glp_ctx *c, const glp_fri_desc *desc, uint32_t num_proofs, const uint64_t *points, const uint64_t *sponge_states,
                       const uint64_t *pending_inputs, uint32_t num_pending, uint64_t *openings_out, uint64_t *proofs_out) {
    GLP_REQUIRE(c && desc && sponge_states && openings_out && proofs_out && (pending_inputs || num_pending == 0), "null argument");
    GLP_REQUIRE(num_pending < 8, "%u pending inputs (the rate is 8)", num_pending);
    GLP_TRY(fri_many_args(num_proofs, points));
    GLP_TRY(fri_check(c, desc, num_proofs, points));
    GLP_TRY(bind(c));
    glp_fri f(c, *desc, num_proofs, points);
    const u32 K = num_proofs, capn = f.g.capn, nq = f.g.nq;
    const int hasher = f.g.hasher;
    HostPool &pool = ctx_host_pool(c);
    std::vector<Challenger> ch(K, Challenger(hasher));
    std::vector<u64> chal((size_t)K * 2);
    auto draw = [&] {
        pool.run(K, [&](size_t k) { const ext2 x = ch[k].get_ext(); chal[2 * k] = x.a; chal[2 * k + 1] = x.b; });
    };
    pool.run(K, [&](size_t k) {
        Challenger &t = ch[k];
        memcpy(t.st, sponge_states + k * 12, 96);
        for (u32 i = 0; i < num_pending; i++) t.in[i] = pending_inputs[k * num_pending + i];
        t.nin = (int)num_pending;
        // as in glp_fri_prove: with nothing pending the last observation permuted and refilled the output buffer
        if (num_pending == 0) { memcpy(t.out, t.st, 64); t.nout = 8; }
    });
    GLP_TRY(fri_many_open(f, openings_out));
    draw();
    GLP_TRY(fri_many_combine(f, chal.data()));
    for (u32 r = 0; r < f.nred; r++) {
        GLP_TRY(fri_many_commit(f));
        pool.run(K, [&](size_t k) {
            ch[k].observe_hashes(&f.cap[k * capn * 4], capn);
            const ext2 x = ch[k].get_ext();
            chal[2 * k] = x.a; chal[2 * k + 1] = x.b;
        });
        GLP_TRY(fri_many_fold(f, chal.data()));
    }
    GLP_TRY(fri_many_final_poly(f, nullptr));
    std::vector<u64> pst((size_t)K * 12), best;
    std::vector<u32> ppos(K);
    pool.run(K, [&](size_t k) {
        ch[k].observe(fri_words(f, (u32)k) + f.o_final, 2 * (size_t)f.final_len);
        memcpy(&pst[k * 12], ch[k].st, 96);
        for (int i = 0; i < ch[k].nin; i++) pst[k * 12 + i] = ch[k].in[i];
        ppos[k] = (u32)ch[k].nin;
    });
    for (u32 k = 0; k < K; k++) GLP_REQUIRE(ppos[k] < 8, "proof of work: %u pending inputs (the rate is 8)", ppos[k]);
    {
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
    GLP_TRY(fri_many_queries(f, best.data(), xi.data()));
    memcpy(proofs_out, f.words.data(), (size_t)K * f.total * 8);
    return GLP_OK;
}
}  // extern "C"
