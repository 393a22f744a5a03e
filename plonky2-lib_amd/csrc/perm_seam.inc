// perm_seam.inc -- glp_perm_*: the permutation argument of a circuit whose quotient stays with the caller (include/glp.h, "the
// permutation argument at the commitment seam").  Included by prover.hip beside fri_openings.inc.
//
// Two steps of plonky2's `prove_with_partition_witness` that are the same for every circuit, whatever its gates:
//   glp_perm_zs_commit        `wires_permutation_partial_products_and_zs` + the commitment of plonk_zs_partial_products: the K5 kernels
//                             of the library's own prover (launch_partial_products, prover_stages.inc), then batch_build
//   glp_perm_quotient_values  the permutation terms of `eval_vanishing_poly_base_batch` on the coset g <W_M>, reduced by the powers
//                             of alpha, the caller's gate share added, divided by Z_H: k_perm_quotient below
// No glp_circuit exists for such a caller: the shape comes from glp_perm_desc, the sigmas from any committed batch at a column
// offset, the challenges of all K proofs from one uploaded table.

// k_perm_quotient: the loop of k_quotient<NCH, 0> (quotient_kernels.inc) -- eight wire and eight sigma loads in flight, the lazy
// non-canonical product chain, beta k_j x chained by k_ratio when k_j = g^j, Acc160 against whole alpha powers, L_0 from k_l0_table --
// over operands the seam hands in.  The loop is a second copy, and a change to the chain belongs in both: a shared __forceinline__ body
// made k_quotient<2, 0> slower (profiles/r22_seam_one_body.txt).
//   sg / wl / zl      coset-major LDEs [columns][R][n] of three batches, `*_stride` words from one proof to the next (the leaf width
//                     times N, so the 4 salt planes of a salted batch are stepped over; 0 for sigmas shared by all proofs); sg points
//                     at the first sigma column
//   tab               [K][tab_stride]: betas[MAXCH], gammas[MAXCH], alpha powers [NCH][nt], nt = T + 1 (the last one multiplies the
//                     caller's gate sums); the proof is blockIdx.y
//   gate_sums / out   natural order on g <W_M>: index i = q S + r is slot q of evaluated plane r, LDE plane r 2^(rb - sb)
// The interleave goes through an LDS tile.  A block owns 256 consecutive natural indices = 256 / S slots of each of the S planes.
// Lane t computes (plane t / QL, slot t % QL), QL = 256 / S >= 16: a run of QL lanes reads QL consecutive words of one LDE plane
// (128 bytes at least).  Gate sums come in and results go out with lane t on natural index t, 2 KB per block and challenge, and
// change places in the tile [plane][slot] (pitch QL + 1).  A lane reads its gate sum from, and writes its result to, its own tile word, so
// one barrier on each side is enough.  The alternative of this code base, a lane that owns a slot and writes its S values side by
// side (k_coset_to_planes), would put S dependent ~1000-multiplication chains on one lane and leave a 2^3..2^7-row batch member
// with n lanes: here every (slot, plane) keeps a lane of its own, as in k_quotient, and the LDS traffic (two words per lane and
// challenge) is nothing against the chain.
struct PQArgs {
    const u64 *sg, *wl, *zl;
    size_t sg_stride, wl_stride, zl_stride;
    const u64 *k_is, *tab, *l0, *gate_sums;
    u64 *out;
    u64 shift_r[MAXR], zh_inv[MAXR];      // per evaluated plane r < S
    u64 w_n;
    u32 lg, rb, sb, nr, npp, qdf, nt, tab_stride, k_ratio;
};
constexpr int PQ_TILE = 256 + MAXR;       // S planes of QL + 1 words, S <= MAXR
template <int NCH>
__global__ __launch_bounds__(256, NCH == 4 ? 3 : 4) void k_perm_quotient(PQArgs a) {      // four challenges: 127 VGPRs and a spill under the four-wave bound
    __shared__ u64 tile[NCH][PQ_TILE];
    const u32 t = threadIdx.x, S = 1u << a.sb, lgql = 8 - a.sb, QL = 1u << lgql, pitch = QL + 1;
    const size_t n = (size_t)1 << a.lg, N = n << a.rb, M = n << a.sb;
    const size_t k = blockIdx.y, i0 = (size_t)blockIdx.x * 256, q0 = i0 >> a.sb;
    // natural index i0 + t = (q0 + (t >> sb)) S + (t & (S - 1))
    const bool nat_live = i0 + t < M;
    const u32 nat_pos = (t & (S - 1)) * pitch + (t >> a.sb);
    if (a.gate_sums) {
        if (nat_live) { _Pragma("unroll") for (int c = 0; c < NCH; c++) tile[c][nat_pos] = a.gate_sums[(k * NCH + c) * M + i0 + t]; }
        __syncthreads();
    }
    const u32 r = t >> lgql, ql = t & (QL - 1), own_pos = r * pitch + ql;
    const size_t q = q0 + ql;
    if (q < n) {
        const size_t plane = (size_t)r << (a.rb - a.sb);
        const size_t slot = plane * n + q, slot_next = plane * n + ((q + 1) & (n - 1));
        const u64 *wl = a.wl + k * a.wl_stride, *zl = a.zl + k * a.zl_stride, *sg = a.sg + k * a.sg_stride;
        const u64 *tb = a.tab + k * a.tab_stride, *apow = tb + 2 * MAXCH;
        u64 betas[NCH], gammas[NCH];
        _Pragma("unroll") for (int c = 0; c < NCH; c++) { betas[c] = tb[c]; gammas[c] = tb[MAXCH + c]; }
        const u64 x = mul(a.shift_r[r], dpow(a.w_n, q));
        constexpr u32 nch = NCH; const u32 nchunks = a.npp + 1, nt = a.nt;
        u64 zx[NCH], zg[NCH];
        Acc160 pa[NCH];
        _Pragma("unroll") for (int c = 0; c < NCH; c++) { acc_zero(pa[c]); zx[c] = zl[(size_t)c * N + slot]; zg[c] = zl[(size_t)c * N + slot_next]; }
        const u64 l0 = a.l0[(size_t)r * n + q];
        _Pragma("unroll") for (int c = 0; c < NCH; c++) {
            const u64 v = mul(l0, sub(zx[c], 1));
            _Pragma("unroll") for (int c2 = 0; c2 < NCH; c2++) acc_fma(pa[c2], v, apow[c2 * nt + c]);
        }
        u64 bkx[NCH];                                      // beta_c k_j x for the next wire j (k_ratio path)
        _Pragma("unroll") for (int c = 0; c < NCH; c++) bkx[c] = mul_nc(betas[c], x);
        for (u32 chunk = 0; chunk < nchunks; chunk++) {
            u64 num[NCH], den[NCH];
            _Pragma("unroll") for (int c = 0; c < NCH; c++) { num[c] = 1; den[c] = 1; }
            const u32 j0 = chunk * a.qdf, j1 = min((chunk + 1) * a.qdf, a.nr);
            for (u32 jb = j0; jb < j1; jb += 8) {          // eight wire + eight sigma loads in flight
                u64 w8[8], s8[8];
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (jb + e < j1) { w8[e] = wl[(size_t)(jb + e) * N + slot]; s8[e] = sg[(size_t)(jb + e) * N + slot]; }
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (jb + e < j1) {
                        // the lazy chain of k_quotient: running products and beta terms stay non-canonical u64, only w + gamma is a
                        // canonical addition; with k_j = g^j, beta k_j x is the previous wire's value times g
                        u64 kx = 0;
                        if (!a.k_ratio) kx = mul_nc(a.k_is[jb + e], x);
                        _Pragma("unroll") for (int c = 0; c < NCH; c++) {
                            const u64 wg = add(w8[e], gammas[c]);
                            const u64 bk = a.k_ratio ? bkx[c] : mul_nc(betas[c], kx);
                            num[c] = mul_nc_cc(num[c], add_cnc(wg, bk));
                            den[c] = mul_nc_cc(den[c], add_cnc(wg, mul_nc_cc(betas[c], s8[e])));
                            if (a.k_ratio) bkx[c] = mul_small_nc(bkx[c], a.k_ratio);
                        }
                    }
            }
            _Pragma("unroll") for (int c = 0; c < NCH; c++) {
                const u64 prev = chunk == 0 ? zx[c] : zl[(size_t)(nch + c * a.npp + chunk - 1) * N + slot];
                const u64 next = chunk == nchunks - 1 ? zg[c] : zl[(size_t)(nch + c * a.npp + chunk) * N + slot];
                const u64 v = sub(mul(prev, num[c]), mul(next, den[c]));
                const u32 kt = nch + c * nchunks + chunk;
                _Pragma("unroll") for (int c2 = 0; c2 < NCH; c2++) acc_fma(pa[c2], v, apow[c2 * nt + kt]);
            }
        }
        const u64 zhi = a.zh_inv[r];
        _Pragma("unroll") for (int c = 0; c < NCH; c++) {
            if (a.gate_sums) acc_fma(pa[c], tile[c][own_pos], apow[c * nt + nt - 1]);
            tile[c][own_pos] = mul(acc_reduce(pa[c]), zhi);
        }
    }
    __syncthreads();
    if (nat_live) { _Pragma("unroll") for (int c = 0; c < NCH; c++) a.out[(k * NCH + c) * M + i0 + t] = tile[c][nat_pos]; }
}

namespace {
struct PermShape { u32 lg, nw, nr, nch, qdf, npp, nzp, k_ratio; };
// the description's own rules; `fn` names the entry point in the message
int perm_desc_check(const char *fn, const glp_perm_desc *d, PermShape &s) {
    GLP_REQUIRE(d, "%s: desc is null", fn);
    GLP_REQUIRE(d->log_n <= (u32)NTT_MAX_LG, "%s: desc.log_n = %u is more than %d", fn, d->log_n, NTT_MAX_LG);
    GLP_REQUIRE(d->num_challenges >= 1 && d->num_challenges <= (u32)MAXCH, "%s: desc.num_challenges = %u outside 1..%d", fn, d->num_challenges, MAXCH);
    GLP_REQUIRE(d->num_routed_wires >= 1 && d->num_routed_wires <= d->num_wires, "%s: desc.num_routed_wires = %u outside 1..num_wires = %u", fn,
                d->num_routed_wires, d->num_wires);
    GLP_REQUIRE(d->chunk_size >= 1, "%s: desc.chunk_size is 0", fn);
    GLP_REQUIRE(d->k_is, "%s: desc.k_is is null", fn);
    const size_t bad = first_noncanonical(d->k_is, d->num_routed_wires);
    GLP_REQUIRE(bad == d->num_routed_wires, "%s: desc.k_is[%zu] = 0x%016llx is not a canonical field element (>= p)", fn, bad,
                (unsigned long long)d->k_is[bad == d->num_routed_wires ? 0 : bad]);
    s.lg = d->log_n; s.nw = d->num_wires; s.nr = d->num_routed_wires; s.nch = d->num_challenges; s.qdf = d->chunk_size;
    s.npp = (u32)(((u64)s.nr + s.qdf - 1) / s.qdf) - 1;
    GLP_REQUIRE((u64)s.nch * (1 + s.npp) <= 0x7FFFFFFFu, "%s: desc: num_challenges * (1 + num_partial_products) does not fit", fn);
    s.nzp = s.nch * (1 + s.npp);
    s.k_ratio = coset_shift_ratio(d->k_is, s.nr);
    return GLP_OK;
}
// [num_proofs][num_challenges] host challenges, canonical or refused by name
int perm_challenges_check(const char *fn, const char *name, const u64 *v, u32 K, u32 nch) {
    GLP_REQUIRE(v, "%s: %s is null", fn, name);
    const size_t cnt = (size_t)K * nch, bad = first_noncanonical(v, cnt);
    GLP_REQUIRE(bad == cnt, "%s: %s[%zu][%zu] = 0x%016llx is not a canonical field element (>= p)", fn, name, bad / nch, bad % nch,
                (unsigned long long)v[bad == cnt ? 0 : bad]);
    return GLP_OK;
}
// the number of proofs one seam call takes in lock step
constexpr u32 SEAM_MAX_PROOFS = 4096;
int seam_num_proofs_check(const char *fn, u32 K) {
    GLP_REQUIRE(K >= 1 && K <= SEAM_MAX_PROOFS, "%s: num_proofs = %u outside 1..%u", fn, K, SEAM_MAX_PROOFS);
    return GLP_OK;
}
}  // namespace

extern "C" {

uint32_t glp_perm_num_polys(const glp_perm_desc *desc) {
    PermShape s;
    return perm_desc_check("glp_perm_num_polys", desc, s) == GLP_OK ? s.nzp : 0;
}

int glp_perm_zs_commit(glp_ctx *c, const glp_perm_desc *desc, uint32_t num_proofs, const uint64_t *wires, int wires_on_device,
                       const uint64_t *sigmas, int sigmas_on_device, const uint64_t *betas, const uint64_t *gammas, uint32_t rate_bits,
                       uint32_t cap_height, uint32_t hasher, const uint64_t *seed, glp_batch **out) {
    static const char *fn = "glp_perm_zs_commit";
    GLP_REQUIRE(out, "%s: out is null", fn);
    *out = nullptr;
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    PermShape s;
    GLP_TRY(perm_desc_check(fn, desc, s));
    GLP_REQUIRE(wires, "%s: wires is null", fn);
    GLP_REQUIRE(sigmas, "%s: sigmas is null", fn);
    const u32 K = num_proofs;
    GLP_TRY(seam_num_proofs_check(fn, K));
    // an argument error here, as every refusal of this entry point (batch_shape_check's is GLP_ERR_UNSUPPORTED)
    GLP_REQUIRE(hasher == GLP_HASH_POSEIDON || hasher == GLP_HASH_KECCAK25, "%s: hasher = %u is not one of GLP_HASH_*", fn, hasher);
    GLP_TRY(batch_shape_check(fn, K, s.nzp, s.lg, rate_bits, cap_height, hasher, BATCH_MAX_BYTES));
    GLP_TRY(perm_challenges_check(fn, "betas", betas, K, s.nch));
    GLP_TRY(perm_challenges_check(fn, "gammas", gammas, K, s.nch));
    const size_t n = (size_t)1 << s.lg;
    GLP_REQUIRE((size_t)K * s.nw <= BATCH_MAX_BYTES / (8 * n), "%s: wires too large (num_proofs * num_wires * 2^log_n words)", fn);
    if (!wires_on_device) GLP_TRY(host_field_check(c, fn, "wires", wires, K, s.nw, n));
    if (!sigmas_on_device) GLP_TRY(host_field_check(c, fn, "sigmas", sigmas, 0, s.nr, n));
    GLP_TRY(bind(c));
    u64 sd[4];
    if (seed) for (int i = 0; i < 4; i++) sd[i] = canon(seed[i]);
    Scratch tmp(c);
    const u64 *dev_wires, *dev_sigmas;
    GLP_TRY(tmp.input(wires, wires_on_device, (size_t)K * s.nw * n, &dev_wires));
    GLP_TRY(tmp.input(sigmas, sigmas_on_device, (size_t)s.nr * n, &dev_sigmas));
    // one table: k_is [nr], then chal [K][2 MAXCH] (betas, gammas), the layout k_pp_rows reads
    std::vector<u64> tab((size_t)s.nr + (size_t)K * 2 * MAXCH, 0);
    memcpy(tab.data(), desc->k_is, (size_t)s.nr * 8);
    for (u32 k = 0; k < K; k++)
        for (u32 i = 0; i < s.nch; i++) {
            tab[s.nr + (size_t)k * 2 * MAXCH + i] = betas[(size_t)k * s.nch + i];
            tab[s.nr + (size_t)k * 2 * MAXCH + MAXCH + i] = gammas[(size_t)k * s.nch + i];
        }
    u64 *dev_tab, *zp, *dens, *tot;
    GLP_TRY(tmp.words(&dev_tab, tab.size()));
    GLP_TRY(h2d(c, dev_tab, tab.data(), tab.size() * 8));
    GLP_TRY(tmp.words(&zp, (size_t)K * s.nzp * n));
    GLP_TRY(tmp.words(&dens, (size_t)K * s.nzp * n));
    GLP_TRY(tmp.words(&tot, (size_t)K * s.nch * nblk(n)));
    {
        StageScope st(c, "perm.partial_products", 8.0 * n * K * (2.0 * s.nr + s.nzp));
        const PermGeo pg = {(int)s.lg, s.nw, s.nr, s.nch, s.npp, s.qdf, K};
        GLP_TRY(launch_partial_products(c, pg, dev_wires, dev_sigmas, dev_tab, nullptr, nullptr, dev_tab + s.nr, zp, dens, tot));
    }
    return batch_build(c, zp, BATCH_VALUES, s.nzp, (int)s.lg, (int)rate_bits, (int)cap_height, out, nullptr, K, (int)hasher, seed ? sd : nullptr,
                       GLP_SALT_TAG_BATCH);
}

int glp_perm_quotient_values(glp_ctx *c, const glp_perm_desc *desc, uint32_t num_proofs, const glp_batch *sigmas_oracle, uint32_t sigma_col_begin,
                             const glp_batch *wires_oracle, const glp_batch *zs_oracle, uint32_t sub_bits, const uint64_t *betas,
                             const uint64_t *gammas, const uint64_t *alphas, const uint64_t *gate_sums, int gate_sums_on_device, uint64_t *out,
                             int out_on_device) {
    static const char *fn = "glp_perm_quotient_values";
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    PermShape s;
    GLP_TRY(perm_desc_check(fn, desc, s));
    GLP_REQUIRE(sigmas_oracle, "%s: sigmas_oracle is null", fn);
    GLP_REQUIRE(wires_oracle, "%s: wires_oracle is null", fn);
    GLP_REQUIRE(zs_oracle, "%s: zs_oracle is null", fn);
    GLP_REQUIRE(out, "%s: out is null", fn);
    const u32 K = num_proofs;
    GLP_TRY(seam_num_proofs_check(fn, K));
    const glp_batch *sb = sigmas_oracle, *wb = wires_oracle, *zb = zs_oracle;
    GLP_REQUIRE(sb->ctx == c && wb->ctx == c && zb->ctx == c, "%s: an oracle belongs to another ctx", fn);
    GLP_REQUIRE((u32)wb->lg == s.lg && (u32)sb->lg == s.lg && (u32)zb->lg == s.lg, "%s: log_n disagrees: desc %u, sigmas_oracle %d, wires_oracle %d, zs_oracle %d",
                fn, s.lg, sb->lg, wb->lg, zb->lg);
    GLP_REQUIRE(sb->rate_bits == wb->rate_bits && zb->rate_bits == wb->rate_bits, "%s: rate_bits disagrees: sigmas_oracle %d, wires_oracle %d, zs_oracle %d",
                fn, sb->rate_bits, wb->rate_bits, zb->rate_bits);
    const u32 rb = (u32)wb->rate_bits;
    GLP_REQUIRE(sub_bits <= rb, "%s: sub_bits = %u is more than rate_bits = %u", fn, sub_bits, rb);
    GLP_REQUIRE(s.qdf <= (1u << sub_bits), "%s: desc.chunk_size = %u is more than 2^sub_bits = %u: the chunk check would exceed the quotient's degree", fn,
                s.qdf, 1u << sub_bits);
    GLP_REQUIRE(wb->ncols >= s.nw, "%s: wires_oracle has %u polynomials, desc.num_wires is %u", fn, wb->ncols, s.nw);
    GLP_REQUIRE(zb->ncols == s.nzp, "%s: zs_oracle has %u polynomials, glp_perm_num_polys is %u", fn, zb->ncols, s.nzp);
    GLP_REQUIRE((u64)sigma_col_begin + s.nr <= sb->ncols, "%s: sigma_col_begin + num_routed_wires = %u + %u runs past the %u polynomials of sigmas_oracle (salts are not polynomials)",
                fn, sigma_col_begin, s.nr, sb->ncols);
    GLP_REQUIRE(wb->K == K, "%s: wires_oracle has %u members, num_proofs is %u", fn, wb->K, K);
    GLP_REQUIRE(zb->K == K, "%s: zs_oracle has %u members, num_proofs is %u", fn, zb->K, K);
    GLP_REQUIRE(sb->K == K || sb->K == 1, "%s: sigmas_oracle has %u members, neither 1 nor num_proofs = %u", fn, sb->K, K);
    GLP_TRY(perm_challenges_check(fn, "betas", betas, K, s.nch));
    GLP_TRY(perm_challenges_check(fn, "gammas", gammas, K, s.nch));
    GLP_TRY(perm_challenges_check(fn, "alphas", alphas, K, s.nch));
    const u32 nch = s.nch, S = 1u << sub_bits, nt = nch * (s.npp + 2) + 1;
    const size_t n = (size_t)1 << s.lg, N = n << rb, M = n << sub_bits, words = (size_t)K * nch * M;
    if (gate_sums && !gate_sums_on_device) GLP_TRY(host_field_check(c, fn, "gate_sums", gate_sums, K, nch, M));
    GLP_TRY(bind(c));
    Scratch tmp(c);
    // one table: k_is [nr], then per proof betas[MAXCH], gammas[MAXCH], alpha powers [nch][nt]
    const u32 tab_stride = 2 * MAXCH + nch * nt;
    std::vector<u64> tab((size_t)s.nr + (size_t)K * tab_stride, 0);
    memcpy(tab.data(), desc->k_is, (size_t)s.nr * 8);
    for (u32 k = 0; k < K; k++) {
        u64 *tk = tab.data() + s.nr + (size_t)k * tab_stride;
        for (u32 i = 0; i < nch; i++) {
            tk[i] = betas[(size_t)k * nch + i];
            tk[MAXCH + i] = gammas[(size_t)k * nch + i];
            alpha_powers(alphas[(size_t)k * nch + i], nt, tk + 2 * MAXCH + (size_t)i * nt);
        }
    }
    u64 *dev_tab, *l0t;
    GLP_TRY(tmp.words(&dev_tab, tab.size()));
    GLP_TRY(h2d(c, dev_tab, tab.data(), tab.size() * 8));
    GLP_TRY(tmp.words(&l0t, (size_t)S * n));
    const u64 *dev_gs = nullptr;
    if (gate_sums) GLP_TRY(tmp.input(gate_sums, gate_sums_on_device, words, &dev_gs));
    u64 *dev_out = out;
    if (!out_on_device) GLP_TRY(tmp.words(&dev_out, words));

    PQArgs a;
    memset(&a, 0, sizeof(a));
    L0Args la;
    coset_plane_tables((int)s.lg, (int)sub_bits, S, 1, la, a.zh_inv);
    memcpy(a.shift_r, la.shift_r, sizeof(u64) * S);
    a.w_n = la.w_n;
    a.sg = sb->lde + (size_t)sigma_col_begin * N; a.wl = wb->lde; a.zl = zb->lde;
    a.sg_stride = sb->K == 1 ? 0 : (size_t)(sb->ncols + sb->salt) * N;
    a.wl_stride = (size_t)(wb->ncols + wb->salt) * N; a.zl_stride = (size_t)(zb->ncols + zb->salt) * N;
    a.k_is = dev_tab; a.tab = dev_tab + s.nr; a.l0 = l0t; a.gate_sums = dev_gs; a.out = dev_out;
    a.lg = s.lg; a.rb = rb; a.sb = sub_bits; a.nr = s.nr; a.npp = s.npp; a.qdf = s.qdf; a.nt = nt; a.tab_stride = tab_stride; a.k_ratio = s.k_ratio;
    {
        StageScope st(c, "perm.quotient_values", 8.0 * M * K * (2.0 * s.nr + s.nzp + (gate_sums ? 2.0 : 1.0) * nch));
        hipLaunchKernelGGL(k_l0_table, dim3(nblk(n)), dim3(256), 0, c->stream, la, l0t, S);
        GLP_HIP(hipGetLastError());
        const dim3 grid(nblk(M), K);
        GLP_LAUNCH_NCH(k_perm_quotient, nch, grid, dim3(256), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
    }
    if (!out_on_device) GLP_TRY(d2h(c, out, dev_out, words * 8));
    return GLP_OK;
}

}  // extern "C"
