// zeta_check.inc -- glp_gate_program_eval_ext and glp_perm_check_zeta: the vanishing identity at zeta of a circuit whose gates stay
// with the caller (include/glp.h, "the vanishing identity at zeta for caller-held circuits").  Included by prover.hip behind
// gate_program.inc; it reads that file's program object and LDS symbol.
//
// plonky2's `verify_with_challenges` checks, before it looks at FRI,
//     vanishing(zeta) == Z_H(zeta) * reduce_with_powers(quotient chunks, zeta^n).
// For a seam caller the gate share of vanishing(zeta) is its gate program read over F_p^2: COL is the opening at zeta, COL_NEXT the
// opening at w_n zeta, X is zeta, IMM and PARAM are embedded base elements and ADD / SUB / MUL are the F_p^2 operations.  The rest is
// the algebra of verify_vanishing (verify_host.h) with the gate terms handed in.
//
// k_gate_program_ext: one lane per proof, one wave per block, so that 4096 proofs spread over 64 CUs.  What is wave-uniform stays on
// the scalar side exactly as in k_gate_program: instruction words through the uniform pointer into the zero-padded device copy (four
// words per scalar load), scalar decode, uniform branches, the pool through a uniform pointer.  What a lane owns:
//   registers     in LDS, two words per register, word h of register r of lane t at (2 r + h) * ZX_BLOCK + t: consecutive lanes 8 bytes
//                 apart, conflict-free, a lane only ever touches its own column -- no barrier.  num_regs * 1 KB, dynamic.
//   openings, point, params, alphas   per proof, vector loads; every word of an opening or a point is reduced once as it is loaded
//   alpha powers  built in this launch: pw_c = alpha_c^t is carried in registers, one multiplication per EMIT and challenge, and
//                 starts again at 1 behind every END -- no table, whatever the largest gate
//   acc_c, total_c  canonical F_p^2 elements: EMIT is acc_c += a * pw_c (a scaling), END is total_c += acc_c * a (a product)
constexpr int ZX_BLOCK = 64;
struct ZXArgs {
    const u64 *code, *pool;
    const u64 *at0, *at1, *at2, *at3, *nx0, *nx1, *nx2, *nx3;      // the openings of oracle 0..3 at the point and at w_n * point
    size_t st0, st1, st2, st3;                                     // words from one proof to the next
    const u64 *points, *alphas, *params;                           // [K][2], [K][NCH], [K][nparams]
    u64 *out;                                                      // [K][NCH][2]
    u32 K, ninstr, nregs, nparams;
};
__device__ __forceinline__ ext2 zx_rd(const u64 *p) { return e_make(canon(p[0]), canon(p[1])); }
// One operand: f is its 27 bits, wave-uniform, so the switch is a scalar branch; the oracle's base and stride are picked by scalar selects.
__device__ __forceinline__ ext2 zx_operand(u32 f, const u64 *regs, const ZXArgs &a, size_t k, const u64 *prm, ext2 x) {
    const u32 kind = f & 7, pl = f >> 3;
    switch (kind) {
    case GLP_GP_REG: return e_make(regs[(size_t)(2 * pl) * ZX_BLOCK], regs[(size_t)(2 * pl + 1) * ZX_BLOCK]);
    case GLP_GP_COL: case GLP_GP_COL_NEXT: {
        const u32 o = pl >> GLP_GP_COL_ORACLE_SHIFT, col = pl & ((1u << GLP_GP_COL_ORACLE_SHIFT) - 1);
        const u64 *b = kind == GLP_GP_COL ? (o == 0 ? a.at0 : o == 1 ? a.at1 : o == 2 ? a.at2 : a.at3)
                                          : (o == 0 ? a.nx0 : o == 1 ? a.nx1 : o == 2 ? a.nx2 : a.nx3);
        const size_t st = o == 0 ? a.st0 : o == 1 ? a.st1 : o == 2 ? a.st2 : a.st3;
        return zx_rd(b + k * st + 2 * (size_t)col);
    }
    case GLP_GP_IMM: return e_from(a.pool[pl]);
    case GLP_GP_PARAM: return e_from(prm[pl]);
    default: return x;
    }
}
template <int NCH>
__global__ __launch_bounds__(ZX_BLOCK) void k_gate_program_ext(ZXArgs a) {
    const u32 t = threadIdx.x;
    const size_t k = (size_t)blockIdx.x * ZX_BLOCK + t;
    if (k >= a.K) return;                                          // no barrier below
    u64 *regs = gp_lds + t;
    const u64 *prm = a.params + k * a.nparams;
    const ext2 x = zx_rd(a.points + 2 * k);
    u64 alpha[NCH], pw[NCH];
    ext2 acc[NCH], tot[NCH];
    _Pragma("unroll") for (int c = 0; c < NCH; c++) { alpha[c] = a.alphas[k * NCH + c]; pw[c] = 1; acc[c] = tot[c] = e_from(0); }
    for (u32 pc = 0; pc < a.ninstr; pc += 4) {
        const u64 w[4] = {a.code[pc], a.code[pc + 1], a.code[pc + 2], a.code[pc + 3]};      // one scalar load
        _Pragma("unroll") for (int j = 0; j < 4; j++) {
            const u64 ins = w[j];
            const u32 op = (u32)ins & 15;
            if (op == 0) continue;
            const ext2 va = zx_operand((u32)(ins >> GLP_GP_A_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), regs, a, k, prm, x);
            if (op <= GLP_GP_OP_MOV) {
                ext2 v = va;
                if (op != GLP_GP_OP_MOV) {
                    const ext2 vb = zx_operand((u32)(ins >> GLP_GP_B_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), regs, a, k, prm, x);
                    v = op == GLP_GP_OP_ADD ? e_add(va, vb) : op == GLP_GP_OP_SUB ? e_sub(va, vb) : e_mul(va, vb);
                }
                const u32 dst = ((u32)ins >> GLP_GP_DST_SHIFT) & 31;
                regs[(size_t)(2 * dst) * ZX_BLOCK] = v.a;
                regs[(size_t)(2 * dst + 1) * ZX_BLOCK] = v.b;
            } else if (op == GLP_GP_OP_EMIT) {
                _Pragma("unroll") for (int c = 0; c < NCH; c++) { acc[c] = e_add(acc[c], e_scale(va, pw[c])); pw[c] = mul(pw[c], alpha[c]); }
            } else {
                _Pragma("unroll") for (int c = 0; c < NCH; c++) { tot[c] = e_add(tot[c], e_mul(acc[c], va)); acc[c] = e_from(0); pw[c] = 1; }
            }
        }
    }
    _Pragma("unroll") for (int c = 0; c < NCH; c++) {
        a.out[(k * NCH + c) * 2] = tot[c].a;
        a.out[(k * NCH + c) * 2 + 1] = tot[c].b;
    }
}

// k_perm_check_zeta: one lane per (proof, challenge); the algebra of verify_vanishing in its order of terms.  Lane (k, c) walks the
// terms of every challenge j (they all enter challenge c's sum, against powers of alpha_c): a chain of about 2 num_challenges
// num_routed_wires products in F_p^2, untuned -- it is nothing beside the program.  verdict: 0 the identity holds, 1 it does not, 2 zeta = 1.
struct ZPArgs {
    const u64 *sg, *wl, *zs, *zn, *qt;
    size_t sg_st, wl_st, zs_st, qt_st;
    const u64 *zetas, *k_is, *chal, *gate_sums;                    // chal [K][3][MAXCH]: betas, gammas, alphas
    u32 *verdict;                                                  // [K][nch]
    u64 n_field;
    u32 K, lg, nr, nch, npp, qdf, chunks;
};
__global__ __launch_bounds__(ZX_BLOCK) void k_perm_check_zeta(ZPArgs a) {
    const size_t i = (size_t)blockIdx.x * ZX_BLOCK + threadIdx.x;
    if (i >= (size_t)a.K * a.nch) return;
    const size_t k = i / a.nch;
    const u32 c = (u32)(i % a.nch), nch = a.nch, npp = a.npp;
    const u64 *sg = a.sg + k * a.sg_st, *wl = a.wl + k * a.wl_st, *zs = a.zs + k * a.zs_st, *zn = a.zn + k * a.zs_st, *qt = a.qt + k * a.qt_st;
    const u64 *ch = a.chal + k * 3 * MAXCH;
    const ext2 zeta = zx_rd(a.zetas + 2 * k), one = e_from(1);
    if (e_eq(zeta, one)) { a.verdict[i] = 2; return; }
    ext2 zpow = zeta;
    for (u32 b = 0; b < a.lg; b++) zpow = e_sqr(zpow);
    const ext2 zh = e_sub(zpow, one);
    const ext2 l0 = e_mul(zh, e_inv(e_scale(e_sub(zeta, one), a.n_field)));
    const u64 alpha = ch[2 * MAXCH + c];
    ext2 van = e_from(0);
    u64 ap = 1;                                                    // alpha^t of the next term
    for (u32 j = 0; j < nch; j++) {
        van = e_add(van, e_scale(e_mul(l0, e_sub(zx_rd(zs + 2 * j), one)), ap));
        ap = mul(ap, alpha);
    }
    for (u32 j = 0; j < nch; j++) {
        const u64 beta = ch[j];
        const ext2 gamma = e_from(ch[MAXCH + j]);
        for (u32 chunk = 0; chunk <= npp; chunk++) {
            ext2 num = one, den = one;
            const u32 w1 = min((chunk + 1) * a.qdf, a.nr);
            for (u32 w = chunk * a.qdf; w < w1; w++) {
                const ext2 wg = e_add(zx_rd(wl + 2 * (size_t)w), gamma);
                num = e_mul(num, e_add(wg, e_scale(zeta, mul(a.k_is[w], beta))));
                den = e_mul(den, e_add(wg, e_scale(zx_rd(sg + 2 * (size_t)w), beta)));
            }
            const ext2 prev = zx_rd(zs + 2 * (size_t)(chunk == 0 ? j : nch + j * npp + chunk - 1));
            const ext2 next = zx_rd(chunk == npp ? zn + 2 * j : zs + 2 * (size_t)(nch + j * npp + chunk));
            van = e_add(van, e_scale(e_sub(e_mul(prev, num), e_mul(next, den)), ap));
            ap = mul(ap, alpha);
        }
    }
    if (a.gate_sums) van = e_add(van, e_scale(zx_rd(a.gate_sums + 2 * i), ap));      // ap = alpha^T
    ext2 q = e_from(0);
    for (u32 j = a.chunks; j-- > 0;) q = e_add(e_mul(q, zpow), zx_rd(qt + 2 * ((size_t)c * a.chunks + j)));
    a.verdict[i] = e_eq(van, e_mul(zh, q)) ? 0 : 1;
}

namespace {
// One glp_ext_openings argument: `polys` polynomials are read at the point, `next_polys` at w_n * point (0: at_next is not looked at).
// Refused by name; host words are scanned per proof.  Then the device pointers: the caller's own, or copies of the words in use.
int ext_openings_check(const char *fn, const char *name, const glp_ext_openings *o, u32 polys, u32 next_polys, u32 K, int on_device) {
    GLP_REQUIRE(o->at, "%s: %s.at is null", fn, name);
    GLP_REQUIRE(o->at_next || next_polys == 0, "%s: %s.at_next is null, and %u of its polynomials are read at w_n * point", fn, name, next_polys);
    GLP_REQUIRE(o->proof_stride >= 2 * (size_t)polys, "%s: %s.proof_stride = %zu is less than 2 * %u polynomials read", fn, name, o->proof_stride, polys);
    GLP_REQUIRE(o->proof_stride <= ((size_t)1 << 32), "%s: %s.proof_stride = %zu is more than 2^32", fn, name, o->proof_stride);
    if (on_device) return GLP_OK;
    for (u32 k = 0; k < K; k++) {
        size_t bad = first_noncanonical(o->at + k * o->proof_stride, 2 * (size_t)polys);
        GLP_REQUIRE(bad == 2 * (size_t)polys, "%s: %s.at: proof %u, word %zu = 0x%016llx is not a canonical field element (>= p)", fn, name, k, bad,
                    (unsigned long long)o->at[k * o->proof_stride + (bad == 2 * (size_t)polys ? 0 : bad)]);
        if (!next_polys) continue;
        bad = first_noncanonical(o->at_next + k * o->proof_stride, 2 * (size_t)next_polys);
        GLP_REQUIRE(bad == 2 * (size_t)next_polys, "%s: %s.at_next: proof %u, word %zu = 0x%016llx is not a canonical field element (>= p)", fn, name, k, bad,
                    (unsigned long long)o->at_next[k * o->proof_stride + (bad == 2 * (size_t)next_polys ? 0 : bad)]);
    }
    return GLP_OK;
}
// HBM openings are read where they are.  Of host openings only the words that are read travel: packed [K][2 polys], the openings at
// w_n * point in a second block of the same pitch (next_polys <= polys), so six views of one openings array are not six copies of it.
int ext_openings_input(Scratch &tmp, const glp_ext_openings *o, u32 polys, u32 next_polys, u32 K, int on_device, const u64 **at, const u64 **nx,
                       size_t *stride) {
    *at = on_device ? o->at : nullptr;
    *nx = on_device && next_polys ? o->at_next : nullptr;
    *stride = on_device ? o->proof_stride : 2 * (size_t)polys;
    if (on_device || !polys) return GLP_OK;
    const size_t pitch = 2 * (size_t)polys;
    std::vector<u64> pack((size_t)K * pitch * (next_polys ? 2 : 1), 0);
    for (u32 k = 0; k < K; k++) {
        memcpy(pack.data() + k * pitch, o->at + k * o->proof_stride, pitch * 8);
        if (next_polys) memcpy(pack.data() + ((size_t)K + k) * pitch, o->at_next + k * o->proof_stride, 2 * (size_t)next_polys * 8);
    }
    u64 *d;
    GLP_TRY(tmp.words(&d, pack.size()));
    GLP_TRY(h2d(tmp.c, d, pack.data(), pack.size() * 8));
    *at = d;
    if (next_polys) *nx = d + (size_t)K * pitch;
    return GLP_OK;
}
// [K][2] host points, canonical or refused naming proof and word
int ext_points_check(const char *fn, const char *name, const u64 *v, u32 K, u32 per_proof) {
    const size_t cnt = (size_t)K * per_proof, bad = first_noncanonical(v, cnt);
    GLP_REQUIRE(bad == cnt, "%s: %s: proof %zu, word %zu = 0x%016llx is not a canonical field element (>= p)", fn, name, bad / per_proof, bad % per_proof,
                (unsigned long long)v[bad == cnt ? 0 : bad]);
    return GLP_OK;
}
}  // namespace

extern "C" {

int glp_gate_program_eval_ext(glp_ctx *c, const glp_gate_program *p, uint32_t num_proofs, uint32_t num_challenges, const uint64_t *points,
                              const glp_ext_openings *openings, int inputs_on_device, const uint64_t *alphas, const uint64_t *params,
                              uint64_t *out, int out_on_device) {
    static const char *fn = "glp_gate_program_eval_ext";
    GLP_TRY(gate_program_handle_check(fn, c, p));
    GLP_REQUIRE(points, "%s: points is null", fn);
    GLP_REQUIRE(openings, "%s: openings is null", fn);
    GLP_REQUIRE(out, "%s: out is null", fn);
    const u32 K = num_proofs, nch = num_challenges;
    GLP_TRY(seam_num_proofs_check(fn, K));
    GLP_REQUIRE(nch >= 1 && nch <= (u32)MAXCH, "%s: num_challenges = %u outside 1..%d", fn, nch, MAXCH);
    char name[32];
    for (u32 o = 0; o < p->noracles; o++) {
        snprintf(name, sizeof(name), "openings[%u]", o);
        GLP_TRY(ext_openings_check(fn, name, openings + o, p->oracle_cols[o], p->next_mask >> o & 1 ? p->oracle_cols[o] : 0, K, inputs_on_device));
    }
    if (!inputs_on_device) GLP_TRY(ext_points_check(fn, "points", points, K, 2));
    GLP_TRY(perm_challenges_check(fn, "alphas", alphas, K, nch));
    GLP_TRY(gate_program_params_check(fn, p, params, K));
    GLP_TRY(bind(c));
    Scratch tmp(c);
    ZXArgs a;
    memset(&a, 0, sizeof(a));
    const u64 *at[GLP_GP_MAX_ORACLES] = {nullptr, nullptr, nullptr, nullptr}, *nx[GLP_GP_MAX_ORACLES] = {nullptr, nullptr, nullptr, nullptr};
    size_t st[GLP_GP_MAX_ORACLES] = {0, 0, 0, 0};
    for (u32 o = 0; o < p->noracles; o++) {
        GLP_TRY(ext_openings_input(tmp, openings + o, p->oracle_cols[o], p->next_mask >> o & 1 ? p->oracle_cols[o] : 0, K, inputs_on_device, &at[o], &nx[o],
                                   &st[o]));
    }
    a.at0 = at[0]; a.at1 = at[1]; a.at2 = at[2]; a.at3 = at[3];
    a.nx0 = nx[0]; a.nx1 = nx[1]; a.nx2 = nx[2]; a.nx3 = nx[3];
    a.st0 = st[0]; a.st1 = st[1]; a.st2 = st[2]; a.st3 = st[3];
    GLP_TRY(tmp.input(points, inputs_on_device, 2 * (size_t)K, &a.points));
    GLP_TRY(tmp.input(alphas, 0, (size_t)K * nch, &a.alphas));
    if (p->nparams) GLP_TRY(tmp.input(params, 0, (size_t)K * p->nparams, &a.params));
    const size_t words = 2 * (size_t)K * nch;
    u64 *dev_out = out;
    if (!out_on_device) GLP_TRY(tmp.words(&dev_out, words));
    a.code = p->dev; a.pool = p->dev + p->code_words; a.out = dev_out;
    a.K = K; a.ninstr = p->ninstr; a.nregs = p->nregs; a.nparams = p->nparams;
    {
        StageScope stg(c, "gate_program.eval_ext", 8.0 * K * (2.0 * p->cols_named + 2.0 * nch + 2));
        const dim3 grid((K + ZX_BLOCK - 1) / ZX_BLOCK);
        const size_t lds = (size_t)p->nregs * 2 * ZX_BLOCK * 8;      // at most 24 KB
        GLP_LAUNCH_NCH(k_gate_program_ext, nch, grid, dim3(ZX_BLOCK), lds, c->stream, a);
        GLP_HIP(hipGetLastError());
    }
    if (!out_on_device) GLP_TRY(d2h(c, out, dev_out, words * 8));
    return GLP_OK;
}

int glp_perm_check_zeta(glp_ctx *c, const glp_perm_desc *desc, uint32_t num_proofs, uint32_t num_quotient_chunks, const uint64_t *zetas,
                        const glp_ext_openings *sigmas, const glp_ext_openings *wires, const glp_ext_openings *zs, const glp_ext_openings *quotient,
                        int inputs_on_device, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas, const uint64_t *gate_sums,
                        int gate_sums_on_device, int32_t *status_out, char *reasons_out) {
    static const char *fn = "glp_perm_check_zeta";
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    PermShape s;
    GLP_TRY(perm_desc_check(fn, desc, s));
    GLP_REQUIRE(zetas, "%s: zetas is null", fn);
    GLP_REQUIRE(sigmas, "%s: sigmas is null", fn);
    GLP_REQUIRE(wires, "%s: wires is null", fn);
    GLP_REQUIRE(zs, "%s: zs is null", fn);
    GLP_REQUIRE(quotient, "%s: quotient is null", fn);
    GLP_REQUIRE(status_out, "%s: status_out is null", fn);
    const u32 K = num_proofs, nch = s.nch, chunks = num_quotient_chunks;
    GLP_TRY(seam_num_proofs_check(fn, K));
    GLP_REQUIRE(chunks >= 1 && chunks <= 256, "%s: num_quotient_chunks = %u outside 1..256", fn, chunks);
    GLP_TRY(ext_openings_check(fn, "sigmas", sigmas, s.nr, 0, K, inputs_on_device));
    GLP_TRY(ext_openings_check(fn, "wires", wires, s.nr, 0, K, inputs_on_device));
    GLP_TRY(ext_openings_check(fn, "zs", zs, s.nzp, nch, K, inputs_on_device));
    GLP_TRY(ext_openings_check(fn, "quotient", quotient, nch * chunks, 0, K, inputs_on_device));
    if (!inputs_on_device) GLP_TRY(ext_points_check(fn, "zetas", zetas, K, 2));
    GLP_TRY(perm_challenges_check(fn, "betas", betas, K, nch));
    GLP_TRY(perm_challenges_check(fn, "gammas", gammas, K, nch));
    GLP_TRY(perm_challenges_check(fn, "alphas", alphas, K, nch));
    if (gate_sums && !gate_sums_on_device) GLP_TRY(ext_points_check(fn, "gate_sums", gate_sums, K, 2 * nch));
    GLP_TRY(bind(c));
    Scratch tmp(c);
    ZPArgs a;
    memset(&a, 0, sizeof(a));
    const u64 *none;
    GLP_TRY(ext_openings_input(tmp, sigmas, s.nr, 0, K, inputs_on_device, &a.sg, &none, &a.sg_st));
    GLP_TRY(ext_openings_input(tmp, wires, s.nr, 0, K, inputs_on_device, &a.wl, &none, &a.wl_st));
    GLP_TRY(ext_openings_input(tmp, zs, s.nzp, nch, K, inputs_on_device, &a.zs, &a.zn, &a.zs_st));
    GLP_TRY(ext_openings_input(tmp, quotient, nch * chunks, 0, K, inputs_on_device, &a.qt, &none, &a.qt_st));
    GLP_TRY(tmp.input(zetas, inputs_on_device, 2 * (size_t)K, &a.zetas));
    if (gate_sums) GLP_TRY(tmp.input(gate_sums, gate_sums_on_device, 2 * (size_t)K * nch, &a.gate_sums));
    // one table: k_is [nr], then per proof betas[MAXCH], gammas[MAXCH], alphas[MAXCH]
    std::vector<u64> tab((size_t)s.nr + (size_t)K * 3 * MAXCH, 0);
    memcpy(tab.data(), desc->k_is, (size_t)s.nr * 8);
    for (u32 k = 0; k < K; k++)
        for (u32 i = 0; i < nch; i++) {
            u64 *tk = tab.data() + s.nr + (size_t)k * 3 * MAXCH;
            tk[i] = betas[(size_t)k * nch + i];
            tk[MAXCH + i] = gammas[(size_t)k * nch + i];
            tk[2 * MAXCH + i] = alphas[(size_t)k * nch + i];
        }
    u64 *dev_tab;
    GLP_TRY(tmp.words(&dev_tab, tab.size()));
    GLP_TRY(h2d(c, dev_tab, tab.data(), tab.size() * 8));
    GLP_TRY(tmp.array(&a.verdict, (size_t)K * nch));
    a.k_is = dev_tab; a.chal = dev_tab + s.nr;
    a.n_field = ((u64)1 << s.lg) % P;
    a.K = K; a.lg = s.lg; a.nr = s.nr; a.nch = nch; a.npp = s.npp; a.qdf = s.qdf; a.chunks = chunks;
    {
        StageScope stg(c, "perm.check_zeta", 16.0 * K * (2.0 * s.nr + s.nzp + nch + nch * chunks));
        hipLaunchKernelGGL(k_perm_check_zeta, dim3((K * nch + ZX_BLOCK - 1) / ZX_BLOCK), dim3(ZX_BLOCK), 0, c->stream, a);
        GLP_HIP(hipGetLastError());
    }
    std::vector<u32> verdict((size_t)K * nch);
    GLP_TRY(d2h(c, verdict.data(), a.verdict, verdict.size() * 4));
    for (u32 k = 0; k < K; k++) {
        char why[GLP_REASON_LEN] = "";
        for (u32 i = 0; i < nch && !why[0]; i++) {
            if (verdict[(size_t)k * nch + i] == 2) snprintf(why, sizeof(why), "zeta = 1");
            else if (verdict[(size_t)k * nch + i]) snprintf(why, sizeof(why), "Mismatch between evaluation and opening of quotient polynomial (challenge %u)", i);
        }
        status_out[k] = why[0] ? GLP_ERR_PROVE : GLP_OK;
        if (reasons_out) {
            memset(reasons_out + (size_t)k * GLP_REASON_LEN, 0, GLP_REASON_LEN);
            strncpy(reasons_out + (size_t)k * GLP_REASON_LEN, why, GLP_REASON_LEN - 1);
        }
    }
    return GLP_OK;
}

}  // extern "C"
