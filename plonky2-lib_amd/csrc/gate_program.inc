// gate_program.inc -- glp_gate_program_*: caller-defined gate constraints of a circuit whose quotient stays with the caller, evaluated
// on the quotient's coset (include/glp.h, "caller-defined gate constraints at the commitment seam").  Included by prover.hip beside
// perm_seam.inc; the result is the gate_sums array k_perm_quotient reads.
//
// k_gate_program is an interpreter: a straight-line program of 64-bit instructions (layout: GLP_GP_* in glp.h), the same for every
// point, run by every lane on its own point.  What is wave-uniform stays on the scalar side: the instruction words, the constant
// pool, the per-proof params and the alpha powers come through uniform pointers (scalar loads, four instruction words per load), the
// decode is scalar arithmetic and the dispatch is uniform branches.  What a lane owns:
//   registers     in LDS, regs[r][256] u64 with lane t at word r * 256 + t: consecutive lanes 8 bytes apart, so every ds_read_b64 /
//                 ds_write_b64 is conflict-free, and a lane only ever touches its own column -- no barrier inside the program.
//                 (Indexed by a run-time r, a VGPR array would live in scratch.)  num_regs * 2 KB, dynamic.
//   acc_c, total_c  two Acc160 per challenge: EMIT is one acc_fma against alpha_c^t, END folds acc_c, multiplies it by the filter into
//                 total_c and clears it.  Neither has a term bound in reach (2^32 terms).
// Lane mapping and output are k_perm_quotient's: a block owns 256 consecutive natural indices, lane t computes (plane t / QL, slot
// t % QL), QL = 256 >> sub_bits, and the results change places in a [plane][slot] tile of pitch QL + 1 behind one barrier.
// The fetch / decode / dispatch loop below exists three times -- here, in k_gate_program_ext (zeta_check.inc) and in
// k_gate_program_rows (trace_program.inc) -- and a change to the format belongs in all three: one walker over a machine type made
// k_gate_program slower (profiles/r22_seam_one_body.txt).
struct GPArgs {
    const u64 *code;                      // instruction words, zero-padded to a multiple of 4 (opcode 0 does nothing; the check refuses it)
    const u64 *pool;
    const u64 *tab;                       // [K][tab_stride]: the address of each oracle's LDE of this proof [GLP_GP_MAX_ORACLES] (coset-major
                                          // [columns][R][n]; a shared oracle's is the same for every proof), alpha powers [NCH][maxc], params
    u64 *out;
    u64 w_M;
    u32 lg, rb, sb, ninstr, nregs, maxc, tab_stride;
};
// One operand of one instruction: f is its 27 bits, wave-uniform, so the switch is a scalar branch and only the load itself is per lane.
// l0..l3: the addresses of the four oracles' LDEs of this proof, four scalars picked by scalar selects (an array indexed by o would be scratch).
__device__ __forceinline__ u64 gp_operand(u32 f, const u64 *regs, u64 l0, u64 l1, u64 l2, u64 l3, size_t N, size_t slot, size_t slot_next,
                                          const u64 *pool, const u64 *prm, u64 x) {
    const u32 kind = f & 7, pl = f >> 3;
    switch (kind) {
    case GLP_GP_REG: return regs[(size_t)pl * 256];
    case GLP_GP_COL: case GLP_GP_COL_NEXT: {
        const u32 o = pl >> GLP_GP_COL_ORACLE_SHIFT, col = pl & ((1u << GLP_GP_COL_ORACLE_SHIFT) - 1);
        typedef const __attribute__((address_space(1))) u64 *gptr;           // HBM, said so: an address made from a table word would be a flat load
        const gptr b = (gptr)(o == 0 ? l0 : o == 1 ? l1 : o == 2 ? l2 : l3);
        return b[(size_t)col * N + (kind == GLP_GP_COL ? slot : slot_next)];
    }
    case GLP_GP_IMM: return pool[pl];
    case GLP_GP_PARAM: return prm[pl];
    default: return x;
    }
}
extern __shared__ __attribute__((aligned(16))) u64 gp_lds[];      // regs [nregs][256], then the tile [NCH][PQ_TILE]
template <int NCH>
__global__ __launch_bounds__(256) void k_gate_program(GPArgs a) {
    const u32 t = threadIdx.x, S = 1u << a.sb, lgql = 8 - a.sb, QL = 1u << lgql, pitch = QL + 1;
    const size_t n = (size_t)1 << a.lg, N = n << a.rb, M = n << a.sb;
    const size_t k = blockIdx.y, i0 = (size_t)blockIdx.x * 256, q0 = i0 >> a.sb;
    u64 *regs = gp_lds + t, *tile = gp_lds + (size_t)a.nregs * 256;
    const u32 r = t >> lgql, ql = t & (QL - 1), own_pos = r * pitch + ql;
    const size_t q = q0 + ql;
    if (q < n) {
        const size_t plane = (size_t)r << (a.rb - a.sb);
        const size_t slot = plane * n + q, slot_next = plane * n + ((q + 1) & (n - 1));
        const u64 *tb = a.tab + k * a.tab_stride, *apow = tb + GLP_GP_MAX_ORACLES, *prm = apow + (size_t)NCH * a.maxc, *pool = a.pool;
        const u64 l0 = tb[0], l1 = tb[1], l2 = tb[2], l3 = tb[3];
        const u32 maxc = a.maxc;
        const u64 x = mul(GEN, dpow(a.w_M, (u64)(q * S + r)));     // g W_M^i, i = q S + r
        Acc160 acc[NCH], tot[NCH];
        _Pragma("unroll") for (int c = 0; c < NCH; c++) { acc_zero(acc[c]); acc_zero(tot[c]); }
        u32 tc = 0;                                                // EMITs since the last END
        for (u32 pc = 0; pc < a.ninstr; pc += 4) {
            const u64 w[4] = {a.code[pc], a.code[pc + 1], a.code[pc + 2], a.code[pc + 3]};      // one scalar load
            _Pragma("unroll") for (int j = 0; j < 4; j++) {
                const u64 ins = w[j];
                const u32 op = (u32)ins & 15;
                if (op == 0) continue;
                const u64 va = gp_operand((u32)(ins >> GLP_GP_A_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), regs, l0, l1, l2, l3, N, slot, slot_next, pool, prm, x);
                if (op <= GLP_GP_OP_MOV) {
                    u64 v = va;
                    if (op != GLP_GP_OP_MOV) {
                        const u64 vb = gp_operand((u32)(ins >> GLP_GP_B_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), regs, l0, l1, l2, l3, N, slot, slot_next, pool, prm, x);
                        v = op == GLP_GP_OP_ADD ? add(va, vb) : op == GLP_GP_OP_SUB ? sub(va, vb) : mul(va, vb);
                    }
                    regs[(size_t)(((u32)ins >> GLP_GP_DST_SHIFT) & 31) * 256] = v;
                } else if (op == GLP_GP_OP_EMIT) {
                    _Pragma("unroll") for (int c = 0; c < NCH; c++) acc_fma(acc[c], va, apow[(size_t)c * maxc + tc]);
                    tc++;
                } else {
                    _Pragma("unroll") for (int c = 0; c < NCH; c++) { acc_fma(tot[c], acc_reduce(acc[c]), va); acc_zero(acc[c]); }
                    tc = 0;
                }
            }
        }
        _Pragma("unroll") for (int c = 0; c < NCH; c++) tile[c * PQ_TILE + own_pos] = acc_reduce(tot[c]);
    }
    __syncthreads();
    // natural index i0 + t = (q0 + (t >> sb)) S + (t & (S - 1))
    if (i0 + t < M) {
        const u32 nat_pos = (t & (S - 1)) * pitch + (t >> a.sb);
        _Pragma("unroll") for (int c = 0; c < NCH; c++) a.out[(k * NCH + c) * M + i0 + t] = tile[c * PQ_TILE + nat_pos];
    }
}

struct glp_gate_program {
    glp_ctx *ctx = nullptr;
    u64 *dev = nullptr;            // code, zero-padded to a multiple of 4 words, then the pool
    u32 ninstr = 0, code_words = 0, npool = 0, nregs = 0, nparams = 0, noracles = 0;
    u32 oracle_cols[GLP_GP_MAX_ORACLES] = {0, 0, 0, 0};
    u32 maxc = 0;                  // the largest number of EMITs in one gate
    u32 cols_named = 0;            // distinct (oracle, polynomial) pairs the program reads: the stage record's bytes
    u32 next_mask = 0;             // bit o: the program reads a COL_NEXT of oracle o (zeta_check.inc asks for at_next only then)
    // the shape trace_program.inc asks for (one gate closed by END IMM(1)): the number of ENDs, the index of the first one, and the
    // last END's operand kind and, for an IMM, its pool word
    u32 num_ends = 0, first_end = 0, end_kind = 0;
    u64 end_word = 0;
};

namespace {
// the rules of glp_gate_program_check are gate_program_check (circuit_common.h: host only, shared with the circuit description's checks)
// what the three evaluators (glp_gate_program_sums, _eval_ext, _rows) ask of the handle, and of the params that go with it
int gate_program_handle_check(const char *fn, const glp_ctx *c, const glp_gate_program *p) {
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    GLP_REQUIRE(p, "%s: program is null", fn);
    GLP_REQUIRE(p->ctx == c, "%s: program belongs to another ctx", fn);
    return GLP_OK;
}
int gate_program_params_check(const char *fn, const glp_gate_program *p, const u64 *params, u32 K) {
    GLP_REQUIRE(params || p->nparams == 0, "%s: params is null, the program has num_params = %u", fn, p->nparams);
    if (p->nparams) GLP_TRY(perm_challenges_check(fn, "params", params, K, p->nparams));
    return GLP_OK;
}
}  // namespace

extern "C" {

int glp_gate_program_check(const glp_gate_program_desc *d, uint32_t *max_constraints_out) {
    static const char *fn = "glp_gate_program_check";
    GLP_REQUIRE(max_constraints_out, "%s: max_constraints_out is null", fn);
    *max_constraints_out = 0;
    GPInfo info;
    GLP_TRY(gate_program_check(fn, d, info));
    *max_constraints_out = info.maxc;
    return GLP_OK;
}

int glp_gate_program_create(glp_ctx *c, const glp_gate_program_desc *d, glp_gate_program **out) {
    static const char *fn = "glp_gate_program_create";
    GLP_REQUIRE(out, "%s: out is null", fn);
    *out = nullptr;
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    GPInfo info;
    GLP_TRY(gate_program_check(fn, d, info));
    GLP_TRY(bind(c));
    std::unique_ptr<glp_gate_program, void (*)(glp_gate_program *)> p(new glp_gate_program(), glp_gate_program_free);
    p->ctx = c;
    p->ninstr = d->num_instructions; p->code_words = (d->num_instructions + 3) & ~3u; p->npool = d->num_pool;
    p->nregs = d->num_regs; p->nparams = d->num_params; p->noracles = d->num_oracles;
    for (u32 o = 0; o < d->num_oracles; o++) p->oracle_cols[o] = d->oracle_cols[o];
    p->maxc = info.maxc; p->cols_named = info.cols_named; p->next_mask = info.next_mask;
    for (u32 i = 0; i < d->num_instructions; i++)
        if (((u32)d->code[i] & 15) == GLP_GP_OP_END && ++p->num_ends == 1) p->first_end = i;
    const u32 end_a = (u32)(d->code[d->num_instructions - 1] >> GLP_GP_A_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1);
    p->end_kind = end_a & 7;
    if (p->end_kind == GLP_GP_IMM) p->end_word = d->pool[end_a >> 3];
    std::vector<u64> img((size_t)p->code_words + p->npool, 0);
    memcpy(img.data(), d->code, (size_t)p->ninstr * 8);
    if (p->npool) memcpy(img.data() + p->code_words, d->pool, (size_t)p->npool * 8);
    void *dv = nullptr;
    GLP_TRY(c->alloc(&dv, img.size() * 8));
    p->dev = (u64 *)dv;
    GLP_TRY(h2d(c, p->dev, img.data(), img.size() * 8));
    *out = p.release();
    return GLP_OK;
}

void glp_gate_program_free(glp_gate_program *p) {
    if (!p) return;
    if (p->dev) {
        (void)hipSetDevice(p->ctx->device);
        (void)hipStreamSynchronize(p->ctx->stream);
        p->ctx->release(p->dev);
    }
    delete p;
}

int glp_gate_program_sums(glp_ctx *c, const glp_gate_program *p, uint32_t num_proofs, const glp_batch *const *oracles, uint32_t sub_bits,
                          uint32_t num_challenges, const uint64_t *alphas, const uint64_t *params, uint64_t *out, int out_on_device) {
    static const char *fn = "glp_gate_program_sums";
    GLP_TRY(gate_program_handle_check(fn, c, p));
    GLP_REQUIRE(oracles, "%s: oracles is null", fn);
    GLP_REQUIRE(out, "%s: out is null", fn);
    const u32 K = num_proofs, nch = num_challenges;
    GLP_TRY(seam_num_proofs_check(fn, K));
    GLP_REQUIRE(nch >= 1 && nch <= (u32)MAXCH, "%s: num_challenges = %u outside 1..%d", fn, nch, MAXCH);
    for (u32 o = 0; o < p->noracles; o++) {
        const glp_batch *b = oracles[o];
        GLP_REQUIRE(b, "%s: oracles[%u] is null", fn, o);
        GLP_REQUIRE(b->ctx == c, "%s: oracles[%u] belongs to another ctx", fn, o);
        GLP_REQUIRE(b->lg == oracles[0]->lg, "%s: log_n disagrees: oracles[0] %d, oracles[%u] %d", fn, oracles[0]->lg, o, b->lg);
        GLP_REQUIRE(b->rate_bits == oracles[0]->rate_bits, "%s: rate_bits disagrees: oracles[0] %d, oracles[%u] %d", fn, oracles[0]->rate_bits, o, b->rate_bits);
        GLP_REQUIRE(b->ncols >= p->oracle_cols[o], "%s: oracles[%u] has %u polynomials, the program's oracle_cols[%u] is %u (salts are not polynomials)", fn, o,
                    b->ncols, o, p->oracle_cols[o]);
        GLP_REQUIRE(b->K == K || b->K == 1, "%s: oracles[%u] has %u members, neither 1 nor num_proofs = %u", fn, o, b->K, K);
    }
    const u32 lg = (u32)oracles[0]->lg, rb = (u32)oracles[0]->rate_bits;
    GLP_REQUIRE(sub_bits <= rb, "%s: sub_bits = %u is more than rate_bits = %u", fn, sub_bits, rb);
    GLP_TRY(perm_challenges_check(fn, "alphas", alphas, K, nch));
    GLP_TRY(gate_program_params_check(fn, p, params, K));
    GLP_TRY(bind(c));
    const size_t n = (size_t)1 << lg, N = n << rb, M = n << sub_bits, words = (size_t)K * nch * M;
    Scratch tmp(c);
    // one table per proof: where its member of each oracle starts (salt planes stepped over), alpha powers [nch][maxc], its params
    const u32 tab_stride = GLP_GP_MAX_ORACLES + nch * p->maxc + p->nparams;
    std::vector<u64> tab((size_t)K * tab_stride, 0);
    for (u32 k = 0; k < K; k++) {
        u64 *tk = tab.data() + (size_t)k * tab_stride;
        for (u32 o = 0; o < p->noracles; o++) {
            const glp_batch *b = oracles[o];
            tk[o] = (u64)(uintptr_t)(b->lde + (b->K == 1 ? 0 : (size_t)k * (b->ncols + b->salt) * N));
        }
        tk += GLP_GP_MAX_ORACLES;
        for (u32 i = 0; i < nch; i++) alpha_powers(alphas[(size_t)k * nch + i], p->maxc, tk + (size_t)i * p->maxc);
        if (p->nparams) memcpy(tk + (size_t)nch * p->maxc, params + (size_t)k * p->nparams, (size_t)p->nparams * 8);
    }
    u64 *dev_tab;
    GLP_TRY(tmp.words(&dev_tab, tab.size()));
    GLP_TRY(h2d(c, dev_tab, tab.data(), tab.size() * 8));
    u64 *dev_out = out;
    if (!out_on_device) GLP_TRY(tmp.words(&dev_out, words));

    GPArgs a;
    memset(&a, 0, sizeof(a));
    a.code = p->dev; a.pool = p->dev + p->code_words; a.tab = dev_tab; a.out = dev_out;
    a.w_M = root_of_unity((int)(lg + sub_bits));
    a.lg = lg; a.rb = rb; a.sb = sub_bits; a.ninstr = p->ninstr; a.nregs = p->nregs; a.maxc = p->maxc; a.tab_stride = tab_stride;
    {
        StageScope st(c, "gate_program.sums", 8.0 * M * K * ((double)p->cols_named + nch));
        const dim3 grid(nblk(M), K);
        const size_t lds = ((size_t)p->nregs * 256 + (size_t)nch * PQ_TILE) * 8;      // at most 24 * 2 KB + 4 * 2112 B < 64 KB
        GLP_LAUNCH_NCH(k_gate_program, nch, grid, dim3(256), lds, c->stream, a);
        GLP_HIP(hipGetLastError());
    }
    if (!out_on_device) GLP_TRY(d2h(c, out, dev_out, words * 8));
    return GLP_OK;
}

}  // extern "C"
