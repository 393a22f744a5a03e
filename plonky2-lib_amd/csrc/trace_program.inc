// trace_program.inc -- glp_gate_program_rows: a gate program read a third way, on the rows of H (include/glp.h, "caller-defined
// running arguments at the commitment seam").  Included by prover.hip behind zeta_check.inc; it reads gate_program.inc's program
// object, operand decoder and LDS symbol.
//
// The first two readings fold what the program EMITs (with alpha powers on the quotient's coset, over F_p^2 at zeta).  This one keeps
// it: EMIT number t of the program is column t of the output, so a caller states the numerators and denominators of its own lookup,
// logUp or grand-product argument as a program over its witness columns and a challenge, and glp_running_columns turns them into
// helper columns and the running column without the witness leaving HBM.
//
// k_gate_program_rows keeps k_gate_program's design: one lane per row, instruction words, pool and params through uniform pointers
// (scalar loads, four instruction words per load) with a scalar decode, registers in LDS as regs[r][256].  gp_operand serves as it
// stands with N = n, slot = i, slot_next = (i + 1) mod n.  There are no accumulators, no alpha table and no tile exchange: EMIT is
// one coalesced 8-byte store per lane, END does nothing (the check below admits one gate, closed by END IMM(1)), and a lane past the
// last row leaves at once since nothing below is a barrier.  A column word is reduced mod p once as it is loaded, the convention of
// glp_gate_program_eval_ext for inputs that never passed a host scan.
struct GPRowsArgs {
    const u64 *code;                      // instruction words, zero-padded to a multiple of 4
    const u64 *pool;
    const u64 *tab;                       // [K][tab_stride]: the address of each input of this proof [GLP_GP_MAX_ORACLES] ([columns][n]; a shared
                                          // input's is the same for every proof), then its params
    u64 *out;                             // [K][nout][n]
    u64 w_n;
    u32 lg, ninstr, nout, tab_stride;
};
__device__ __forceinline__ u64 gpr_operand(u32 f, const u64 *regs, u64 l0, u64 l1, u64 l2, u64 l3, size_t n, size_t i, size_t i_next, const u64 *pool,
                                           const u64 *prm, u64 x) {
    const u64 v = gp_operand(f, regs, l0, l1, l2, l3, n, i, i_next, pool, prm, x);
    const u32 kind = f & 7;               // wave-uniform
    return kind == GLP_GP_COL || kind == GLP_GP_COL_NEXT ? canon(v) : v;
}
__global__ __launch_bounds__(256) void k_gate_program_rows(GPRowsArgs a) {
    const u32 t = threadIdx.x;
    const size_t n = (size_t)1 << a.lg, k = blockIdx.y, i = (size_t)blockIdx.x * 256 + t;
    if (i >= n) return;                                            // no barrier below
    const size_t i_next = (i + 1) & (n - 1);
    u64 *regs = gp_lds + t;
    const u64 *tb = a.tab + k * a.tab_stride, *prm = tb + GLP_GP_MAX_ORACLES, *pool = a.pool;
    const u64 l0 = tb[0], l1 = tb[1], l2 = tb[2], l3 = tb[3];
    const u64 x = dpow(a.w_n, (u64)i);                             // w_n^i
    u64 *o = a.out + k * a.nout * n + i;                           // the next EMIT's word of this row
    for (u32 pc = 0; pc < a.ninstr; pc += 4) {
        const u64 w[4] = {a.code[pc], a.code[pc + 1], a.code[pc + 2], a.code[pc + 3]};      // one scalar load
        _Pragma("unroll") for (int j = 0; j < 4; j++) {
            const u64 ins = w[j];
            const u32 op = (u32)ins & 15;
            if (op == 0 || op == GLP_GP_OP_END) continue;
            const u64 va = gpr_operand((u32)(ins >> GLP_GP_A_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), regs, l0, l1, l2, l3, n, i, i_next, pool, prm, x);
            if (op <= GLP_GP_OP_MOV) {
                u64 v = va;
                if (op != GLP_GP_OP_MOV) {
                    const u64 vb = gpr_operand((u32)(ins >> GLP_GP_B_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), regs, l0, l1, l2, l3, n, i, i_next, pool, prm, x);
                    v = op == GLP_GP_OP_ADD ? add(va, vb) : op == GLP_GP_OP_SUB ? sub(va, vb) : mul(va, vb);
                }
                regs[(size_t)(((u32)ins >> GLP_GP_DST_SHIFT) & 31) * 256] = v;
            } else {                                               // EMIT
                *o = va;
                o += n;
            }
        }
    }
}

namespace {
// [count] host words of one named array, canonical or refused naming the array and the word
int rows_words_check(const char *fn, const char *name, u32 index, const u64 *v, size_t count) {
    const size_t bad = first_noncanonical(v, count);
    GLP_REQUIRE(bad == count, "%s: %s[%u]: word %zu = 0x%016llx is not a canonical field element (>= p)", fn, name, index, bad,
                (unsigned long long)v[bad == count ? 0 : bad]);
    return GLP_OK;
}
}  // namespace

extern "C" {

int glp_gate_program_rows(glp_ctx *c, const glp_gate_program *p, uint32_t num_proofs, uint32_t log_n, const uint64_t *const *inputs,
                          const uint32_t *input_members, int inputs_on_device, const uint64_t *params, uint64_t *out, int out_on_device) {
    static const char *fn = "glp_gate_program_rows";
    GLP_TRY(gate_program_handle_check(fn, c, p));
    GLP_REQUIRE(inputs, "%s: inputs is null", fn);
    GLP_REQUIRE(input_members, "%s: input_members is null", fn);
    GLP_REQUIRE(out, "%s: out is null", fn);
    const u32 K = num_proofs, lg = log_n;
    GLP_TRY(seam_num_proofs_check(fn, K));
    GLP_REQUIRE(lg <= (u32)NTT_MAX_LG, "%s: log_n = %u is more than %d", fn, lg, NTT_MAX_LG);
    // the shape: one gate, closed by END IMM(1) (p->end_* were taken down when the program was made)
    GLP_REQUIRE(p->num_ends == 1, "%s: instruction %u, field op: END before the last instruction (the program has %u); a program on the rows of H is a single gate",
                fn, p->first_end, p->num_ends);
    GLP_REQUIRE(p->end_kind == GLP_GP_IMM, "%s: instruction %u, field a: the END of a program on the rows of H takes IMM(1), not an operand of kind %u", fn,
                p->ninstr - 1, p->end_kind);
    GLP_REQUIRE(p->end_word == 1, "%s: instruction %u, field a: the END of a program on the rows of H takes IMM(1), its pool word is 0x%016llx", fn,
                p->ninstr - 1, (unsigned long long)p->end_word);
    GLP_REQUIRE(p->maxc >= 1, "%s: instruction %u, field op: END closes a program without an EMIT: no column to write", fn, p->ninstr - 1);
    const size_t n = (size_t)1 << lg;
    size_t in_cols = 0;
    for (u32 o = 0; o < p->noracles; o++) {
        GLP_REQUIRE(inputs[o], "%s: inputs[%u] is null", fn, o);
        GLP_REQUIRE(input_members[o] == 1 || input_members[o] == K, "%s: input_members[%u] = %u is neither 1 nor num_proofs = %u", fn, o, input_members[o], K);
        in_cols += (size_t)input_members[o] * p->oracle_cols[o];
    }
    GLP_REQUIRE((size_t)K * p->maxc <= BATCH_MAX_BYTES / (8 * n), "%s: out too large (num_proofs * num_out * 2^log_n words)", fn);
    GLP_REQUIRE(in_cols <= BATCH_MAX_BYTES / (8 * n), "%s: inputs too large (members * columns * 2^log_n words)", fn);
    GLP_TRY(gate_program_params_check(fn, p, params, K));
    if (!inputs_on_device)
        for (u32 o = 0; o < p->noracles; o++) GLP_TRY(rows_words_check(fn, "inputs", o, inputs[o], (size_t)input_members[o] * p->oracle_cols[o] * n));
    GLP_TRY(bind(c));
    Scratch tmp(c);
    const u64 *dev_in[GLP_GP_MAX_ORACLES] = {nullptr, nullptr, nullptr, nullptr};
    for (u32 o = 0; o < p->noracles; o++) GLP_TRY(tmp.input(inputs[o], inputs_on_device, (size_t)input_members[o] * p->oracle_cols[o] * n, &dev_in[o]));
    // one table per proof: where its member of each input starts, then its params
    const u32 tab_stride = GLP_GP_MAX_ORACLES + p->nparams;
    std::vector<u64> tab((size_t)K * tab_stride, 0);
    for (u32 k = 0; k < K; k++) {
        u64 *tk = tab.data() + (size_t)k * tab_stride;
        for (u32 o = 0; o < p->noracles; o++) tk[o] = (u64)(uintptr_t)(dev_in[o] + (input_members[o] == 1 ? 0 : (size_t)k * p->oracle_cols[o] * n));
        if (p->nparams) memcpy(tk + GLP_GP_MAX_ORACLES, params + (size_t)k * p->nparams, (size_t)p->nparams * 8);
    }
    u64 *dev_tab;
    GLP_TRY(tmp.words(&dev_tab, tab.size()));
    GLP_TRY(h2d(c, dev_tab, tab.data(), tab.size() * 8));
    const size_t words = (size_t)K * p->maxc * n;
    u64 *dev_out = out;
    if (!out_on_device) GLP_TRY(tmp.words(&dev_out, words));

    GPRowsArgs a;
    memset(&a, 0, sizeof(a));
    a.code = p->dev; a.pool = p->dev + p->code_words; a.tab = dev_tab; a.out = dev_out;
    a.w_n = root_of_unity((int)lg);
    a.lg = lg; a.ninstr = p->ninstr; a.nout = p->maxc; a.tab_stride = tab_stride;
    {
        StageScope st(c, "gate_program.rows", 8.0 * n * K * ((double)p->cols_named + p->maxc));
        hipLaunchKernelGGL(k_gate_program_rows, dim3(nblk(n), K), dim3(256), (size_t)p->nregs * 256 * 8, c->stream, a);      // at most 48 KB of LDS
        GLP_HIP(hipGetLastError());
    }
    if (!out_on_device) GLP_TRY(d2h(c, out, dev_out, words * 8));
    return GLP_OK;
}

}  // extern "C"
