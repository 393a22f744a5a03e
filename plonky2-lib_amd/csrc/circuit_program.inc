// circuit_program.inc -- GLP_GATE_PROGRAM: a gate of a glp_circuit whose constraints are a gate program (include/glp.h, "GATE PROGRAMS IN A
// CIRCUIT").  Included by prover.hip last of the seam files: it needs the quotient's arguments (quotient_kernels.inc), the program
// checker (gate_program.inc) and the witness checker's sink (witness_check.inc).  What is here:
//   cp_run                    the fifth fetch / decode / dispatch loop over the instruction word (the other four: gate_program.inc,
//                             zeta_check.inc, trace_program.inc, witness_program.inc -- a change to the format belongs in all): one gate
//                             at one point, constants and wires through two base pointers, EMIT k handed to a sink
//   k_quotient_gate_program   the quotient's reading, in the lane map of k_quotient_gate: one lane per slot q of evaluated plane rq,
//                             blockIdx.z = proof, coset-major loads coalesced along q; out += zh_inv filter sum_k v_k alpha_c^(k0 + k)
//   k_witness_check_program   the reading on the rows of H, k_witness_check_gate's frame around the same loop and WcSink
//   circuit_program_check     the in-circuit rules and the degree walk, for glp_gate_program_circuit_check and glp_circuit_create_prog
// The design is k_gate_program's (DESIGN.md section 7): instruction words, pool and alpha powers through uniform pointers (scalar loads,
// four words per load), scalar decode, uniform branches, and the register file in LDS as regs[r][256] with lane t at word r * 256 + t --
// conflict-free ds_read_b64 / ds_write_b64, a lane touches its own column only, so there is no barrier inside the program.
// The verifier's reading (F_p^2 at zeta, on the host) is program_constraints in verify_host.h.
struct CPArgs {
    const u64 *code;                  // instruction words, zero-padded to a multiple of 4 (opcode 0 does nothing; the check refuses it)
    const u64 *pool;
    u32 ninstr, nregs, gi;            // gi: the gate's index in the gate table (its selector data make the filter)
};
// One operand: f is its 27 bits, wave-uniform, so the switch is a scalar branch and only the load is per lane.  C0 / W: constant
// polynomial c and wire j of this lane's point at C0[c * N] and W[j * N].  The public-input hash comes as four scalars (an array
// indexed by the payload would live in scratch).
__device__ __forceinline__ u64 cp_operand(u32 f, const u64 *regs, const u64 *C0, const u64 *W, size_t N, const u64 *pool, u64 h0, u64 h1, u64 h2,
                                          u64 h3) {
    const u32 kind = f & 7, pl = f >> 3;
    switch (kind) {
    case GLP_GP_REG: return regs[(size_t)pl * 256];
    case GLP_GP_COL: {
        const u32 col = pl & ((1u << GLP_GP_COL_ORACLE_SHIFT) - 1);
        return (pl >> GLP_GP_COL_ORACLE_SHIFT ? W : C0)[(size_t)col * N];
    }
    case GLP_GP_IMM: return pool[pl];
    default: return pl == 0 ? h0 : pl == 1 ? h1 : pl == 2 ? h2 : h3;       // GLP_GP_PARAM (COL_NEXT and X never pass the check)
    }
}
// SINK: a type with emit(k, v), handed constraint k's canonical value (the quotient's accumulators below, or WcSink)
template <class SINK>
__device__ __forceinline__ void cp_run(const CPArgs &g, u64 *regs, const u64 *C0, const u64 *W, size_t N, u64 h0, u64 h1, u64 h2, u64 h3, SINK &sink) {
    const u64 *pool = g.pool;
    u32 tc = 0;                                                    // EMITs so far
    for (u32 pc = 0; pc < g.ninstr; pc += 4) {
        const u64 w[4] = {g.code[pc], g.code[pc + 1], g.code[pc + 2], g.code[pc + 3]};      // one scalar load
        _Pragma("unroll") for (int j = 0; j < 4; j++) {
            const u64 ins = w[j];
            const u32 op = (u32)ins & 15;
            if (op == 0 || op == GLP_GP_OP_END) continue;          // END IMM(1): the filter is the library's, applied by the caller
            const u64 va = cp_operand((u32)(ins >> GLP_GP_A_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), regs, C0, W, N, pool, h0, h1, h2, h3);
            if (op <= GLP_GP_OP_MOV) {
                u64 v = va;
                if (op != GLP_GP_OP_MOV) {
                    const u64 vb = cp_operand((u32)(ins >> GLP_GP_B_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), regs, C0, W, N, pool, h0, h1, h2, h3);
                    v = op == GLP_GP_OP_ADD ? add(va, vb) : op == GLP_GP_OP_SUB ? sub(va, vb) : mul(va, vb);
                }
                regs[(size_t)(((u32)ins >> GLP_GP_DST_SHIFT) & 31) * 256] = v;
            } else {
                sink.emit(tc, va);
                tc++;
            }
        }
    }
}
extern __shared__ __attribute__((aligned(16))) u64 cp_lds[];        // regs [nregs][256]
// EMIT k: acc_c += v alpha_c^(k0 + k), the circuit's own powers (p.apow, whole words).  Acc160 has no term bound in reach (2^32 terms).
template <int NCH>
struct CpQuotientSink {
    Acc160 acc[NCH];
    const u64 *ap;                    // p.apow + k0
    u32 nt;
    __device__ __forceinline__ void emit(u32 k, u64 v) {
        _Pragma("unroll") for (int c = 0; c < NCH; c++) acc_fma(acc[c], v, ap[(size_t)c * nt + k]);
    }
};
template <int NCH>
__global__ __launch_bounds__(256) void k_quotient_gate_program(QArgs a, QProof p0, QBatch qb, CPArgs g) {
    const QProof p = q_proof(p0, qb);
    const size_t n = (size_t)1 << a.lg, N = n << a.rb;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;                                            // no barrier below
    const u32 rq = blockIdx.y, r = rq * a.step;
    const size_t slot = (size_t)r * n + q;
    CpQuotientSink<NCH> sink;
    _Pragma("unroll") for (int c = 0; c < NCH; c++) acc_zero(sink.acc[c]);
    sink.ap = p.apow + ((u32)NCH + (u32)NCH * (a.npp + 1));
    sink.nt = a.nterms;
    cp_run(g, cp_lds + threadIdx.x, a.cs + slot, p.wl + slot, N, p.pih[0], p.pih[1], p.pih[2], p.pih[3], sink);
    const u64 filter = gate_filter(a, a.gates[g.gi], N, slot);
    const size_t Rq = (size_t)gridDim.y;
    _Pragma("unroll") for (int c = 0; c < NCH; c++) {
        u64 *o = p.out + ((size_t)c * Rq + rq) * n + q;
        *o = add(*o, mul(mul(filter, acc_reduce(sink.acc[c])), a.zh_inv[rq]));
    }
}
// k_witness_check_gate (witness_check.inc) around the program: N = n, slot = row, the constants on H
__global__ __launch_bounds__(256) void k_witness_check_program(WcArgs w, CPArgs g) {
    const size_t n = (size_t)1 << w.lg, k = blockIdx.y;
    unsigned long long *res = w.res + k * w.res_stride;
    size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    WcSink sink;
    bool mine = row < n;
    if (w.fetch) {                                       // one wave per proof; lane 0 owns the row of the first failure
        const unsigned long long key = res[WC_KEY];
        mine = threadIdx.x == 0 && key != ~0ull;
        row = mine ? (size_t)(key >> 32) : 0;
        sink.want = (u32)key;
    }
    mine = mine && wc_row_gate(w, n, row) == g.gi;
    if (mine) {
        const u64 *pih = w.pih + k * 4;
        cp_run(g, cp_lds + threadIdx.x, w.consts + row, w.wires + k * (size_t)w.nw * n + row, n, pih[0], pih[1], pih[2], pih[3], sink);
    }
    if (w.fetch) {
        if (mine) { res[WC_VALUE] = sink.val; res[WC_GATE] = g.gi; }
        return;
    }
    u64 cnt = sink.nfail;
    u32 rows = sink.nfail ? 1 : 0;
    unsigned long long key = sink.nfail ? ((unsigned long long)row << 32 | sink.kmin) : ~0ull;
    wc_block_reduce(cnt, rows, key);
    if (threadIdx.x == 0 && rows) {
        atomicAdd(res + WC_CONSTRAINTS, (unsigned long long)cnt);
        atomicAdd(res + WC_ROWS, (unsigned long long)rows);
        atomicAdd(res + WC_BY_GATE + g.gi, (unsigned long long)rows);
        atomicMin(res + WC_KEY, key);
    }
}

namespace {
// (the in-circuit rules on top of glp_gate_program_check's are circuit_program_check, circuit_common.h)
CPArgs circuit_program_args(const glp_circuit *cc, u32 gi) {
    const glp_circuit::Program &pr = cc->programs[cc->gates[gi].p0];
    const u32 words = ((u32)pr.code.size() + 3) & ~3u;
    CPArgs g;
    g.code = cc->dev_programs + cc->dev_at[cc->gates[gi].p0]; g.pool = g.code + words;
    g.ninstr = (u32)pr.code.size(); g.nregs = pr.nregs; g.gi = gi;
    return g;
}
// after the launches of the built-in gates: one launch per program gate, for every challenge count
int quotient_program_launches(glp_ctx *c, const glp_circuit *cc, u32 nch, dim3 grid, const QArgs &a, const QProof &qp, const QBatch &qbt) {
    for (u32 gi : cc->program_gates) {
        const CPArgs g = circuit_program_args(cc, gi);
        const size_t lds = (size_t)g.nregs * 256 * 8;              // at most 24 * 2 KB
        GLP_LAUNCH_NCH(k_quotient_gate_program, nch, grid, dim3(256), lds, c->stream, a, qp, qbt, g);
        GLP_HIP(hipGetLastError());
    }
    return GLP_OK;
}
int wc_launch_program(glp_ctx *c, const glp_circuit *cc, const WcArgs &w, u32 gi, u32 K) {
    const CPArgs g = circuit_program_args(cc, gi);
    const size_t n = (size_t)1 << w.lg, lds = (size_t)g.nregs * 256 * 8;
    if (w.fetch) hipLaunchKernelGGL(k_witness_check_program, dim3(1, K), dim3(64), lds, c->stream, w, g);
    else hipLaunchKernelGGL(k_witness_check_program, dim3(nblk(n), K), dim3(256), lds, c->stream, w, g);
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}
}  // namespace

extern "C" int glp_gate_program_circuit_check(const glp_gate_program_desc *d, uint32_t *num_constraints_out, uint32_t *degree_out,
                                              uint32_t *wires_used_out, uint32_t *consts_used_out) {
    CPInfo info;
    const int rc = circuit_program_check("glp_gate_program_circuit_check", d, info);
    if (rc != GLP_OK) info = CPInfo();
    if (num_constraints_out) *num_constraints_out = info.emits;
    if (degree_out) *degree_out = info.degree;
    if (wires_used_out) *wires_used_out = info.wires;
    if (consts_used_out) *consts_used_out = info.consts;
    return rc;
}
