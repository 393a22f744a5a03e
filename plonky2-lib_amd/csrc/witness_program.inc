// witness_program.inc -- caller-defined generators as unit programs (include/glp.h, "witness generation, the dataflow half", UNIT
// PROGRAMS): the host check of a program and the kernel that runs a wave's program units.  Included by witness.hip between the wave
// kernels and the planner's driver; the planner (witness_plan.h, which also holds the chunk and program-table records WProgChunk and
// WProgEntry) files program units as free units of kind GLP_WGEN_PROGRAM.
//
// k_witness_programs is the fourth walker of the gate-program instruction word (after k_gate_program, k_gate_program_ext and
// k_gate_program_rows) and follows the first: one 64-lane workgroup runs one chunk -- up to 64 units of ONE program, blockIdx.y = proof
// -- so the instruction stream is wave-uniform.  The chunk record, the program table, the instruction words (four per load) and the pool
// come through uniform pointers (scalar loads), the decode is scalar arithmetic, the dispatch uniform branches.  What a lane owns: its
// unit's cell run (read through the plan's 32-bit copy of cells[], as witness_free_unit does) and its column of the register file in
// LDS, regs[r][64] u64 with lane t at word r * 64 + t: consecutive lanes 8 bytes apart, conflict-free, no barrier.
// Every index was range-checked on the host: registers, pool words and input numbers by witness_program_check, cells by the planner,
// the number of EMITs against the unit's output cells by both.  A value read from a witness is an operand, never an address or a count.
namespace {
struct WProgArgs {
    u64 *wires;                  // proof 0
    const u64 *image;            // every program's code, then its pool
    const WProgEntry *progs;
    const WProgChunk *chunks;    // by wave
    const WFree *units;          // by wave, sorted by program; cell_begin points into cells
    const u32 *cells;
    u32 nw, lg;
};

// Address spaces, said so.  The plan's lists and the programs were written by the host before the launch and nothing in it writes them:
// read as constant memory, a load at a wave-uniform address is a scalar load even though the kernel stores to the witness between two
// of them.  The register file is LDS and the witness HBM: typed, the three sources of an operand stay three loads under a uniform
// branch (as plain pointers the compiler merged them into one flat load behind a select of addresses).
typedef const __attribute__((address_space(4))) u64 *wp_c64;
typedef const __attribute__((address_space(4))) u32 *wp_c32;
typedef __attribute__((address_space(3))) u64 *wp_lds64;
typedef __attribute__((address_space(1))) u64 *wp_g64;
typedef const __attribute__((address_space(1))) u32 *wp_g32;
__device__ __forceinline__ u64 wp_operand(u32 f, wp_lds64 regs, wp_g64 W, wp_g32 in, wp_c64 pool) {
    const u32 kind = f & 7, pl = f >> 3;
    switch (kind) {
    case GLP_GP_REG: return regs[pl * 64];
    case GLP_GP_COL: return W[in[pl]];
    default: return pool[pl];                          // GLP_GP_IMM: the check admits nothing else
    }
}
extern __shared__ __attribute__((aligned(16))) u64 wp_lds[];      // regs [max num_regs of the plan][64]
__global__ __launch_bounds__(64) void k_witness_programs(WProgArgs a, u32 chunk0) {
    const wp_c32 chp = (wp_c32)(uintptr_t)(a.chunks + chunk0 + blockIdx.x);
    const u32 prog = chp[0], first = chp[1], count = chp[2];
    const u32 t = threadIdx.x;
    if (t >= count) return;
    const wp_c32 pe = (wp_c32)(uintptr_t)(a.progs + prog);      // code_off, code_words, pool_off, num_inputs
    const u32 code_words = pe[1], num_inputs = pe[3];
    const wp_c64 code = (wp_c64)(uintptr_t)(a.image + pe[0]), pool = (wp_c64)(uintptr_t)(a.image + pe[2]);
    const size_t n = (size_t)1 << a.lg;
    const wp_g64 W = (wp_g64)(uintptr_t)(a.wires + (size_t)blockIdx.y * a.nw * n);
    const wp_g32 in = (wp_g32)(uintptr_t)(a.cells + a.units[first + t].cell_begin), out = in + num_inputs;
    const wp_lds64 regs = (wp_lds64)wp_lds + t;
    constexpr u32 FIELD = (1u << GLP_GP_OPERAND_BITS) - 1;
    u32 emitted = 0;
    for (u32 pc = 0; pc < code_words; pc += 4) {
        const u64 w[4] = {code[pc], code[pc + 1], code[pc + 2], code[pc + 3]};      // one scalar load
        _Pragma("unroll") for (int j = 0; j < 4; j++) {
            const u64 ins = w[j];
            const u32 op = (u32)ins & 15;
            if (op == 0 || op == GLP_GP_OP_END) continue;
            const u32 fb = (u32)(ins >> GLP_GP_B_SHIFT) & FIELD;
            const u64 va = wp_operand((u32)(ins >> GLP_GP_A_SHIFT) & FIELD, regs, W, in, pool);
            if (op == GLP_GP_OP_EMIT) {
                const u32 c = out[emitted++];
                if (c != NONE) W[c] = va;
                continue;
            }
            u64 v = va;
            if (op <= GLP_GP_OP_MUL) {
                const u64 vb = wp_operand(fb, regs, W, in, pool);
                v = op == GLP_GP_OP_ADD ? add(va, vb) : op == GLP_GP_OP_SUB ? sub(va, vb) : mul(va, vb);
            } else if (op == GLP_WP_OP_INV0) {
                v = winv(va);                             // a^(p - 2), 64 squarings whatever a is; 0 for a = 0
            } else if (op == GLP_WP_OP_BITS) {
                const u32 spec = (u32)pool[fb >> 3], lo = spec & 255, width = spec >> 8;      // uniform: a pool word, lo + 256 width
                v = (va >> lo) & (width >= 64 ? ~0ull : ((1ull << width) - 1));
            } else if (op == GLP_WP_OP_LT) {
                v = va < wp_operand(fb, regs, W, in, pool) ? 1 : 0;
            }
            regs[(((u32)ins >> GLP_GP_DST_SHIFT) & 31) * 64] = v;
        }
    }
}

// the rules of glp_witness_program_check; `where` opens the message: the entry point, or the entry point and "programs[p]"
int witness_program_check(const char *where, const glp_witness_program_desc *d) {
    GLP_REQUIRE(d, "%s: desc is null", where);
    GLP_REQUIRE(d->num_regs >= 1 && d->num_regs <= GLP_GP_MAX_REGS, "%s: desc.num_regs = %u outside 1..%u", where, d->num_regs, GLP_GP_MAX_REGS);
    GLP_REQUIRE(d->num_inputs >= 1 && d->num_inputs <= GLP_WP_MAX_CELLS, "%s: desc.num_inputs = %u outside 1..%u", where, d->num_inputs, GLP_WP_MAX_CELLS);
    GLP_REQUIRE(d->num_outputs >= 1 && d->num_outputs <= GLP_WP_MAX_CELLS, "%s: desc.num_outputs = %u outside 1..%u", where, d->num_outputs, GLP_WP_MAX_CELLS);
    GLP_REQUIRE(d->num_instructions >= 1, "%s: desc.num_instructions is 0: an empty program", where);
    GLP_REQUIRE(d->num_instructions <= GLP_GP_MAX_INSTRUCTIONS, "%s: desc.num_instructions = %u is more than %u", where, d->num_instructions,
                GLP_GP_MAX_INSTRUCTIONS);
    GLP_REQUIRE(d->code, "%s: desc.code is null", where);
    GLP_REQUIRE(d->pool || d->num_pool == 0, "%s: desc.pool is null with num_pool = %u", where, d->num_pool);
    GLP_REQUIRE(d->num_pool <= (1u << 24), "%s: desc.num_pool = %u is more than 2^24", where, d->num_pool);
    const size_t bad = first_noncanonical(d->pool, d->num_pool);
    GLP_REQUIRE(bad == d->num_pool, "%s: desc.pool[%zu] = 0x%016llx is not a canonical field element (>= p)", where, bad,
                (unsigned long long)d->pool[bad == d->num_pool ? 0 : bad]);
    constexpr u32 FIELD = (1u << GLP_GP_OPERAND_BITS) - 1;
    u32 written = 0, emits = 0;
    for (u32 i = 0; i < d->num_instructions; i++) {
        const u64 ins = d->code[i];
        const u32 op = (u32)ins & 15, dst = ((u32)ins >> GLP_GP_DST_SHIFT) & 31;
        const u32 fa = (u32)(ins >> GLP_GP_A_SHIFT) & FIELD, fb = (u32)(ins >> GLP_GP_B_SHIFT) & FIELD;
        GLP_REQUIRE(op >= GLP_GP_OP_ADD && op <= GLP_WP_OP_LT && !(ins >> 63), "%s: instruction %u, field op: 0x%016llx has the unknown opcode %u%s", where, i,
                    (unsigned long long)ins, op, ins >> 63 ? " (bit 63 is set)" : "");
        const bool has_dst = op != GLP_GP_OP_EMIT && op != GLP_GP_OP_END;
        const bool has_b = op <= GLP_GP_OP_MUL || op == GLP_WP_OP_BITS || op == GLP_WP_OP_LT;
        const bool last = i + 1 == d->num_instructions;
        if (last) GLP_REQUIRE(op == GLP_GP_OP_END, "%s: instruction %u, field op: the last instruction is not END", where, i);
        else GLP_REQUIRE(op != GLP_GP_OP_END, "%s: instruction %u, field op: END before the last instruction, a unit program has exactly one", where, i);
        if (has_dst) GLP_REQUIRE(dst < d->num_regs, "%s: instruction %u, field dst: register %u is not below num_regs = %u", where, i, dst, d->num_regs);
        else GLP_REQUIRE(dst == 0, "%s: instruction %u, field dst: %u in an instruction without a destination", where, i, dst);
        if (!has_b) GLP_REQUIRE(fb == 0, "%s: instruction %u, field b: 0x%x in an instruction with one operand", where, i, fb);
        for (int side = 0; side < (has_b ? 2 : 1); side++) {
            const char *field = side ? "b" : "a";
            const u32 f = side ? fb : fa, kind = f & 7, pl = f >> 3;
            if (side && op == GLP_WP_OP_BITS) GLP_REQUIRE(kind == GLP_GP_IMM, "%s: instruction %u, field b: the bit range of BITS is an IMM, not operand kind %u", where, i, kind);
            switch (kind) {
            case GLP_GP_REG:
                GLP_REQUIRE(pl < d->num_regs, "%s: instruction %u, field %s: register %u is not below num_regs = %u", where, i, field, pl, d->num_regs);
                GLP_REQUIRE(written >> pl & 1, "%s: instruction %u, field %s: register %u is read before it is written", where, i, field, pl);
                break;
            case GLP_GP_COL:
                GLP_REQUIRE((pl >> GLP_GP_COL_ORACLE_SHIFT) == 0, "%s: instruction %u, field %s: oracle index %u, a unit program's COL has oracle 0", where, i, field,
                            pl >> GLP_GP_COL_ORACLE_SHIFT);
                GLP_REQUIRE(pl < d->num_inputs, "%s: instruction %u, field %s: input cell %u is not below num_inputs = %u", where, i, field, pl, d->num_inputs);
                break;
            case GLP_GP_IMM:
                GLP_REQUIRE(pl < d->num_pool, "%s: instruction %u, field %s: pool index %u is not below num_pool = %u", where, i, field, pl, d->num_pool);
                break;
            case GLP_GP_COL_NEXT: case GLP_GP_PARAM: case GLP_GP_X:
                GLP_REQUIRE(false, "%s: instruction %u, field %s: operand kind %u (%s) has no meaning in a unit program", where, i, field, kind,
                            kind == GLP_GP_COL_NEXT ? "COL_NEXT" : kind == GLP_GP_PARAM ? "PARAM" : "X");
            default:
                GLP_REQUIRE(false, "%s: instruction %u, field %s: unknown operand kind %u", where, i, field, kind);
            }
        }
        if (op == GLP_WP_OP_BITS) {
            const u64 spec = d->pool[fb >> 3];
            const u32 lo = (u32)spec & 255, width = (u32)(spec >> 8) & 255;
            GLP_REQUIRE(spec >> 16 == 0, "%s: instruction %u, field b: the bit range 0x%llx of BITS has bits set above bit 15 (lo + 256 * width)", where, i,
                        (unsigned long long)spec);
            GLP_REQUIRE(width >= 1, "%s: instruction %u, field b: the bit range of BITS has width 0 (lo = %u)", where, i, lo);
            GLP_REQUIRE(lo + width <= 64, "%s: instruction %u, field b: the bit range of BITS has lo + width = %u + %u, more than 64", where, i, lo, width);
        }
        if (op == GLP_GP_OP_END)
            GLP_REQUIRE((fa & 7) == GLP_GP_IMM && d->pool[fa >> 3] == 1, "%s: instruction %u, field a: the operand of END is not an IMM with the pool word 1", where, i);
        if (has_dst) written |= 1u << dst;
        if (op == GLP_GP_OP_EMIT) emits++;
    }
    GLP_REQUIRE(emits == d->num_outputs, "%s: desc.num_outputs = %u, the program has %u EMITs", where, d->num_outputs, emits);
    return GLP_OK;
}
}  // namespace

extern "C" int glp_witness_program_check(const glp_witness_program_desc *d) { return witness_program_check("glp_witness_program_check", d); }
