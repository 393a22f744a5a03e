// circuit_common.h -- what a verifier holds of a circuit (plonky2's CommonCircuitData + VerifierOnlyCircuitData) and the host work that
// makes it: the flat proof layout, the rules a description and its gate programs are held to before anything is uploaded, the
// Fiat-Shamir transcript, and the circuit digest.  No HIP runtime call and no context in here: glp_circuit (prover_types.h) derives
// from CircuitCommon and adds the device half; verify_host.h and proof_bytes.h read the view alone, so
// examples/verify_host.cpp runs them, and every refusal below, without a GPU under the host sanitizers (tests/test_verify_host.py).
// The refusals keep the order glp_circuit_create_prog always had; the verifier's unchecked indexing relies on them.
#pragma once
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "acc.h"            // ACC3_MAX_TERMS
#include "fri_shape.h"      // POW_MAX_BITS, fri_proof_layout
#include "gate_shapes.h"
#include "host_check.h"
#include "keccak.h"
#include "poseidon.h"

using namespace glp;
using namespace glf;

constexpr int MAXCH = 4;      // num_challenges supported
constexpr int CIRCUIT_MAX_DEGREE_BITS = 24;     // = NTT_MAX_LG (ntt.h; held equal in circuit_create.inc)

struct Layout {
    size_t caps, openings, fri_caps, queries, final_poly, pow, pis, total, nopen, query_stride;
    u32 oracle_cols[4], depth0, step_depth[16], final_len;
    u32 leaf_len[4];   // words of one Merkle leaf of oracle k: oracle_cols[k], + GLP_SALT_SIZE for the blinded oracles 1..3 of a zk circuit
};
// caps of the three oracles of a proof | openings | the FriProof (fri_shape.h) | public inputs
inline void make_layout(const glp_circuit_desc &c, Layout &L, bool zk) {
    const u32 cap = 1u << c.cap_height, nch = c.num_challenges;
    memset(&L, 0, sizeof(L));
    L.oracle_cols[0] = c.num_constants + c.num_routed_wires;
    L.oracle_cols[1] = c.num_wires;
    L.oracle_cols[2] = nch * (1 + c.num_partial_products);
    L.oracle_cols[3] = nch * c.quotient_degree_factor;
    for (int k = 0; k < 4; k++) L.leaf_len[k] = L.oracle_cols[k] + (zk && k > 0 ? GLP_SALT_SIZE : 0);
    L.nopen = (size_t)c.num_constants + c.num_routed_wires + c.num_wires + 2 * nch + nch * c.num_partial_products +
              nch * c.quotient_degree_factor;
    L.openings = 3 * (size_t)cap * 4;
    L.fri_caps = L.openings + 2 * L.nopen;
    const FriProofLayout f = fri_proof_layout(c.degree_bits + c.rate_bits, c.rate_bits, c.cap_height, L.leaf_len, 4, c.reduction_arity_bits,
                                              c.num_reductions, c.num_query_rounds);
    L.depth0 = f.depth0;
    for (u32 i = 0; i < c.num_reductions; i++) L.step_depth[i] = f.step_depth[i];
    L.query_stride = f.query_stride;
    L.final_len = f.final_len;
    L.queries = L.fri_caps + f.queries;
    L.final_poly = L.fri_caps + f.final_poly;
    L.pow = L.fri_caps + f.pow;
    L.pis = L.fri_caps + f.total;
    L.total = L.pis + c.num_public_inputs;
}

// ------------------------------------------------------------------------------------------ gate programs: the rules
struct GPInfo { u32 maxc, cols_named, next_mask; };
// what the in-circuit rules of a gate program yield: its EMIT count, its degree, and one more than the largest wire / constant
// polynomial it reads
struct CPInfo { u32 emits = 0, degree = 0, wires = 0, consts = 0; };

// the rules of glp_gate_program_check (gate_program.inc); `fn` names the entry point in the message
inline int gate_program_check(const char *fn, const glp_gate_program_desc *d, GPInfo &info) {
    GLP_REQUIRE(d, "%s: desc is null", fn);
    GLP_REQUIRE(d->num_regs >= 1 && d->num_regs <= GLP_GP_MAX_REGS, "%s: desc.num_regs = %u outside 1..%u", fn, d->num_regs, GLP_GP_MAX_REGS);
    GLP_REQUIRE(d->num_oracles >= 1 && d->num_oracles <= GLP_GP_MAX_ORACLES, "%s: desc.num_oracles = %u outside 1..%u", fn, d->num_oracles,
                GLP_GP_MAX_ORACLES);
    GLP_REQUIRE(d->oracle_cols, "%s: desc.oracle_cols is null", fn);
    GLP_REQUIRE(d->num_instructions >= 1, "%s: desc.num_instructions is 0: an empty program", fn);
    GLP_REQUIRE(d->num_instructions <= GLP_GP_MAX_INSTRUCTIONS, "%s: desc.num_instructions = %u is more than %u", fn, d->num_instructions,
                GLP_GP_MAX_INSTRUCTIONS);
    GLP_REQUIRE(d->code, "%s: desc.code is null", fn);
    GLP_REQUIRE(d->pool || d->num_pool == 0, "%s: desc.pool is null with num_pool = %u", fn, d->num_pool);
    GLP_REQUIRE(d->num_pool <= (1u << 24) && d->num_params <= (1u << 24), "%s: desc.num_pool = %u or num_params = %u is more than 2^24", fn,
                d->num_pool, d->num_params);
    const size_t bad = first_noncanonical(d->pool, d->num_pool);
    GLP_REQUIRE(bad == d->num_pool, "%s: desc.pool[%zu] = 0x%016llx is not a canonical field element (>= p)", fn, bad,
                (unsigned long long)d->pool[bad == d->num_pool ? 0 : bad]);
    u32 written = 0, emits = 0;
    std::vector<u32> named;
    info.maxc = 0; info.next_mask = 0;
    for (u32 i = 0; i < d->num_instructions; i++) {
        const u64 ins = d->code[i];
        const u32 op = (u32)ins & 15, dst = ((u32)ins >> GLP_GP_DST_SHIFT) & 31;
        const u32 fa = (u32)(ins >> GLP_GP_A_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), fb = (u32)(ins >> GLP_GP_B_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1);
        GLP_REQUIRE(op >= GLP_GP_OP_ADD && op <= GLP_GP_OP_END && !(ins >> 63), "%s: instruction %u, field op: 0x%016llx has the unknown opcode %u%s", fn, i,
                    (unsigned long long)ins, op, ins >> 63 ? " (bit 63 is set)" : "");
        const bool has_dst = op <= GLP_GP_OP_MOV, has_b = op <= GLP_GP_OP_MUL;
        if (has_dst) GLP_REQUIRE(dst < d->num_regs, "%s: instruction %u, field dst: register %u is not below num_regs = %u", fn, i, dst, d->num_regs);
        else GLP_REQUIRE(dst == 0, "%s: instruction %u, field dst: %u in an instruction without a destination", fn, i, dst);
        if (!has_b) GLP_REQUIRE(fb == 0, "%s: instruction %u, field b: 0x%x in an instruction with one operand", fn, i, fb);
        for (int side = 0; side < (has_b ? 2 : 1); side++) {
            const char *field = side ? "b" : "a";
            const u32 f = side ? fb : fa, kind = f & 7, pl = f >> 3;
            switch (kind) {
            case GLP_GP_REG:
                GLP_REQUIRE(pl < d->num_regs, "%s: instruction %u, field %s: register %u is not below num_regs = %u", fn, i, field, pl, d->num_regs);
                GLP_REQUIRE(written >> pl & 1, "%s: instruction %u, field %s: register %u is read before it is written", fn, i, field, pl);
                break;
            case GLP_GP_COL: case GLP_GP_COL_NEXT: {
                const u32 o = pl >> GLP_GP_COL_ORACLE_SHIFT, col = pl & ((1u << GLP_GP_COL_ORACLE_SHIFT) - 1);
                GLP_REQUIRE(o < d->num_oracles, "%s: instruction %u, field %s: oracle index %u is not below num_oracles = %u", fn, i, field, o, d->num_oracles);
                GLP_REQUIRE(col < d->oracle_cols[o], "%s: instruction %u, field %s: column index %u is not below oracle_cols[%u] = %u", fn, i, field, col, o,
                            d->oracle_cols[o]);
                named.push_back(pl);
                if (kind == GLP_GP_COL_NEXT) info.next_mask |= 1u << o;
                break;
            }
            case GLP_GP_IMM:
                GLP_REQUIRE(pl < d->num_pool, "%s: instruction %u, field %s: pool index %u is not below num_pool = %u", fn, i, field, pl, d->num_pool);
                break;
            case GLP_GP_PARAM:
                GLP_REQUIRE(pl < d->num_params, "%s: instruction %u, field %s: param index %u is not below num_params = %u", fn, i, field, pl, d->num_params);
                break;
            case GLP_GP_X:
                GLP_REQUIRE(pl == 0, "%s: instruction %u, field %s: X with the payload %u", fn, i, field, pl);
                break;
            default:
                GLP_REQUIRE(false, "%s: instruction %u, field %s: unknown operand kind %u", fn, i, field, kind);
            }
        }
        if (has_dst) written |= 1u << dst;
        if (op == GLP_GP_OP_EMIT) {
            emits++;
            GLP_REQUIRE(emits <= GLP_GP_MAX_CONSTRAINTS, "%s: instruction %u, field op: EMIT number %u of one gate, more than %u", fn, i, emits, GLP_GP_MAX_CONSTRAINTS);
        } else if (op == GLP_GP_OP_END) {
            info.maxc = std::max(info.maxc, emits);
            emits = 0;
        }
        if (i + 1 == d->num_instructions)
            GLP_REQUIRE(op == GLP_GP_OP_END, "%s: instruction %u, field op: the last instruction is not END", fn, i);
    }
    std::sort(named.begin(), named.end());
    info.cols_named = (u32)(std::unique(named.begin(), named.end()) - named.begin());
    return GLP_OK;
}
// the in-circuit rules on top of glp_gate_program_check's (circuit_program.inc); `fn` names the entry point (and the program) in the message
inline int circuit_program_check(const char *fn, const glp_gate_program_desc *d, CPInfo &info) {
    info = CPInfo();
    GPInfo gi;
    GLP_TRY(gate_program_check(fn, d, gi));
    GLP_REQUIRE(d->num_oracles == 2, "%s: desc.num_oracles = %u: a gate of a circuit reads oracle 0 (the constants) and oracle 1 (the wires)", fn,
                d->num_oracles);
    GLP_REQUIRE(d->num_params <= 4, "%s: desc.num_params = %u: the params of a gate of a circuit are the 4 words of the public-input hash", fn,
                d->num_params);
    u32 deg[GLP_GP_MAX_REGS] = {0};
    for (u32 i = 0; i < d->num_instructions; i++) {
        const u64 ins = d->code[i];
        const u32 op = (u32)ins & 15, dst = ((u32)ins >> GLP_GP_DST_SHIFT) & 31;
        const u32 f[2] = {(u32)(ins >> GLP_GP_A_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1), (u32)(ins >> GLP_GP_B_SHIFT) & ((1u << GLP_GP_OPERAND_BITS) - 1)};
        u32 dg[2] = {0, 0};
        for (int side = 0; side < (op <= GLP_GP_OP_MUL ? 2 : 1); side++) {
            const char *field = side ? "b" : "a";
            const u32 kind = f[side] & 7, pl = f[side] >> 3;
            GLP_REQUIRE(kind != GLP_GP_COL_NEXT, "%s: instruction %u, field %s: COL_NEXT: a gate of a circuit does not see the next row", fn, i, field);
            GLP_REQUIRE(kind != GLP_GP_X, "%s: instruction %u, field %s: X: a gate of a circuit does not see the point", fn, i, field);
            if (kind == GLP_GP_REG) dg[side] = deg[pl];
            else if (kind == GLP_GP_COL) {
                const u32 col = pl & ((1u << GLP_GP_COL_ORACLE_SHIFT) - 1);
                u32 &used = pl >> GLP_GP_COL_ORACLE_SHIFT ? info.wires : info.consts;
                used = std::max(used, col + 1);
                dg[side] = 1;
            }
        }
        if (op <= GLP_GP_OP_MOV) {
            const u64 sum = (u64)dg[0] + dg[1];
            deg[dst] = op == GLP_GP_OP_MUL ? (u32)std::min<u64>(sum, 0xFFFFFFFFu) : std::max(dg[0], dg[1]);
        } else if (op == GLP_GP_OP_EMIT) {
            info.emits++;
            GLP_REQUIRE(info.emits <= GLP_GATE_PROGRAM_MAX_CONSTRAINTS, "%s: instruction %u, field op: EMIT number %u, more than the %u the quotient accumulators hold",
                        fn, i, info.emits, GLP_GATE_PROGRAM_MAX_CONSTRAINTS);
            info.degree = std::max(info.degree, dg[0]);
        } else {
            GLP_REQUIRE(i + 1 == d->num_instructions, "%s: instruction %u, field op: END before the last instruction (a gate of a circuit is one gate)", fn, i);
            const u32 kind = f[0] & 7, pl = f[0] >> 3;
            GLP_REQUIRE(kind == GLP_GP_IMM && d->pool[pl] == 1, "%s: instruction %u, field a: the operand of END must be IMM of a pool word 1 (the selector filter is "
                        "the library's)", fn, i);
        }
    }
    return GLP_OK;
}

// ------------------------------------------------------------------------------------------ a description: the rules
// What glp_circuit_create_prog asks of a description before it allocates anything, the canonical form of the field arrays apart
// (circuit_fields_check, next).
// (The flags play no part: the caller has refused unknown ones, and no rule depends on zero knowledge.)
inline int circuit_desc_check(const glp_circuit_desc &d, const glp_gate_program_desc *programs, u32 num_programs) {
    GLP_REQUIRE(d.gates && d.k_is && d.constants && d.sigmas, "null array in circuit description");
    GLP_REQUIRE(d.num_challenges >= 1 && d.num_challenges <= (u32)MAXCH, "num_challenges=%u outside 1..%d", d.num_challenges, MAXCH);
    if (d.hasher != GLP_HASH_POSEIDON && d.hasher != GLP_HASH_KECCAK25) return set_error(GLP_ERR_UNSUPPORTED, "hasher %u is not one of GLP_HASH_*", d.hasher);
    GLP_REQUIRE(d.rate_bits >= 1 && d.rate_bits <= 4, "rate_bits=%u outside 1..4", d.rate_bits);
    GLP_REQUIRE(d.num_routed_wires <= d.num_wires && d.num_routed_wires > 0, "bad wire counts");
    if ((int)d.degree_bits > CIRCUIT_MAX_DEGREE_BITS) return set_error(GLP_ERR_UNSUPPORTED, "degree_bits=%u > %d", d.degree_bits, CIRCUIT_MAX_DEGREE_BITS);
    const u32 qdf = d.quotient_degree_factor;
    if (qdf == 0 || (qdf & (qdf - 1)) || qdf > (1u << d.rate_bits))
        return set_error(GLP_ERR_UNSUPPORTED, "quotient_degree_factor=%u must be a power of two <= 2^rate_bits", qdf);
    GLP_REQUIRE(d.num_partial_products == (d.num_routed_wires + qdf - 1) / qdf - 1, "num_partial_products inconsistent");
    GLP_REQUIRE(d.num_reductions <= 16 && d.cap_height <= d.degree_bits + d.rate_bits, "bad FRI parameters");
    GLP_REQUIRE(d.proof_of_work_bits <= POW_MAX_BITS, "proof_of_work_bits=%u: this build searches at most 2^40 candidates and accepts up to %u bits",
                d.proof_of_work_bits, POW_MAX_BITS);
    u32 sum_ab = 0;
    for (u32 i = 0; i < d.num_reductions; i++) {
        GLP_REQUIRE(d.reduction_arity_bits[i] >= 1 && d.reduction_arity_bits[i] <= 5, "arity_bits outside 1..5");
        sum_ab += d.reduction_arity_bits[i];
        GLP_REQUIRE(sum_ab <= d.degree_bits && d.degree_bits + d.rate_bits - sum_ab >= d.cap_height, "FRI reduction deeper than the domain");
    }
    // Shapes the quotient kernel assumes (gate_shapes.h), checked here so that a malformed description is an error and never an
    // out-of-bounds read on the device: wires / constants / constraints each gate type touches.
    std::vector<CPInfo> pinfo(num_programs);
    for (u32 i = 0; i < num_programs; i++) {
        char who[64];
        snprintf(who, sizeof(who), "glp_circuit_create_prog: programs[%u]", i);
        GLP_TRY(circuit_program_check(who, programs + i, pinfo[i]));
    }
    u32 maxc = 0;
    for (u32 i = 0; i < d.num_gates; i++) {
        const glp_gate &g = d.gates[i];
        GateShape s;
        if (g.type == GLP_GATE_PROGRAM && num_programs) {
            // the shape of a program gate is what its program reads and emits; held to the degree rule of the recursion gates below
            GLP_REQUIRE(g.p0 < num_programs, "gate %u (type %u), field p0: program %u, the circuit has num_programs = %u", i, g.type, g.p0, num_programs);
            GLP_REQUIRE(g.p1 == 0, "gate %u (type %u), field p1: %u, must be 0", i, g.type, g.p1);
            const CPInfo &pi = pinfo[g.p0];
            s = GateShape();
            s.wires = pi.wires; s.constraints = pi.emits; s.degree = pi.degree;
            GLP_REQUIRE(s.constraints == g.num_constraints, "gate %u (type %u), field num_constraints: %u, program %u has %u EMITs", i, g.type,
                        g.num_constraints, g.p0, s.constraints);
            GLP_REQUIRE(s.wires <= d.num_wires, "gate %u (type %u), field p0: program %u reads wire %u, the circuit has num_wires = %u", i, g.type, g.p0,
                        s.wires - 1, d.num_wires);
            GLP_REQUIRE(pi.consts <= d.num_constants, "gate %u (type %u), field p0: program %u reads constant polynomial %u, the circuit has num_constants = %u",
                        i, g.type, g.p0, pi.consts - 1, d.num_constants);
        } else if (!gate_type_known(g.type) || !gate_shape(g, s))
            return set_error(gate_type_known(g.type) ? GLP_ERR_ARG : GLP_ERR_UNSUPPORTED,
                             "gate %u: type %u with parameters (%u, %u) is not supported", i, g.type, g.p0, g.p1);
        GLP_REQUIRE(s.wires <= d.num_wires, "gate %u (type %u) needs %u wires, circuit has %u", i, g.type, s.wires, d.num_wires);
        GLP_REQUIRE(d.num_selectors + s.consts <= d.num_constants, "gate %u (type %u) needs %u constants", i, g.type, s.consts);
        GLP_REQUIRE(s.constraints == g.num_constraints, "gate %u (type %u): num_constraints %u, expected %u", i, g.type, g.num_constraints, s.constraints);
        GLP_REQUIRE(s.routed <= d.num_routed_wires, "gate %u (type %u): %u routed inputs, circuit has %u routed wires", i, g.type, s.routed,
                    d.num_routed_wires);
        if (s.degree || g.type == GLP_GATE_PROGRAM) {
            // The quotient is evaluated on quotient_degree_factor cosets, so filter x constraint may have degree quotient_degree_factor + 1
            // at most (what plonky2's selector grouping guarantees for every gate it places): the filter has one factor per other gate of
            // the group, and the UNUSED factor when there are several selectors.
            const u32 filt = g.group_end - g.group_start - 1 + (d.num_selectors > 1 ? 1 : 0);
            GLP_REQUIRE(g.group_start < g.group_end && s.degree + filt <= qdf + 1, "gate %u (type %u): degree %u with a selector filter of degree %u exceeds "
                        "quotient_degree_factor %u + 1", i, g.type, s.degree, g.group_start < g.group_end ? filt : 0, qdf);
        }
        GLP_REQUIRE(g.selector_index < d.num_selectors && g.group_start <= g.row && g.row < g.group_end, "bad selector data for gate %u", i);
        GLP_REQUIRE(g.type == GLP_GATE_PROGRAM || g.num_constraints <= ACC3_MAX_TERMS, "gate %u: %u constraints exceed the %u the quotient accumulators hold", i,
                    g.num_constraints, ACC3_MAX_TERMS);      // a program gate: GLP_GATE_PROGRAM_MAX_CONSTRAINTS, held by circuit_program_check
        maxc = std::max(maxc, g.num_constraints);
    }
    GLP_REQUIRE(maxc <= d.num_gate_constraints, "num_gate_constraints smaller than a gate's constraint count");
    return GLP_OK;
}
// field arrays from outside: canonical or rejected by name (one host pass, small against the uploads and the commitment that follow).
// tables = false: the coset shifts alone, for a holder of the view, who never sees the constants and the sigmas.
inline int circuit_fields_check(const glp_circuit_desc &d, bool tables) {
    const size_t nrows = (size_t)1 << d.degree_bits;
    const u64 *sec[3] = {d.k_is, d.constants, d.sigmas};
    const size_t cnt[3] = {d.num_routed_wires, (size_t)d.num_constants * nrows, (size_t)d.num_routed_wires * nrows};
    const char *names[3] = {"k_is", "constants", "sigmas"};
    for (int i = 0; i < (tables ? 3 : 1); i++) {
        const size_t bad = first_noncanonical(sec[i], cnt[i]);
        GLP_REQUIRE(bad == cnt[i], "%s[%zu] = 0x%016llx is not a canonical field element (>= p)", names[i], bad, (unsigned long long)sec[i][bad]);
    }
    return GLP_OK;
}

// ------------------------------------------------------------------------------------------ transcript
struct Challenger {   // iop/challenger.rs, overwrite-mode duplex sponge; challenges pop from the END of the rate
    u64 st[12]; u64 in[8]; int nin = 0; u64 out[8]; int nout = 0;
    int hasher = GLP_HASH_POSEIDON;      // H::Permutation: Poseidon, or KeccakPermutation (hash chain, keccak.h)
    explicit Challenger(int hasher_ = GLP_HASH_POSEIDON) : hasher(hasher_) { memset(st, 0, sizeof(st)); }
    void duplex() {
        for (int i = 0; i < nin; i++) st[i] = in[i];
        nin = 0;
        if (hasher == GLP_HASH_KECCAK25) kec::permute(st); else pos::permute(st);
        memcpy(out, st, 64); nout = 8;
    }
    // observe_hash / observe_cap for digests of the proof's hasher: a HashOut is its 4 elements, a BytesHash<25> its four 7-byte chunks
    void observe_hashes(const u64 *digests, size_t count) {
        for (size_t i = 0; i < count; i++) {
            if (hasher == GLP_HASH_KECCAK25) { u64 e[4]; kec::digest_to_elements(digests + 4 * i, e); observe(e, 4); }
            else observe(digests + 4 * i, 4);
        }
    }
    void observe(const u64 *e, size_t n) {
        for (size_t i = 0; i < n; i++) { nout = 0; in[nin++] = e[i]; if (nin == 8) duplex(); }
    }
    u64 get() { if (nin > 0 || nout == 0) duplex(); return out[--nout]; }
    ext2 get_ext() { u64 a = get(); u64 b = get(); return e_make(a, b); }
};
inline void host_hash_no_pad(const u64 *in, size_t len, u64 out[4]) {
    u64 st[12] = {0};
    for (size_t off = 0; off < len; off += 8) {
        size_t c = std::min<size_t>(8, len - off);
        for (size_t i = 0; i < c; i++) st[i] = in[off + i];
        pos::permute(st);
    }
    memcpy(out, st, 32);
}

// ------------------------------------------------------------------------------------------ the view
struct CircuitCommon {
    glp_circuit_desc d;            // scalars + host copies below
    bool zk = false;               // GLP_CIRCUIT_ZERO_KNOWLEDGE: wires, Z / partial products and quotient oracles are salted
    std::vector<glp_gate> gates;
    std::vector<u64> k_is;
    u64 digest[4];
    std::vector<u64> cs_cap;       // the cap of constants_sigmas_commitment
    Layout L;
    // GLP_GATE_PROGRAM (glp_circuit_create_prog): the programs as the host interpreter reads them (program_constraints, verify_host.h)
    struct Program { std::vector<u64> code, pool; u32 nregs = 0; };
    std::vector<Program> programs;
};
// the view of a description that circuit_desc_check has accepted, all but the commitment
inline void circuit_common_describe(CircuitCommon &v, const glp_circuit_desc &d, u32 flags, const glp_gate_program_desc *programs, u32 num_programs) {
    v.d = d;
    v.gates.assign(d.gates, d.gates + d.num_gates);
    v.k_is.assign(d.k_is, d.k_is + d.num_routed_wires);
    v.d.gates = v.gates.data(); v.d.k_is = v.k_is.data(); v.d.constants = nullptr; v.d.sigmas = nullptr;
    v.zk = (flags & GLP_CIRCUIT_ZERO_KNOWLEDGE) != 0;
    make_layout(v.d, v.L, v.zk);
    for (u32 i = 0; i < num_programs; i++) {
        const glp_gate_program_desc &pd = programs[i];
        CircuitCommon::Program pr;
        pr.code.assign(pd.code, pd.code + pd.num_instructions);
        pr.pool.assign(pd.pool, pd.pool + pd.num_pool);
        pr.nregs = pd.num_regs;
        v.programs.push_back(std::move(pr));
    }
}
// its commitment: the constants/sigmas cap and the digest -- the description's circuit_digest, or if that is zero the library's
// recipe over the cap
inline void circuit_common_commit(CircuitCommon &v, const std::vector<u64> &cs_cap) {
    const glp_circuit_desc &d = v.d;
    v.cs_cap = cs_cap;
    bool zero = true;
    for (int i = 0; i < 4; i++) zero = zero && d.circuit_digest[i] == 0;
    if (zero && d.hasher == GLP_HASH_KECCAK25) {
        // the same recipe with C::Hasher = KeccakHash<25>: every hash enters as its four 7-byte chunks (BytesHash::to_vec)
        u64 pad[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, ds[4], e[4];
        kec::host_hash_no_pad(pad, 12, ds);
        std::vector<u64> parts;
        for (size_t i = 0; i < v.cs_cap.size(); i += 4) { kec::digest_to_elements(&v.cs_cap[i], e); parts.insert(parts.end(), e, e + 4); }
        kec::digest_to_elements(ds, e);
        parts.insert(parts.end(), e, e + 4);
        parts.push_back(d.degree_bits);
        kec::host_hash_no_pad(parts.data(), parts.size(), v.digest);
    } else if (zero) {
        // hash_pad([]) = hash_no_pad([1, 0 x 10, 1]); digest = hash_no_pad(cap ++ that ++ [degree_bits])
        u64 pad[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, ds[4];
        host_hash_no_pad(pad, 12, ds);
        std::vector<u64> parts(v.cs_cap);
        parts.insert(parts.end(), ds, ds + 4);
        parts.push_back(d.degree_bits);
        host_hash_no_pad(parts.data(), parts.size(), v.digest);
    } else {
        memcpy(v.digest, d.circuit_digest, 32);
    }
    memcpy(v.d.circuit_digest, v.digest, 32);
}
