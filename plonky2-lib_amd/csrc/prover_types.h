// prover_types.h -- host-side types shared by the prover (prover.hip) and the verifier (verifier.hip): the circuit handle, which is
// the verifier's view of the circuit (circuit_common.h: description, flat proof layout, programs, cap and digest; the Fiat-Shamir
// transcript is there too) plus everything that lives on the device.
#pragma once
#include <algorithm>
#include <string.h>
#include <vector>
#include "batch.h"
#include "circuit_common.h"
#include "common.h"

constexpr int MAXR = 16;      // 2^rate_bits supported
constexpr u32 APL_WORDS = 4;  // table words per alpha power in the quotient kernels' limb form (quotient_kernels.inc AccHL): m0 | m1 << 32, m2, m0' | m1' << 32, m2'

// per-proof table of the query-round kernel (verify_dev.h), one stride per proof: alpha, z_b, red_b = sum_j alpha^j opening_{b,j}, betas (ext each),
// x_index[nq].  Here because k_trv_pack (transcript_dev.h, compiled into the prover's object too) writes it.
constexpr u32 FT_ALPHA = 0, FT_Z = 2, FT_RED = FT_Z + 2 * GLP_FRI_MAX_POINTS, FT_BETAS = FT_RED + 2 * GLP_FRI_MAX_POINTS, FT_XIDX = FT_BETAS + 32;

struct DevGate { u32 type, selector_index, group_start, group_end, row, num_constraints, p0, p1; };
// CosetInterpolationGate's interpolation domain and barycentric weights, built once in glp_circuit_create and stored behind the
// device gate table (so no kernel argument changes): for subgroup_bits b = 1 .. COSET_MAX_BITS the 2^b pairs
// {x_i = g^i, w_i = x_i / 2^b}, g = the root of unity of order 2^b, from word 2 (2^b - 2) on.  At most 32 pairs per gate.
constexpr u32 COSET_TABLE_WORDS = 2 * ((2u << COSET_MAX_BITS) - 2);
inline void coset_table_fill(u64 *t) {
    for (u32 b = 1; b <= COSET_MAX_BITS; b++) {
        const u64 g = root_of_unity((int)b), ninv = inv((u64)1 << b);
        u64 x = 1;
        for (u32 i = 0; i < (1u << b); i++, x = mul(x, g)) { t[2 * ((1u << b) - 2 + i)] = x; t[2 * ((1u << b) - 2 + i) + 1] = mul(x, ninv); }
    }
}
GLF_HD const u64 *coset_table(const DevGate *gates, u32 num_gates, u32 bits) { return (const u64 *)(gates + num_gates) + 2 * ((1u << bits) - 2); }

struct glp_circuit : CircuitCommon {
    glp_ctx *ctx = nullptr;
    DevGate *dev_gates = nullptr;
    u64 *dev_k_is = nullptr;
    u32 k_ratio = 0;               // g if k_is[j] = g^j for all j with g < 2^32 (then the quotient kernel chains by g), else 0
    u64 *dev_sigmas = nullptr;     // [nr][n] values on H (natural order), for the partial products
    u64 *dev_consts = nullptr;     // [nc][n] values on H (selectors first): which gate sits on a row (witness.hip)
    mutable u32 *dev_sigma_pos = nullptr;   // [nr][n] sigma decoded into flat positions j' n + i': made by witness_sigma_decode (witness_check.inc) for the first caller
    // quotient launch plan (built once in glp_circuit_create): which gates share a launch
    u64 *dev_limb_desc = nullptr;  // [group][num_wires][LIMB_SLOTS] column programs of k_quotient_limbs
    // limb gates in groups of up to LIMB_SLOTS = 5 (one set of accumulators in registers per group; the kernel walks the groups in turn):
    // limb_count = gates over all groups, group g holds gates limb_gi[5 g .. 5 g + limb_gcount[g])
    u32 limb_count = 0, limb_groups = 0, limb_gcount[4] = {0, 0, 0, 0}, limb_gi[20] = {0}, limb_jlo[4] = {0, 0, 0, 0}, limb_jhi[4] = {0, 0, 0, 0};
    u32 limb_extra_count = 0, limb_extra_gi[4] = {0, 0, 0, 0};
    u32 arith_gi = 0, arith_ops = 0;   // ArithmeticGate evaluated inside the permutation loop (0 ops: none)
    u32 light_count = 0, light_gi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<u32> single_gates; // gates that keep a launch of their own
    glp_batch *cs = nullptr;       // constants_sigmas_commitment
    // GLP_GATE_PROGRAM (glp_circuit_create_prog; circuit_program.inc): programs[i] as k_quotient_gate_program / k_witness_check_program
    // read it, at dev_programs + dev_at[i]: the code, zero-padded to a multiple of 4 words, then the pool
    u64 *dev_programs = nullptr;
    std::vector<size_t> dev_at;
    std::vector<u32> program_gates; // the gates of type GLP_GATE_PROGRAM: one k_quotient_gate_program launch each
};

// dev_sigma_pos on first use (witness_check.inc); shared by glp_witness_check and glp_witness_plan_create (witness.hip)
int witness_sigma_decode(glp_ctx *c, const glp_circuit *cc, const char *fn);
