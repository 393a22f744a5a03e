// prover_types.h -- host-side types shared by the prover (prover.hip) and the verifier (verifier.hip):
// the circuit handle, the flat proof layout and the Fiat-Shamir transcript.
#pragma once
#include <algorithm>
#include <string.h>
#include <vector>
#include "batch.h"
#include "common.h"
#include "gate_shapes.h"
#include "keccak.h"
#include "poseidon.h"

using namespace glp;
using namespace glf;

constexpr int MAXCH = 4;      // num_challenges supported
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

struct Layout {
    size_t caps, openings, fri_caps, queries, final_poly, pow, pis, total, nopen, query_stride;
    u32 oracle_cols[4], depth0, step_depth[16], final_len;
    u32 leaf_len[4];   // words of one Merkle leaf of oracle k: oracle_cols[k], + SALT_SIZE for the blinded oracles 1..3 of a zk circuit
};

struct glp_circuit {
    glp_ctx *ctx = nullptr;
    glp_circuit_desc d;            // scalars + host copies below
    bool zk = false;               // GLP_CIRCUIT_ZERO_KNOWLEDGE: wires, Z / partial products and quotient oracles are salted
    std::vector<glp_gate> gates;
    std::vector<u64> k_is;
    u64 digest[4];
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
    std::vector<u64> cs_cap;
    Layout L;
    // GLP_GATE_PROGRAM (glp_circuit_create_prog; circuit_program.inc): the programs as the host interpreters read them (the verifier's is
    // in verifier.hip) and, at dev_programs + dev_at, as k_quotient_gate_program / k_witness_check_program read them: the code,
    // zero-padded to a multiple of 4 words, then the pool
    struct Program { std::vector<u64> code, pool; u32 nregs = 0; size_t dev_at = 0; };
    std::vector<Program> programs;
    u64 *dev_programs = nullptr;
    std::vector<u32> program_gates; // the gates of type GLP_GATE_PROGRAM: one k_quotient_gate_program launch each
};

// what the in-circuit rules of a gate program yield (circuit_program.inc): its EMIT count, its degree, and one more than the largest
// wire / constant polynomial it reads
struct CPInfo { u32 emits = 0, degree = 0, wires = 0, consts = 0; };

// dev_sigma_pos on first use (witness_check.inc); shared by glp_witness_check and glp_witness_plan_create (witness.hip)
int witness_sigma_decode(glp_ctx *c, const glp_circuit *cc, const char *fn);

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
