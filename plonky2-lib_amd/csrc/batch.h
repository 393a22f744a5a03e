// batch.h -- device-resident PolynomialBatch (plonky2 `fri/oracle.rs`).
#pragma once
#include "common.h"

struct glp_batch {
    glp_ctx *ctx = nullptr;
    u32 ncols = 0;
    int lg = 0, rate_bits = 0, cap_height = 0;
    u64 *coeffs = nullptr;    // [ncols][n]     bit-reversed coefficient order
    u64 *lde = nullptr;       // [ncols + salt][R][n]  coset-major LDE values, salt columns last
    u32 salt = 0;             // SALT_SIZE = 4 for a blinded batch (PolynomialBatch blinding = true), else 0; leaves are ncols + salt wide
    u64 *digests = nullptr;   // [ndigests][4]  level 0 (leaf j at slot j) ... cap level
    size_t ndigests = 0;
    int hasher = GLP_HASH_POSEIDON;   // GenericConfig::Hasher of the tree
    u32 K = 1;                // many-proofs batches (glp_prove_batch, glp_batch_many_from_*): K independent oracles of identical shape, arrays [K][...]
    bool view = false;        // glp_batch_member: a K = 1 window into a many-proofs batch; the pointers belong to the parent
};

namespace glp {
enum BatchInput { BATCH_VALUES = 0, BATCH_COEFFS_NATURAL = 1, BATCH_COEFFS_BITREV = 2 };
// The shape rules of a batch of K oracles, stated once: K in 1..65535 (the tree index rides in grid.y), log_n <= NTT_MAX_LG and a known
// hasher (GLP_ERR_UNSUPPORTED), rate_bits <= 4, cap_height <= log_n + rate_bits, ncols > 0, K * ncols columns in 31 bits and, where
// max_bytes is given, an LDE of at most that many bytes (GLP_ERR_ARG).  `fn`, if not null, names the entry point in the message.
// batch_build calls it first; an entry point that allocates or uploads before batch_build calls it up front, with BATCH_MAX_BYTES.
constexpr size_t BATCH_MAX_BYTES = (size_t)64 << 30;
int batch_shape_check(const char *fn, u32 K, size_t ncols, u32 log_n, u32 rate_bits, u32 cap_height, u32 hasher, size_t max_bytes = 0);
// One pipeline for every K >= 1: coeffs [K * ncols][n], LDE [K][ncols + salt][N], one tree per member; K = 1 is the one-member case.
int batch_build(glp_ctx *c, const u64 *dev_in, int input_kind, u32 ncols, int lg, int rate_bits, int cap_height,
                glp_batch **out, const u64 *host_src = nullptr, u32 K = 1, int hasher = GLP_HASH_POSEIDON,
                const u64 *salt_seed = nullptr /* non-null: blinded, 4 salt columns (merkle_fill_salts) */, u32 salt_tag = 0);
constexpr u32 SALT_SIZE = 4;
void batch_destroy(glp_batch *b);
// Values on the planes of `channels` cosets shift * <w_M>, M = n << sub_bits, to their coefficients in chunks of n (prover.hip).
//   pv   [channels][S][n], S = 2^sub_bits: plane r slot q holds the value at shift * w_M^(q S + r)
//   out  [channels * S][n], bit-reversed order: chunk j of a channel is its X^(j n) block (`coeffs.chunks(n)`)
//   pV   scratch of the same size; out may be pV
int coset_planes_to_chunk_coeffs(glp_ctx *c, const u64 *pv, u64 *pV, u64 *out, u32 channels, int lg, int sub_bits, u64 shift);
}  // namespace glp
