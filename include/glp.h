/*
 * glp.h -- C ABI of libglprover.so: an MI355X (gfx950) backend for the Goldilocks-field
 * `CircuitData::prove()` path of the plonky2 fork that Orbiter-Finance/Plonky2-lib drives
 * (every `data.prove(pw)` call site, e.g. [REF src/ecdsa/gadgets/ecdsa.rs:349],
 * [REF src/hash/keccak256.rs:248], [REF src/zkdsa/circuits/mod.rs:326]).
 *
 * The prover's arithmetic lives in the `plonky2` crate, a path-patched dependency that is NOT
 * part of /root/reference [REF Cargo.toml:10-12,32-34]; the entry points below are what an
 * `extern "C"` block inside that crate would bind, at the same seams where the fork links its
 * CUDA NTT library (sppark, [REF Cargo.lock:955-977,1411-1416]).  Each function names the
 * plonky2 0.1.4 item it replaces.  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions: every function returns GLP_OK (0) or a negative error code and records a message
 * retrievable with glp_last_error() (thread-local).  Pointers are caller-owned HOST memory
 * unless the parameter name starts with `dev_`.  Field elements are canonical uint64_t
 * (< p = 2^64 - 2^32 + 1); extension elements are two consecutive uint64_t (a + b*X, X^2 = 7).
 * A word >= p in an array of field elements, at every entry point that takes one:
 *   HOST array     refused: GLP_ERR_ARG before anything is allocated or launched, the message naming the function, the parameter,
 *                  the position (proof / column / index) and the value; an in-place array is left as it was, no handle comes back.
 *   DEVICE array   (`dev_*`, or `*_on_device` != 0) reduced mod p once as it is loaded: every result is word for word the result
 *                  for `input % p`, everything stored or handed back is canonical, a const buffer is not written to.
 * Seeds are taken mod p.  Each entry point below says "host: refused" / "device: reduced" where its wording is not the rule's own.
 * A glp_ctx is bound to one GPU and one HIP stream; calls on one ctx must be serialised by the
 * caller; distinct ctxs are independent (this is what shards a batch of proofs over 8 GPUs).
 * There is no CPU fallback: without a usable gfx950 device glp_ctx_create fails.
 */
#ifndef GLP_H
#define GLP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define GLP_API __attribute__((visibility("default")))
#else
#define GLP_API
#endif

#define GLP_OK 0
#define GLP_ERR_ARG (-1)         /* bad argument (null pointer, size out of range, ...) */
#define GLP_ERR_HIP (-2)         /* a HIP runtime call failed; message has the HIP error string */
#define GLP_ERR_UNSUPPORTED (-3) /* valid request outside what this build implements */
#define GLP_ERR_NOGPU (-4)       /* no gfx950 device visible */
#define GLP_ERR_PROVE (-5)       /* prove: the transcript cannot continue (PoW search exhausted, zeta in the subgroup); verify: proof rejected */

#define GLP_HASH_POSEIDON 0      /* PoseidonGoldilocksConfig */
#define GLP_HASH_KECCAK25 1      /* KeccakGoldilocksConfig: KeccakHash<25> [REF src/hash/keccak256.rs:281] */

typedef struct glp_ctx glp_ctx;
typedef struct glp_batch glp_batch; /* plonky2 `PolynomialBatch`: coefficients + LDE + Merkle tree, device resident */

GLP_API const char *glp_last_error(void);
GLP_API const char *glp_version(void);
GLP_API int glp_device_count(void);

/* Environment variables read when a context is made (tuning switches for the A/B rows under profiles/; the defaults ship):
 *   GLP_NTT_2PASS_LG      = 20..22 (default 22): largest log2(n) transformed in two passes; above it a third pass over 2^20-point blocks
 *   GLP_NTT_STRIDED32_LW  = 3 | 4  (default 4):  log2 columns of the 512- / 1024-row strided tile (64- or 128-byte row segments)
 *   GLP_NTT_STRIDED32_TL  = 1..64  (default 8):  tiles one block of that kernel walks, software-pipelined (1 = one tile per block)
 *   GLP_MERKLE_COOP_MAX   (default 4096), GLP_MERKLE_QUAD_MAX (default 32768): Poseidon leaf hashing spreads one sponge over 12 of 16 lanes up to
 *                         the first many leaves per launch, over a quad of lanes up to the second, and keeps one sponge per lane above it
 *                         (FRI layers alike; Merkle levels: 12 of 16 lanes up to 8192 parents, a quad up to the second threshold)
 *   GLP_HOST_THREADS      (read on the first glp_prove_batch of a context): host threads for the transcripts of a batch
 *   GLP_WITNESS_NARROW_MAX (read when a witness plan is made; default 256): a wave of glp_witness_generate with more units than this gets
 *                         launches of its own while num_proofs is below the CU count ("witness generation, the dataflow half")
 *   GLP_POOL_POISON       = 0..255 (default unset; a test switch, slow): every block of the context's device pool, the library's own scratch
 *                         and glp_dev_alloc alike, is filled with that byte when it is handed out and again when it is returned, on the
 *                         context's stream, which is drained after each fill.  Results must not depend on it. */
GLP_API int glp_ctx_create(int device_id, glp_ctx **out);
GLP_API void glp_ctx_destroy(glp_ctx *ctx);
GLP_API int glp_ctx_synchronize(glp_ctx *ctx);
/* The HIP stream (hipStream_t) every kernel of this ctx is launched on. */
GLP_API void *glp_ctx_stream(glp_ctx *ctx);
/* Seed of the salts of zero-knowledge proofs (GLP_CIRCUIT_ZERO_KNOWLEDGE; rule at glp_batch_from_values_salted).  NULL (the default):
 * every glp_prove* call, session and glp_prove_batch call draws a fresh seed from the OS (getrandom).  A fixed seed makes proofs
 * reproducible, for tests; proving two different witnesses of one circuit with the same fixed seed reuses the salts and breaks
 * hiding.  Seed words are taken mod p. */
GLP_API int glp_ctx_set_salt_seed(glp_ctx *ctx, const uint64_t seed[4]);

/* Device buffers for the *_device entry points, for callers that do not link a HIP runtime themselves (a Rust / Go host
 * that keeps a witness resident in HBM across proofs).  Memory comes from and returns to the context's pool. */
GLP_API int glp_dev_alloc(glp_ctx *ctx, size_t bytes, void **dev_out);
GLP_API int glp_dev_free(glp_ctx *ctx, void *dev);
GLP_API int glp_dev_upload(glp_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);     /* synchronous */
GLP_API int glp_dev_download(glp_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);   /* synchronous */

/* ---- per-stage device timing (hipEvent pairs on the ctx stream) -------------------------------
 * With profiling on, each kernel stage of the following calls is bracketed by events.
 * glp_ctx_stage_count / glp_ctx_stage_get read them back after synchronising. */
GLP_API int glp_ctx_set_profiling(glp_ctx *ctx, int on);
GLP_API int glp_ctx_stage_reset(glp_ctx *ctx);
GLP_API int glp_ctx_stage_count(glp_ctx *ctx);
GLP_API int glp_ctx_stage_get(glp_ctx *ctx, int index, const char **name, float *ms, double *algorithmic_bytes);

/* ---- primitives (used by the parity tests and by a fine-grained FFI binding) ------------------ */
/* hash/poseidon.rs `Poseidon::poseidon`: permute `count` states of 12 elements on the GPU.  A word >= p: refused (host array). */
GLP_API int glp_poseidon_permute(glp_ctx *ctx, uint64_t *states, size_t count);
/* field/src/fft.rs `fft` / `ifft` on `ncols` independent columns of n = 2^log_n elements,
 * natural order in and out (values[i] = p(w^i), w = primitive_root_of_unity(log_n)).  A word >= p: refused (host arrays), cols unchanged. */
GLP_API int glp_fft(glp_ctx *ctx, uint64_t *cols, uint32_t ncols, uint32_t log_n);
GLP_API int glp_ifft(glp_ctx *ctx, uint64_t *cols, uint32_t ncols, uint32_t log_n);
/* polynomial/mod.rs `lde(rate_bits)` + `coset_fft(shift)`: in [ncols][n] coefficients,
 * out [ncols][n << rate_bits] values, out[c][i] = p_c(shift * W^i), natural order.  A coefficient >= p: refused (host array). */
GLP_API int glp_lde(glp_ctx *ctx, const uint64_t *coeffs, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
            uint64_t shift, uint64_t *out);

/* Synthetic-trace helper for benchmarks: dev_out[i] = SplitMix64(seed, i) folded into [0, p)
 * (z >= p ? z - p : z).  Lets bench.py create HBM-resident inputs without a PCIe copy. */
GLP_API int glp_fill_random_device(glp_ctx *ctx, uint64_t *dev_out, size_t count, uint64_t seed);

/* ---- PolynomialBatch (fri/oracle.rs) ----------------------------------------------------------
 * glp_batch_from_values  = PolynomialBatch::from_values  (ifft, lde x 2^rate_bits on the coset 7*H,
 *                          transpose + bit-reverse, MerkleTree::new(leaves, cap_height))
 * glp_batch_from_coeffs  = PolynomialBatch::from_coeffs
 * Input layout: column-major [ncols][n], n = 2^log_n, natural order.  No blinding (the salted form is
 * glp_batch_from_values_salted below).
 * The *_device variants take a device pointer on the ctx's GPU (input already resident in HBM).
 * A word >= p: the host entry points (these, the *_h and the salted one) refuse it naming column and index; the *_device ones reduce it
 * as it is loaded, and the coefficients a from_coeffs batch keeps (glp_batch_coeffs) are the reduced ones. */
GLP_API int glp_batch_from_values(glp_ctx *ctx, const uint64_t *values, uint32_t ncols, uint32_t log_n,
                          uint32_t rate_bits, uint32_t cap_height, glp_batch **out);
GLP_API int glp_batch_from_values_device(glp_ctx *ctx, const uint64_t *dev_values, uint32_t ncols, uint32_t log_n,
                                 uint32_t rate_bits, uint32_t cap_height, glp_batch **out);
GLP_API int glp_batch_from_coeffs(glp_ctx *ctx, const uint64_t *coeffs, uint32_t ncols, uint32_t log_n,
                          uint32_t rate_bits, uint32_t cap_height, glp_batch **out);
GLP_API int glp_batch_from_coeffs_device(glp_ctx *ctx, const uint64_t *dev_coeffs, uint32_t ncols, uint32_t log_n,
                                 uint32_t rate_bits, uint32_t cap_height, glp_batch **out);
/* The hash of the commitment: plonky2's `GenericConfig::Hasher`.  GLP_HASH_POSEIDON = PoseidonGoldilocksConfig (every driver of the
 * reference but one); GLP_HASH_KECCAK25 = KeccakGoldilocksConfig, `KeccakHash<25>` [REF src/hash/keccak256.rs:281]: Keccak-256
 * truncated to 25 bytes; such a digest occupies the same 4-word slot as a Poseidon HashOut (little-endian bytes, top 7 bytes of the
 * last word zero), so caps, paths and digest arrays keep their shapes.  The *_h entry points are the ones above with the hash named. */
GLP_API int glp_batch_from_values_h(glp_ctx *ctx, const uint64_t *values, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
                                    uint32_t cap_height, uint32_t hasher, glp_batch **out);
/* ---- salted (blinded) commitments: zero-knowledge proving --------------------------------------------------------------
 * plonky2 `PolynomialBatch::from_values(.., blinding = true)` (fri/oracle.rs, recalled from plonky2 0.1.x, unpinned): the LDE gets
 * SALT_SIZE = 4 extra columns of random values, one value per LDE point, after the polynomial columns; Merkle leaf j is
 * (ncols polynomial values, s0, s1, s2, s3) and its hash covers all of it.  The salts have no coefficients: they are never opened.
 * This library derives them from a keyed PRF, one Poseidon permutation per leaf (plonky2 draws them from the OS RNG; a salt only has
 * to be unpredictable, so a proof made here is a valid plonky2 proof):
 *     salt(seed, tag, leaf)[0..4) = the first four outputs of
 *         Poseidon([seed0, seed1, seed2, seed3 + k mod p, tag, leaf & 0xffffffff, leaf >> 32, 0, 0, 0, 0, 0])
 * leaf = the Merkle leaf index (merkle_tree.leaves[leaf], not the LDE point), k = the proof's index in a glp_prove_batch call (0
 * otherwise), tag = GLP_SALT_TAG_* below.  Seed words are taken mod p. */
#define GLP_SALT_SIZE 4
#define GLP_SALT_TAG_WIRES 0           /* wires_commitment */
#define GLP_SALT_TAG_ZS 1              /* partial_products_and_zs_commitment */
#define GLP_SALT_TAG_QUOTIENT 2        /* quotient_polys_commitment */
#define GLP_SALT_TAG_BATCH 3           /* glp_batch_from_values_salted */
#define GLP_SALT_TAG_WITNESS 4         /* the random cells of a witness plan (glp_witness_plan_create_rand) */
/* The same PRF gives the random cells of a generated witness (the advice of the blinding rows; "witness generation, the dataflow half",
 * RANDOM CELLS).  For random cell number i in the caller's order, proof k of the glp_witness_generate call and the seed of that call:
 *     b = i >> 3, j = i & 7
 *     value = Poseidon([seed0, seed1, seed2, seed3 + k mod p, GLP_SALT_TAG_WITNESS, b & 0xffffffff, b >> 32, 0, 0, 0, 0, 0])[j]
 * One permutation yields the eight rate words; the four capacity words are never written anywhere.  The value is a canonical field
 * element. */
/* from_values with blinding = true under `hasher`, salts from `seed`.  glp_batch_leaf returns glp_batch_leaf_len() = ncols + 4 words
 * for such a batch; glp_batch_info / glp_batch_coeffs keep counting the ncols polynomials. */
GLP_API int glp_batch_from_values_salted(glp_ctx *ctx, const uint64_t *values, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
                                         uint32_t cap_height, uint32_t hasher, const uint64_t seed[4], glp_batch **out);
/* words of one Merkle leaf: ncols, or ncols + GLP_SALT_SIZE for a salted batch (0 for NULL) */
GLP_API uint32_t glp_batch_leaf_len(const glp_batch *b);
GLP_API int glp_batch_from_coeffs_h(glp_ctx *ctx, const uint64_t *coeffs, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
                                    uint32_t cap_height, uint32_t hasher, glp_batch **out);
/* Keccak-256 of `count` messages of `len` bytes each (msgs [count][len], digests_out [count][32]) on the GPU: the primitive under
 * GLP_HASH_KECCAK25, exposed so that it can be checked against the reference's (input, digest) pairs
 * [REF src/hash/keccak256.rs:196-212,256-277]. */
GLP_API int glp_keccak256(glp_ctx *ctx, const uint8_t *msgs, size_t count, size_t len, uint8_t *digests_out);
GLP_API void glp_batch_free(glp_batch *b);
GLP_API int glp_batch_info(const glp_batch *b, uint32_t *ncols, uint32_t *log_n, uint32_t *rate_bits, uint32_t *cap_height);
/* merkle_tree.cap: [2^cap_height][4] */
GLP_API int glp_batch_cap(const glp_batch *b, uint64_t *cap_out);
/* `polynomials[col].coeffs`, natural order, for cols [col_begin, col_begin + ncols) -> [ncols][n] */
GLP_API int glp_batch_coeffs(const glp_batch *b, uint32_t col_begin, uint32_t ncols, uint64_t *out);
/* merkle_tree.leaves[leaf_index] (= `MerkleTree::get`): the ncols LDE values of row bitrev(leaf_index) */
GLP_API int glp_batch_leaf(const glp_batch *b, uint64_t leaf_index, uint64_t *out /* [glp_batch_leaf_len(b)] */);
/* `MerkleTree::prove(leaf_index)`: (log_n + rate_bits - cap_height) sibling digests, bottom-up, [k][4] */
GLP_API int glp_batch_merkle_proof(const glp_batch *b, uint64_t leaf_index, uint64_t *siblings_out);
/* every digest bottom-up: level 0 (leaf digests, index = leaf index) ... cap level; count =
 * sum_{w = N, N/2, .., 2^cap_height} w.  For tests. */
GLP_API size_t glp_batch_num_digests(const glp_batch *b);
GLP_API int glp_batch_digests(const glp_batch *b, uint64_t *out);

/* ---- many-proof batches: num_proofs PolynomialBatches of one shape, built and held as one object ---------------------------------
 * The commitments of num_proofs proofs of one circuit that advance in lock step (glp_fri_begin_many below): one transform and one
 * Merkle launch over all of them instead of num_proofs glp_batch_from_* calls.
 *   values / coeffs  [num_proofs][ncols][n], natural order; host memory, or (*_on_device != 0) an HBM pointer on the ctx's GPU.
 *                    A word >= p: host: refused naming proof, column and index; device: reduced as it is loaded
 *   seed             NULL: no blinding.  Else 4 words: member k is salted with (seed0, seed1, seed2, seed3 + k) and tag
 *                    GLP_SALT_TAG_BATCH, the rule of glp_prove_batch: member k is word for word
 *                    glp_batch_from_values_salted(member k's values, .., {seed0, seed1, seed2, seed3 + k})
 *   num_proofs       1..4096, and num_proofs * ncols * 2^(log_n + rate_bits) words at most 64 GiB (the cap of glp_prove_batch)
 * glp_batch_info and glp_batch_leaf_len describe one member.  The accessors that read ONE tree (glp_batch_cap, _coeffs, _leaf,
 * _merkle_proof, _digests) answer GLP_ERR_ARG for a batch of more than one member: take a member first. */
GLP_API int glp_batch_many_from_values(glp_ctx *ctx, const uint64_t *values, int values_on_device, uint32_t num_proofs, uint32_t ncols,
                                       uint32_t log_n, uint32_t rate_bits, uint32_t cap_height, uint32_t hasher, const uint64_t *seed,
                                       glp_batch **out);
GLP_API int glp_batch_many_from_coeffs(glp_ctx *ctx, const uint64_t *coeffs, int coeffs_on_device, uint32_t num_proofs, uint32_t ncols,
                                       uint32_t log_n, uint32_t rate_bits, uint32_t cap_height, uint32_t hasher, const uint64_t *seed,
                                       glp_batch **out);
/* members of the batch: 1 for every glp_batch_from_* batch (0 for NULL) */
GLP_API uint32_t glp_batch_num_proofs(const glp_batch *b);
/* Member k as a batch of its own: a BORROWED view whose device pointers point into b.  Valid until b is freed; released with
 * glp_batch_free, which frees no device memory for a view.  Every accessor above and glp_fri_begin / glp_fri_prove take it. */
GLP_API int glp_batch_member(const glp_batch *b, uint32_t k, glp_batch **view_out);
/* every member's merkle_tree.cap in one copy: [num_proofs][2^cap_height][4] */
GLP_API int glp_batch_caps(const glp_batch *b, uint64_t *caps_out);

/* ---- the caller's quotient at the commitment seam ------------------------------------------------------------------------------
 * An integrator that keeps its own quotient (see the next block) computes it from the committed oracles' values on the coset
 * g <W_M>, g = 7, M = 2^(log_n + sub_bits), W_M = primitive_root_of_unity(log_n + sub_bits), sub_bits = plonky2's
 * quotient_degree_bits <= rate_bits, and commits what comes out.  With the batches in HBM these three calls are both ends:
 *   glp_batch_lde_values         `PolynomialBatch::get_lde_values(i, step)` / `get_lde_values_packed`, for whole row windows
 *   glp_coset_ifft               `PolynomialValues::coset_ifft(shift)`
 *   glp_batch_from_coset_values  the tail of `prove_with_partition_witness`: `coset_ifft(g)`, `quotient_poly.chunks(degree)`,
 *                                `PolynomialBatch::from_coeffs`
 *
 * glp_batch_lde_values: the value for (i, c), i in [row_begin, row_begin + num_rows) inside [0, M), c < num_cols, is
 * p_{col_begin + c}(g * W_M^i) = word col_begin + c of glp_batch_leaf(b, bitrev(i * step)), step = 2^(rate_bits - sub_bits):
 * row i is the slice `get_lde_values(i, step)` returns.  Salts are never returned: the column range is held to the ncols
 * polynomials, as in glp_batch_coeffs.  The row window lets a CPU quotient stream row blocks instead of holding M x ncols words.
 *   layout         GLP_LDE_ROW_MAJOR: out[i - row_begin][c];  GLP_LDE_COL_MAJOR: out[c][i - row_begin]
 *   out_on_device  0: out is host memory and the call returns after the copy.  Else out is an HBM pointer on the batch's context
 *                  (a caller whose quotient is its own kernel) and the call is asynchronous on the ctx stream.
 * Unlike the one-tree accessors it also takes a many-proof batch: out gets a leading [num_proofs], the same window for every
 * member, in one launch.  A glp_batch_member view is the case of one member.
 * Errors: GLP_ERR_ARG naming the field for a null pointer, num_cols or num_rows of 0, a column range past ncols, sub_bits >
 * rate_bits, a row window past M, an unknown layout. */
#define GLP_LDE_ROW_MAJOR 0u   /* out[i - row_begin][c]: row i is the slice get_lde_values(i, step) returns */
#define GLP_LDE_COL_MAJOR 1u   /* out[c][i - row_begin] */
GLP_API int glp_batch_lde_values(const glp_batch *b, uint32_t col_begin, uint32_t num_cols, uint32_t sub_bits,
                                 uint64_t row_begin, uint64_t num_rows, uint32_t layout,
                                 uint64_t *out, int out_on_device);
/* `PolynomialValues::coset_ifft(shift)` in place on host memory, cols [ncols][2^log_n]: natural-order values on shift * <w> in,
 * natural-order coefficients out.  The shape of glp_fft / glp_ifft, and the inverse of glp_lde with rate_bits = 0.  shift must be a
 * non-zero canonical field element (GLP_ERR_ARG otherwise); a word >= p in cols: refused, cols unchanged. */
GLP_API int glp_coset_ifft(glp_ctx *ctx, uint64_t *cols, uint32_t ncols, uint32_t log_n, uint64_t shift);
/* values [num_proofs][num_polys][M], natural order on g <W_M> (the transposed `quotient_values` of `compute_quotient_polys`); host
 * memory, or (values_on_device != 0) an HBM pointer on the ctx's GPU.  Per polynomial `coset_ifft(g)` gives M coefficients, split
 * into 2^sub_bits chunks of n (`trim_to_len(quotient_degree)` is a no-op: M is the quotient degree).  The result is a batch of
 * num_polys << sub_bits polynomials, column p * 2^sub_bits + j = chunk j of polynomial p (the order of
 * `quotient_poly.chunks(degree)`), committed as `PolynomialBatch::from_coeffs(.., rate_bits, blinding = (seed != NULL),
 * cap_height)` under `hasher`: word for word glp_batch_many_from_coeffs on those chunks with the same seed (tag
 * GLP_SALT_TAG_BATCH, member k salted with seed3 + k), and glp_batch_from_coeffs_h at num_proofs == 1 without a seed.
 * num_proofs and the size bounds are those of glp_batch_many_from_coeffs; sub_bits in 0..rate_bits (0: one chunk, a plain coset
 * iFFT).  Every accessor, glp_batch_member, glp_fri_begin* and glp_batch_lde_values take the result like any other batch.
 * A value >= p: host: refused naming proof, column (the polynomial) and index; device: reduced as it is loaded. */
GLP_API int glp_batch_from_coset_values(glp_ctx *ctx, const uint64_t *values, int values_on_device, uint32_t num_proofs,
                                        uint32_t num_polys, uint32_t log_n, uint32_t sub_bits, uint32_t rate_bits,
                                        uint32_t cap_height, uint32_t hasher, const uint64_t *seed, glp_batch **out);

/* ---- the permutation argument at the commitment seam ----------------------------------------------------------------------------
 * Two steps of `prove_with_partition_witness` that are the same for every plonky2 circuit, whatever its gates, for the integrator of
 * the blocks around this one (no glp_circuit exists for its circuit): Z and the partial products
 * (`wires_permutation_partial_products_and_zs`, committed as plonk_zs_partial_products) and the permutation terms of the vanishing
 * polynomial on the quotient's coset.  With them the caller's own quotient code evaluates its gate constraints only.
 * glp_perm_desc is the part of CommonCircuitData these steps read.  Challenges are host arrays [num_proofs][num_challenges],
 * canonical; `*_on_device` != 0 marks an HBM pointer on the context's GPU; num_proofs is 1..4096 and every array gets a leading
 * [num_proofs] (one proof is num_proofs = 1).  Every refusal is GLP_ERR_ARG, names the field and happens before any launch. */
typedef struct {
    uint32_t log_n;
    uint32_t num_wires;          /* columns of the wires oracle; the routed ones come first */
    uint32_t num_routed_wires;   /* 1..num_wires */
    uint32_t num_challenges;     /* 1..4 */
    uint32_t chunk_size;         /* plonky2's quotient_degree_factor: routed wires per partial-product chunk, >= 1;
                                    num_partial_products = ceil(num_routed_wires / chunk_size) - 1, last chunk may be short */
    const uint64_t *k_is;        /* [num_routed_wires] coset shifts, canonical */
} glp_perm_desc;
/* num_challenges * (1 + num_partial_products): the polynomials of plonk_zs_partial_products; 0 for a refused description */
GLP_API uint32_t glp_perm_num_polys(const glp_perm_desc *desc);
/* Z and the partial products of num_proofs witnesses on H, committed: a batch of num_proofs members of glp_perm_num_polys columns
 * each, in the layout of `all_wires_permutation_partial_products` (the Z of every challenge first, then each challenge's partial
 * products).  Word for word glp_batch_many_from_values(those values, .., seed): seed NULL = no blinding, else member k is salted with
 * (seed0, seed1, seed2, seed3 + k) and tag GLP_SALT_TAG_BATCH; at num_proofs == 1 without a seed it is glp_batch_from_values_h.  For a
 * circuit the library can prove, the result's cap is what glp_session_partial_products returns.  A zero denominator (probability about
 * n * num_routed_wires * 2^-64) is not detected, as in the session.
 *   wires    [num_proofs][num_wires][n] values on H      sigmas   [num_routed_wires][n] values on H, shared by all proofs
 *            a word >= p of either: host: refused by name; device: reduced as it is loaded
 * Size bounds, log_n, rate_bits, cap_height and hasher: those of glp_batch_many_from_values. */
GLP_API int glp_perm_zs_commit(glp_ctx *ctx, const glp_perm_desc *desc, uint32_t num_proofs,
                               const uint64_t *wires, int wires_on_device, const uint64_t *sigmas, int sigmas_on_device,
                               const uint64_t *betas, const uint64_t *gammas,
                               uint32_t rate_bits, uint32_t cap_height, uint32_t hasher, const uint64_t *seed, glp_batch **out);
/* With M = 2^(log_n + sub_bits), S = 2^sub_bits, x_i = g W_M^i (the coset of glp_batch_lde_values) and T = num_challenges *
 * (num_partial_products + 2) permutation terms, for proof k and challenge c:
 *     out[k][c][i] = ( sum_{t < T} alpha_{k,c}^t term_t(x_i)  +  alpha_{k,c}^T gate_sums[k][c][i] ) / Z_H(x_i)
 * The terms in plonky2's order (`eval_vanishing_poly_base_batch`): L_0(x) (Z_j(x) - 1) for j < num_challenges; then per challenge j
 * and chunk  prev prod(w + beta_j k x + gamma_j) - next prod(w + beta_j sigma + gamma_j),  Z "next" being row (i + S) mod M.
 *   sigmas_oracle   columns [sigma_col_begin, sigma_col_begin + num_routed_wires) are the sigmas (plonky2 keeps them after the
 *                   constants); one member, shared by all proofs, or num_proofs members
 *   wires_oracle    at least num_wires polynomials;  zs_oracle: glp_perm_num_polys polynomials (glp_perm_zs_commit's result);
 *                   num_proofs members each (a glp_batch_member view is a batch of one).  Salted or not, each.
 *   gate_sums       NULL, or [num_proofs][num_challenges][M]: the caller's sum_t alpha^t (filtered gate constraint t), natural order on
 *                   the same coset.  With NULL the second summand is absent; the map is linear, so a caller may add its share afterwards.
 *                   A word >= p: host: refused naming proof, column (the challenge) and index; device: reduced as it is loaded.
 *   out             [num_proofs][num_challenges][M]: what glp_batch_from_coset_values takes with num_polys = num_challenges.  Host
 *                   memory: the call returns after the copy; an HBM pointer: nothing is copied back.
 * Refused beyond the common rules: sub_bits > rate_bits; chunk_size > 2^sub_bits (the chunk check would exceed the quotient's
 * degree); oracles that disagree in log_n (with desc and each other), rate_bits or ctx; wires_oracle with fewer than num_wires
 * polynomials; zs_oracle whose polynomial count is not glp_perm_num_polys; a sigma range past its oracle's polynomials (salts are not
 * polynomials); a member count that is neither num_proofs nor, for the sigmas only, 1. */
GLP_API int glp_perm_quotient_values(glp_ctx *ctx, const glp_perm_desc *desc, uint32_t num_proofs,
                                     const glp_batch *sigmas_oracle, uint32_t sigma_col_begin,
                                     const glp_batch *wires_oracle, const glp_batch *zs_oracle, uint32_t sub_bits,
                                     const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                                     const uint64_t *gate_sums, int gate_sums_on_device, uint64_t *out, int out_on_device);

/* ---- caller-defined gate constraints at the commitment seam: gate programs --------------------------------------------------------
 * The one step of `prove_with_partition_witness` the blocks above leave to the caller is the gate share of the vanishing polynomial,
 * glp_perm_quotient_values' gate_sums.  A gate program states it as a straight-line register machine over F_p (no branches, no loops)
 * that the library runs on every point x_i = g W_M^i of the quotient's coset, so the trace never leaves HBM.  The interpreter knows
 * nothing about selectors or gate types: a plonky2 selector filter is ordinary SUB / MUL instructions ending in END, an AIR is one
 * gate closed by END IMM(1).
 *
 * One instruction is one 64-bit word (bit 63 is zero):
 *     bits  3..0   opcode GLP_GP_OP_*          bits  8..4   dst register (ADD, SUB, MUL, MOV; else 0)
 *     bits 35..9   operand a                   bits 62..36  operand b (ADD, SUB, MUL; else 0)
 * An operand is 27 bits: kind GLP_GP_* in its bits 2..0, a payload in its bits 26..3:
 *     GLP_GP_REG       register r < num_regs (it must have been written by an earlier instruction)
 *     GLP_GP_COL       polynomial c (payload bits 21..0) of oracle o (payload bits 23..22) at x_i
 *     GLP_GP_COL_NEXT  the same polynomial at w_n x_i: natural row (i + S) mod M, S = 2^sub_bits (AIR transition constraints)
 *     GLP_GP_IMM       word j of the constant pool (canonical, shared by all proofs)
 *     GLP_GP_PARAM     word j of params[proof][num_params] (per-proof values such as the public-input hash)
 *     GLP_GP_X         x_i itself (payload 0)
 * Operations, every result canonical:
 *     ADD / SUB / MUL dst, a, b     field operations          MOV dst, a
 *     EMIT a    constraint t of the current gate: acc_c += a * alpha_c^t for every challenge c, then t += 1
 *     END a     closes the gate with filter value a: total_c += reduce(acc_c) * a, acc_c = 0, t = 0
 * and the result for proof k, challenge c, point i is total_c = sum_gates filter_g sum_t alpha_{k,c}^t v_{g,t}(x_i). */
#define GLP_GP_MAX_REGS 24u
#define GLP_GP_MAX_INSTRUCTIONS 65536u
#define GLP_GP_MAX_CONSTRAINTS 4096u   /* EMITs between two ENDs */
#define GLP_GP_MAX_ORACLES 4u
#define GLP_GP_OP_ADD 1u
#define GLP_GP_OP_SUB 2u
#define GLP_GP_OP_MUL 3u
#define GLP_GP_OP_MOV 4u
#define GLP_GP_OP_EMIT 5u
#define GLP_GP_OP_END 6u
#define GLP_GP_REG 0u
#define GLP_GP_COL 1u
#define GLP_GP_COL_NEXT 2u
#define GLP_GP_IMM 3u
#define GLP_GP_PARAM 4u
#define GLP_GP_X 5u
#define GLP_GP_DST_SHIFT 4
#define GLP_GP_A_SHIFT 9
#define GLP_GP_B_SHIFT 36
#define GLP_GP_OPERAND_BITS 27
#define GLP_GP_COL_ORACLE_SHIFT 22     /* inside the payload of GLP_GP_COL / GLP_GP_COL_NEXT */
#define GLP_GP_OPERAND(kind, payload) ((uint64_t)(kind) | ((uint64_t)(payload) << 3))
#define GLP_GP_COL_PAYLOAD(oracle, col) (((uint64_t)(oracle) << GLP_GP_COL_ORACLE_SHIFT) | (uint64_t)(col))
#define GLP_GP_INSTR(op, dst, a, b) \
    ((uint64_t)(op) | ((uint64_t)(dst) << GLP_GP_DST_SHIFT) | ((uint64_t)(a) << GLP_GP_A_SHIFT) | ((uint64_t)(b) << GLP_GP_B_SHIFT))

typedef struct glp_gate_program glp_gate_program;
typedef struct {
    const uint64_t *code;  uint32_t num_instructions;   /* 1..GLP_GP_MAX_INSTRUCTIONS, the last one END */
    const uint64_t *pool;  uint32_t num_pool;           /* canonical words; NULL with num_pool == 0 */
    uint32_t num_regs, num_params, num_oracles;         /* 1..GLP_GP_MAX_REGS; any; 1..GLP_GP_MAX_ORACLES */
    const uint32_t *oracle_cols;      /* [num_oracles]: polynomials the program may read of each */
} glp_gate_program_desc;
/* Host only, no context: GLP_OK and the largest number of EMITs in any one gate (the length of the alpha-power table), or
 * GLP_ERR_ARG with a message "instruction <index>, field <op | dst | a | b>: ..." for an unknown opcode or operand kind, a set bit
 * the opcode does not use, a register index >= num_regs, a register read before it is written, a pool, param or oracle index out of
 * range, a column index >= oracle_cols[o], more than GLP_GP_MAX_CONSTRAINTS EMITs in one gate, a last instruction that is not END;
 * and naming the description's field for a non-canonical pool word, num_regs of 0 or above GLP_GP_MAX_REGS, num_oracles outside
 * 1..GLP_GP_MAX_ORACLES, an empty program or one of more than GLP_GP_MAX_INSTRUCTIONS instructions. */
GLP_API int  glp_gate_program_check(const glp_gate_program_desc *d, uint32_t *max_constraints_out);
/* Checks the program as above and keeps a copy of it in HBM; the description's arrays may be freed afterwards. */
GLP_API int  glp_gate_program_create(glp_ctx *ctx, const glp_gate_program_desc *d, glp_gate_program **out);
GLP_API void glp_gate_program_free(glp_gate_program *p);
/* Runs the program on the coset g <W_M>, M = 2^(log_n + sub_bits), of num_proofs proofs (1..4096) in one launch.
 *   oracles   [num_oracles] committed batches of one log_n, rate_bits and ctx, oracle o with at least oracle_cols[o] polynomials and
 *             num_proofs members, or 1 member shared by all proofs.  Salted or not, each; salts are never read.
 *   alphas    [num_proofs][num_challenges], canonical, num_challenges in 1..4
 *   params    [num_proofs][num_params], canonical; NULL only with num_params == 0
 *   out       [num_proofs][num_challenges][M], natural order on g <W_M>: the layout and coset of glp_perm_quotient_values' gate_sums,
 *             so an HBM out (out_on_device != 0) is passed straight on with gate_sums_on_device = 1.  With host memory the call
 *             returns after the copy.
 * Refused beyond the common rules: sub_bits > rate_bits; oracles that disagree in log_n, rate_bits or ctx; an oracle with fewer
 * polynomials than oracle_cols[o]; a member count that is neither num_proofs nor 1; num_challenges outside 1..4; a non-canonical alpha
 * or param; params == NULL with num_params > 0.  Every refusal is GLP_ERR_ARG, names the field and happens before any launch. */
GLP_API int  glp_gate_program_sums(glp_ctx *ctx, const glp_gate_program *p, uint32_t num_proofs,
                                   const glp_batch *const *oracles, uint32_t sub_bits, uint32_t num_challenges,
                                   const uint64_t *alphas /* [num_proofs][num_challenges] */,
                                   const uint64_t *params /* [num_proofs][num_params] or NULL */,
                                   uint64_t *out, int out_on_device);

/* ---- the vanishing identity at zeta for caller-held circuits ------------------------------------------------------------------------
 * The verifier's side of the seam.  glp_fri_verify_many shows that the claimed openings are openings of the committed polynomials;
 * plonky2's `verify_with_challenges` first checks that they satisfy the circuit:
 *     vanishing(zeta) == Z_H(zeta) * reduce_with_powers(quotient chunks, zeta^n).
 * A gate program is straight-line code over F_p whose inputs are polynomials, so it evaluates at any point of F_p^2 (elements are two
 * canonical words a, b = a + b X, X^2 = 7): the program object made for the prover serves the verifier unchanged.  The reading is
 *     GLP_GP_COL       the opening of polynomial c of oracle o at the point         GLP_GP_COL_NEXT  its opening at w_n * point
 *     GLP_GP_X         the point itself            GLP_GP_IMM, GLP_GP_PARAM   base elements, embedded
 *     ADD / SUB / MUL  the F_p^2 operations (an extension-gate body traced over pairs of wires becomes plonky2's extension algebra
 *                      over F_p^2);  EMIT and END keep their meaning: alphas are base-field challenges, the accumulators F_p^2 elements.
 * Openings arrive through glp_ext_openings, which may point straight into the openings array of glp_fri_verify_many (the order of
 * glp_fri_open: for the plonk instance every polynomial of oracles 0..3 at zeta, then the first num_challenges polynomials of the zs
 * oracle at g zeta).  num_proofs is 1..4096 and every array gets a leading [num_proofs].  Host inputs (inputs_on_device == 0) are
 * scanned, and a word >= p is refused naming proof and word index; device inputs (HBM pointers on the context's GPU) are reduced mod p
 * once as they are loaded.  Canonical-form checking of proof bytes stays with glp_proof_from_bytes and glp_fri_verify*.  Every refusal
 * is GLP_ERR_ARG, names the field and happens before any launch. */
typedef struct {
    const uint64_t *at;        /* element (proof k, polynomial c) = at + k * proof_stride + 2 c, two words (F_p^2) */
    const uint64_t *at_next;   /* the same at w_n * point; NULL where nothing reads it */
    size_t proof_stride;       /* words between proofs, >= 2 * polynomials read (and at most 2^32) */
} glp_ext_openings;
/* The program at points[k] over the openings of num_proofs proofs, one launch: out[k][c] = sum_gates filter_g sum_t alpha_{k,c}^t v_{g,t},
 * the program's gate_sums at zeta.
 *   points    [num_proofs][2]                 openings  [num_oracles], oracle o with oracle_cols[o] polynomials; at_next is needed
 *                                                       only for an oracle one of whose COL_NEXT the program reads
 *   alphas    [num_proofs][num_challenges] and params [num_proofs][num_params] (NULL only with num_params == 0): host, canonical
 *   out       [num_proofs][num_challenges][2]; an HBM out (out_on_device != 0) is glp_perm_check_zeta's gate_sums as it stands
 * Refused: null pointers; num_proofs outside 1..4096 or num_challenges outside 1..4; proof_stride < 2 * oracle_cols[o]; at_next ==
 * NULL for an oracle whose COL_NEXT the program reads; a non-canonical alpha or param; params == NULL with num_params > 0; a
 * non-canonical host point or opening. */
GLP_API int  glp_gate_program_eval_ext(glp_ctx *ctx, const glp_gate_program *p, uint32_t num_proofs, uint32_t num_challenges,
                                       const uint64_t *points /* [K][2] */, const glp_ext_openings *openings /* [num_oracles] */,
                                       int inputs_on_device, const uint64_t *alphas /* [K][nch], host */,
                                       const uint64_t *params /* [K][num_params], host, or NULL */,
                                       uint64_t *out /* [K][nch][2] */, int out_on_device);
/* With n = 2^log_n and T = num_challenges * (num_partial_products + 2), checks for proof k and every challenge c
 *     sum_{t < T} alpha_{k,c}^t term_t(zeta_k) + alpha_{k,c}^T gate_sums[k][c] == (zeta_k^n - 1) sum_j quotient[c * chunks + j] zeta_k^(n j)
 * with the terms of the formula above glp_perm_quotient_values evaluated at zeta, L_0(zeta) = (zeta^n - 1) / (n (zeta - 1)) and Z "next"
 * zs.at_next: the algebra of glp_verify's identity check with the gate terms taken from the caller.
 *   sigmas, wires   num_routed_wires polynomials each are read (the routed wires come first)
 *   zs              glp_perm_num_polys polynomials at zeta; at_next: the first num_challenges at g zeta
 *   quotient        num_challenges * num_quotient_chunks polynomials, num_quotient_chunks in 1..256
 *   betas, gammas, alphas   host [num_proofs][num_challenges], canonical
 *   gate_sums       NULL (the gate term is absent), or [num_proofs][num_challenges][2]; with gate_sums_on_device != 0 the HBM out of
 *                   glp_gate_program_eval_ext passed straight on: nothing returns to the host between the two calls
 *   status_out      [num_proofs]: GLP_OK = the identity holds, GLP_ERR_PROVE = rejected (the convention of glp_fri_verify_many)
 *   reasons_out     NULL or [num_proofs][GLP_REASON_LEN], empty if accepted, else in glp_verify's words: "zeta = 1" or
 *                   "Mismatch between evaluation and opening of quotient polynomial (challenge <c>)", c the first such challenge
 * The call returns GLP_OK when it ran.  Refused: null pointers (at_next of zs included), num_proofs or num_quotient_chunks out of range,
 * a description glp_perm_num_polys refuses, a proof_stride below twice the polynomials read, non-canonical challenges or host inputs. */
GLP_API int  glp_perm_check_zeta(glp_ctx *ctx, const glp_perm_desc *desc, uint32_t num_proofs, uint32_t num_quotient_chunks,
                                 const uint64_t *zetas /* [K][2] */,
                                 const glp_ext_openings *sigmas, const glp_ext_openings *wires, const glp_ext_openings *zs,
                                 const glp_ext_openings *quotient, int inputs_on_device,
                                 const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas /* host [K][nch] */,
                                 const uint64_t *gate_sums /* NULL or [K][nch][2] */, int gate_sums_on_device,
                                 int32_t *status_out /* [K] */, char *reasons_out /* NULL or [K][GLP_REASON_LEN] */);

/* ---- caller-defined running arguments at the commitment seam: trace programs and running columns ------------------------------------
 * A lookup table, a logUp or cross-table argument and a custom permutation are all the same two steps over the witness: new columns
 * (numerators and denominators under a challenge) computed from committed ones on the rows of H, then helper columns h = num / den
 * and a running column Z over them.  The library recites nobody's lookup layout: the caller states its argument as a gate program,
 * and the witness never leaves HBM.  The pipeline is five calls:
 *     glp_gate_program_rows        numerators and denominators on H from the witness columns and a challenge (a PARAM)
 *     glp_running_columns          h_t = num_t / den_t and Z, with the totals that say whether the argument closes
 *     glp_batch_many_from_values   commits them (values_on_device = 1, ncols = num_args * (num_terms + 1))
 *     glp_gate_program_sums        the constraints over the committed h and Z -- h den - num, and Z(w x) - Z(x) - sum_t h_t(x) with
 *                                  GLP_GP_COL_NEXT -- on the quotient's coset
 *     then the quotient, FRI and zeta calls above, as for any caller-held circuit.
 * num_proofs is 1..4096 and every array gets a leading [num_proofs].  Host inputs (inputs_on_device == 0) are scanned, and a word
 * >= p is refused by name; device inputs (HBM pointers on the context's GPU) are reduced mod p once as they are loaded.  Every
 * refusal is GLP_ERR_ARG, names the field and happens before any launch.
 *
 * glp_gate_program_rows runs a program on the n = 2^log_n rows of H.  It is the third reading of a program object (the coset:
 * glp_gate_program_sums; F_p^2 at zeta: glp_gate_program_eval_ext); at row i of proof k
 *     GLP_GP_COL       column c of input o at row i               GLP_GP_COL_NEXT  the same column at row (i + 1) mod n
 *     GLP_GP_X         w_n^i                                      GLP_GP_IMM, GLP_GP_PARAM, ADD / SUB / MUL / MOV   as before
 *     EMIT a           number t, counted from the start of the program: out[k][t][i] = a
 * The program must be a single gate: exactly one END, its last instruction, whose operand is a GLP_GP_IMM with the pool word 1 (the
 * AIR shape "closed by END IMM(1)"), and at least one EMIT.  Any other shape is refused naming the instruction and the field.
 *   inputs          [num_oracles] arrays [members][oracle_cols[o]][n], values on H in natural order: the layout of glp_perm_zs_commit's
 *                   wires and of glp_batch_many_from_values (a batch holds coefficients and the LDE on g H, not values on H)
 *   input_members   [num_oracles]: num_proofs, or 1 for an input shared by all proofs (a table, say)
 *   params          [num_proofs][num_params], host, canonical; NULL only with num_params == 0
 *   out             [num_proofs][num_out][n], num_out = the max_constraints glp_gate_program_check reports.  With host memory the call
 *                   returns after the copy; with an HBM pointer nothing is copied back and the call is asynchronous.
 * Refused: null pointers; num_proofs outside 1..4096; log_n above the largest batch's; input_members[o] neither 1 nor num_proofs;
 * more than 64 GiB of inputs or of out; params == NULL with num_params > 0; a non-canonical param; a non-canonical host input word,
 * naming the input and the word index. */
GLP_API int  glp_gate_program_rows(glp_ctx *ctx, const glp_gate_program *p, uint32_t num_proofs, uint32_t log_n,
                                   const uint64_t *const *inputs /* [num_oracles] */,
                                   const uint32_t *input_members /* [num_oracles]: 1 or num_proofs */, int inputs_on_device,
                                   const uint64_t *params /* [K][num_params] or NULL */,
                                   uint64_t *out /* [K][num_out][n] */, int out_on_device);
/* The helper columns and the running column of num_args arguments of num_terms terms each, for num_proofs proofs, with K = num_proofs,
 * A = num_args, T = num_terms, n = 2^log_n:
 *     out[k][a][t][i] = nums(k, a, t, i) / dens(k, a, t, i)    for t < T
 *     out[k][a][T][i] = Z[i]:    Z[0] = 0, Z[i + 1] = Z[i] + sum_t out[k][a][t][i]     (GLP_RUN_SUM, logUp)
 *                                Z[0] = 1, Z[i + 1] = Z[i] * prod_t out[k][a][t][i]    (GLP_RUN_PRODUCT, grand product)
 *     totals_out[k][a] = the value Z would take at row n: Z[n - 1] combined with row n - 1's contribution.
 * A closed argument has total 0 (sum) or 1 (product); cross-table arguments compare totals across calls.
 *   nums, dens        element (k, a, t, i) at k * in_proof_stride + (a T + t) n + i; nums == NULL means every numerator is 1.  The
 *                     stride (>= A T n, at most 2^33) lets a rows program that EMITs all denominators and then all numerators be
 *                     passed straight on: dens = rows_out, nums = rows_out + A T n, in_proof_stride = 2 A T n, no copy.  Neither
 *                     may overlap out.
 *   out               [K][A (T + 1)][n], contiguous: what glp_batch_many_from_values(.., values_on_device = 1, ..) takes with
 *                     ncols = A (T + 1)
 *   totals_out        host [K][A], required: the call is synchronous
 * A zero denominator is GLP_ERR_PROVE, its message naming proof, argument, term and row of the first one in (k, a, t, i) order;
 * out and totals_out are unspecified then.  (Inversion is batched over a row's terms; a zero is kept out of the batch, so it
 * spoils no other term's value before it is reported.)
 * Refused: null ctx, dens, out or totals_out; kind not one of GLP_RUN_*; num_proofs outside 1..4096, num_args outside 1..16,
 * num_terms outside 1..64; log_n above the largest batch's; more than 64 GiB of out; in_proof_stride below A T n or above 2^33; a
 * non-canonical host word of nums or dens, naming the array, the proof and the word index. */
#define GLP_RUN_SUM 0u       /* logUp:          Z[0] = 0, Z[i+1] = Z[i] + sum_t h_t[i] */
#define GLP_RUN_PRODUCT 1u   /* grand product:  Z[0] = 1, Z[i+1] = Z[i] * prod_t h_t[i] */
GLP_API int  glp_running_columns(glp_ctx *ctx, uint32_t kind, uint32_t num_proofs, uint32_t num_args, uint32_t num_terms,
                                 uint32_t log_n, const uint64_t *nums /* NULL = all ones */, const uint64_t *dens,
                                 size_t in_proof_stride, int inputs_on_device,
                                 uint64_t *out /* [K][num_args][num_terms + 1][n] */, int out_on_device,
                                 uint64_t *totals_out /* host [K][num_args] */);

/* ---- openings and FRI of caller-held batches (fri/oracle.rs `PolynomialBatch::prove_openings`) ----------------------------------
 * For an integrator that keeps its own quotient (circuits with lookup tables, Poseidon2Gate, custom gates, starky AIRs: anything
 * glp_circuit_create answers with GLP_ERR_UNSUPPORTED): commit with glp_batch_from_values / _from_coeffs, evaluate the committed
 * polynomials at the opening points and run FRI over them here.  glp_fri_desc is plonky2's `FriInstanceInfo` plus the `FriParams`
 * the prover reads.  A point names its polynomials in the order of its ranges; that order is the order of the alpha powers and of
 * the openings.  With F = 0, for each point b in order (plonky2's combination rule, the coefficient-form `divide_by_linear`):
 *     F <- alpha^(len_b) F + (sum_j alpha^j p_{b,j}(X) - sum_j alpha^j p_{b,j}(z_b)) / (X - z_b),   j over that point's polynomials.
 * Many proofs of one instance in lock step, over many-proof batches: glp_fri_begin_many / glp_fri_prove_many below; glp_fri_begin and
 * glp_fri_prove answer GLP_ERR_UNSUPPORTED for a batch of more than one member (a glp_batch_member view is a batch of one). */
#define GLP_FRI_MAX_ORACLES 8
#define GLP_REASON_LEN 160     /* chars of one rejection reason (glp_verify_batch, glp_fri_verify*) */
#define GLP_FRI_MAX_POINTS 4
#define GLP_FRI_MAX_RANGES 16     /* per point */
typedef struct { uint32_t oracle, col_begin, num_cols; } glp_fri_range;      /* polynomials [col_begin, col_begin+num_cols) of oracles[oracle] */
typedef struct { uint64_t point[2]; uint32_t num_ranges; const glp_fri_range *ranges; } glp_fri_point;   /* plonky2 FriBatchInfo */
typedef struct {
    uint32_t num_oracles;  const glp_batch *const *oracles;   /* FriInstanceInfo.oracles: same ctx, log_n, rate_bits, cap_height, hasher; salted or not, each */
    uint32_t num_points;   const glp_fri_point *points;       /* FriInstanceInfo.batches, in order */
    uint32_t num_reductions, reduction_arity_bits[16];
    uint32_t proof_of_work_bits, num_query_rounds;
} glp_fri_desc;
typedef struct glp_fri glp_fri;
/* Stepped form: mirrors glp_session_* from `open` onward (order enforced; GLP_ERR_ARG otherwise):
 *
 *   glp_fri_begin        validates and copies the description; the batches are borrowed and must outlive the handle
 *   glp_fri_open         out: 2 words per (point, polynomial), points in order: `PolynomialCoeffs::to_extension().eval(point)`, what the
 *                        Rust prover computes for its `OpeningSet`
 *   glp_fri_combine      in: FRI alpha (ext)
 *   num_reductions x { glp_fri_commit (out: layer cap [2^cap_height][4]) ; glp_fri_fold (in: beta, ext) }
 *   glp_fri_final_poly   out: final polynomial coefficients (ext), glp_fri_final_poly_len of them
 *   glp_pow_search_h     (stateless) the proof-of-work witness on the caller's sponge
 *   glp_fri_queries      in: pow witness, num_query_rounds indices in [0, 2^(log_n + rate_bits))
 *   glp_fri_proof        out: plonky2's `FriProof`, glp_fri_proof_words words, laid out as the tail of glp_prove's proof:
 *                          commit_phase_merkle_caps [num_reductions][2^cap_height][4]
 *                          query_round_proofs [num_query_rounds]: per oracle (leaf: glp_batch_leaf_len words, salts last; Merkle path),
 *                                                                 then per reduction (evals, Merkle path)
 *                          final_poly | pow_witness
 *   glp_fri_end
 *
 * glp_fri_begin errors: GLP_ERR_ARG with a message naming the field for a null pointer or a count out of range (num_oracles,
 * num_points, num_ranges, num_reductions); oracles that disagree in log_n, rate_bits, cap_height, hasher or ctx; a range past its
 * oracle's ncols (the salts are not polynomials); a point with no polynomial; arity bits that sum above log_n or any arity bit
 * outside 1..4; num_query_rounds = 0.  GLP_ERR_PROVE for a point that lies on the coset g H (b = 0 and a^n = g^n), as the session
 * answers zeta in the subgroup. */
GLP_API int glp_fri_begin(glp_ctx *ctx, const glp_fri_desc *desc, glp_fri **out);
GLP_API size_t glp_fri_num_openings(const glp_fri *f);
GLP_API int glp_fri_open(glp_fri *f, uint64_t *openings_out /* [2 * glp_fri_num_openings] */);
GLP_API int glp_fri_combine(glp_fri *f, const uint64_t alpha[2]);
GLP_API int glp_fri_commit(glp_fri *f, uint64_t *cap_out);
GLP_API int glp_fri_fold(glp_fri *f, const uint64_t beta[2]);
GLP_API size_t glp_fri_final_poly_len(const glp_fri *f);                /* ext coefficients */
GLP_API int glp_fri_final_poly(glp_fri *f, uint64_t *coeffs_out /* [2 * glp_fri_final_poly_len] */);
GLP_API int glp_fri_queries(glp_fri *f, uint64_t pow_witness, const uint64_t *indices, uint32_t num_indices);
GLP_API size_t glp_fri_proof_words(const glp_fri *f);
GLP_API int glp_fri_proof(glp_fri *f, uint64_t *proof_out /* [glp_fri_proof_words] */);
GLP_API void glp_fri_end(glp_fri *f);
/* One-call form: the same sequence driven by the library's transcript, resumed from a duplex-sponge state plus num_pending (< 8)
 * buffered inputs (the convention of glp_pow_search_h).  The caller has just observed the openings, so its output buffer is empty --
 * or, with num_pending = 0, holds the state's 8 rate words: the last observation filled the rate and permuted, and plonky2's
 * `duplexing` refills the output buffer; the library resumes either way from (state, num_pending) alone.  The permutation is that of
 * the batches' hasher.  Order (fri/prover.rs): alpha; per reduction observe the cap, draw beta; observe
 * the final polynomial; the SMALLEST proof-of-work witness; num_query_rounds indices, get() % N.  openings_out
 * [2 * sum of the points' polynomial counts] is filled for the caller's proof (they are computed inside the call anyway).
 * sponge_state and pending_inputs are field elements: a word >= p is GLP_ERR_ARG naming it, decided before any launch. */
GLP_API int glp_fri_prove(glp_ctx *ctx, const glp_fri_desc *desc, const uint64_t sponge_state[12], const uint64_t *pending_inputs,
                          uint32_t num_pending, uint64_t *openings_out, uint64_t *proof_out);

/* ---- the same for num_proofs proofs of ONE instance in lock step ------------------------------------------------------------------
 * What glp_prove_batch is to glp_prove, for circuits whose quotient stays with the caller: small proofs are bound by launch and host
 * round-trip latency when proved one by one; here every step is a fixed number of launches over all proofs and one copy to or from
 * the host.  desc is the description of one proof: ranges, arities, proof-of-work bits and query count are shared; desc->points[].point
 * is ignored, proof k opens at points[k][0 .. num_points) (every proof has its own zeta).  Each oracle is either per proof
 * (glp_batch_num_proofs == num_proofs: glp_batch_many_from_*) or shared by all proofs (a batch of one: preprocessed columns, as
 * constants_sigmas is in glp_prove_batch); for num_proofs > 1 at least one is per proof.
 * Errors beyond those of glp_fri_begin, all GLP_ERR_ARG naming the field unless said: num_proofs outside 1..4096; points null; an
 * oracle whose member count is neither 1 nor num_proofs; only shared oracles; points[k][p] not canonical; points[k][p] on the coset
 * g H is GLP_ERR_PROVE and names proof k.
 * The handle takes the step functions above with a leading [num_proofs] on every array:
 *   glp_fri_open         out: [num_proofs][glp_fri_num_openings][2]
 *   glp_fri_combine      in:  alphas [num_proofs][2]
 *   glp_fri_commit       out: [num_proofs][2^cap_height][4]          glp_fri_fold   in: betas [num_proofs][2]
 *   glp_fri_final_poly   out: [num_proofs][glp_fri_final_poly_len][2]
 *   glp_pow_search_many  (stateless) the num_proofs witnesses in one launch
 *   glp_fri_queries_many in:  pow_witnesses [num_proofs], indices [num_proofs][num_query_rounds]  (glp_fri_queries is GLP_ERR_ARG here)
 *   glp_fri_proof        out: [num_proofs][glp_fri_proof_words]
 * Proof k is word for word what glp_fri_prove returns for member k of every per-proof oracle (tests/test_gpu_fri_many.py). */
GLP_API int glp_fri_begin_many(glp_ctx *ctx, const glp_fri_desc *desc, uint32_t num_proofs, const uint64_t *points /* [num_proofs][num_points][2] */,
                               glp_fri **out);
GLP_API uint32_t glp_fri_num_proofs(const glp_fri *f);                  /* 1 for a glp_fri_begin handle */
GLP_API int glp_fri_queries_many(glp_fri *f, const uint64_t *pow_witnesses, const uint64_t *indices);
/* glp_pow_search_h for num_proofs sponges with num_pending (< 8) buffered inputs each: sponge_states [num_proofs][12], pending_inputs
 * [num_proofs][num_pending], witnesses_out [num_proofs], the smallest witness of each.  A state or pending word >= p is GLP_ERR_ARG
 * naming sponge_states[k][i] or pending_inputs[k][i], decided before any launch. */
GLP_API int glp_pow_search_many(glp_ctx *ctx, uint32_t hasher, uint32_t num_proofs, const uint64_t *sponge_states, const uint64_t *pending_inputs,
                                uint32_t num_pending, uint32_t bits, uint64_t *witnesses_out);
/* One-call form: glp_fri_prove's transcript order for each proof, the num_proofs transcripts on the context's host threads
 * (GLP_HOST_THREADS, as glp_prove_batch).  sponge_states [num_proofs][12], pending_inputs [num_proofs][num_pending], openings_out
 * [num_proofs][openings][2], proofs_out [num_proofs][FriProof words].  A state or pending word >= p is GLP_ERR_ARG, as for
 * glp_pow_search_many. */
GLP_API int glp_fri_prove_many(glp_ctx *ctx, const glp_fri_desc *desc, uint32_t num_proofs, const uint64_t *points, const uint64_t *sponge_states,
                               const uint64_t *pending_inputs, uint32_t num_pending, uint64_t *openings_out, uint64_t *proofs_out);

/* ---- verifying FRI proofs of caller-held instances (fri/verifier.rs `verify_fri_proof`) --------------------------------------------
 * The other half of glp_fri_*: num_proofs FriProofs of ONE instance checked in one device launch, for the circuits whose quotient stays
 * with the caller (no glp_circuit exists for them, so glp_verify_batch cannot take them).  The verifier holds no glp_batch, only caps,
 * so it has a description of its own; it mirrors glp_fri_desc field for field where the two overlap and obeys the same shape rules.
 *   glp_fri_oracle_shape  num_cols: polynomials of the oracle; salted != 0: a leaf carries GLP_SALT_SIZE salts after them (never
 *                         named by a range); shared != 0: one cap for all proofs, else one per proof
 *   points[].ranges       as in glp_fri_desc; points[].point is read only by glp_fri_verify
 * Arrays (host memory), K = num_proofs:
 *   points         [K][num_points][2]               proof k's opening points
 *   caps           [num_oracles] pointers: [2^cap_height][4] for a shared oracle, else [K][2^cap_height][4] (glp_batch_caps)
 *   openings       [K][glp_fri_verify_num_openings][2]   the claimed openings, order of glp_fri_open
 *   proofs         [K][glp_fri_verify_proof_words]  layout of glp_fri_proof
 *   status_out     [K]: GLP_OK = accepted, GLP_ERR_PROVE = rejected;   reasons_out  NULL or [K][GLP_REASON_LEN] (empty if accepted)
 * The return value is that of glp_verify_batch: GLP_OK whenever every proof could be judged, whatever the verdicts.  A reason names the
 * query round and the failed check and ends in "[check N]", N the stable number of the check (the return value of
 * tests/fri_restate.py::verify_fri_proof); the reported failure is the first failing check of the first failing query:
 *   1  a word that is not canonical (>= p; a KeccakHash<25> digest longer than 25 bytes) in proof, openings, caps or points
 *   2  proof of work                          3  a query point equal to an opening point (rejected, never divided by zero)
 *   4  an initial Merkle path                 5  a layer's evaluation disagrees with the previous fold
 *   6  a layer's Merkle path                  7  final polynomial
 * Per proof the canonical-form scan and the transcript run on the context's host threads (GLP_HOST_THREADS) beside the upload; every
 * query round of every proof is one launch over K x num_query_rounds 16-lane groups, as in glp_verify_batch.
 * GLP_ERR_ARG, naming the field: a count outside GLP_FRI_MAX_*; a range past num_cols; a point with no polynomial; arity bits outside
 * 1..4 or summing above log_n; num_query_rounds = 0; num_proofs outside 1..65536; a null pointer; num_pending >= 8; an unknown hasher;
 * (stepped form) an index >= 2^(log_n + rate_bits) or a challenge that is not canonical. */
typedef struct { uint32_t num_cols, salted, shared; } glp_fri_oracle_shape;
typedef struct {
    uint32_t num_oracles;  const glp_fri_oracle_shape *oracles;
    uint32_t log_n, rate_bits, cap_height, hasher;            /* what the prover's batches carry; hasher: GLP_HASH_* */
    uint32_t num_points;   const glp_fri_point *points;
    uint32_t num_reductions, reduction_arity_bits[16];
    uint32_t proof_of_work_bits, num_query_rounds;
} glp_fri_verify_desc;
/* == glp_fri_proof_words / glp_fri_num_openings of the matching prover handle; 0 for a description the verifier refuses */
GLP_API size_t glp_fri_verify_proof_words(const glp_fri_verify_desc *desc);
GLP_API size_t glp_fri_verify_num_openings(const glp_fri_verify_desc *desc);
/* One-call form: each proof's transcript resumes from (sponge_states[k], pending_inputs[k][num_pending]) exactly as glp_fri_prove's does
 * (with num_pending = 0 the output buffer is refilled from the state).  Order: alpha; per reduction observe the cap, draw beta; observe
 * the final polynomial; observe the witness; draw the response and check it against proof_of_work_bits; num_query_rounds indices,
 * get() % N.  sponge_states [K][12], pending_inputs [K][num_pending]. */
GLP_API int glp_fri_verify_many(glp_ctx *ctx, const glp_fri_verify_desc *desc, uint32_t num_proofs, const uint64_t *points,
                                const uint64_t *const *caps, const uint64_t *openings, const uint64_t *proofs, const uint64_t *sponge_states,
                                const uint64_t *pending_inputs, uint32_t num_pending, int32_t *status_out, char *reasons_out);
/* Stepped form, for a caller that keeps its own Fiat-Shamir: it drew alphas [K][2], betas [K][num_reductions][2] and indices
 * [K][num_query_rounds] and has checked the proof of work itself; the library does the canonical-form scan and every query check
 * (checks 1 and 3..7).  The reduced openings are computed on the device from the uploaded openings. */
GLP_API int glp_fri_verify_queries_many(glp_ctx *ctx, const glp_fri_verify_desc *desc, uint32_t num_proofs, const uint64_t *points,
                                        const uint64_t *const *caps, const uint64_t *openings, const uint64_t *proofs, const uint64_t *alphas,
                                        const uint64_t *betas, const uint64_t *indices, int32_t *status_out, char *reasons_out);
/* One proof at desc->points[].point (caps [num_oracles] pointers to [2^cap_height][4] whatever `shared` says): GLP_OK = accepted,
 * GLP_ERR_PROVE with the reason in glp_last_error() = rejected. */
GLP_API int glp_fri_verify(glp_ctx *ctx, const glp_fri_verify_desc *desc, const uint64_t *const *caps, const uint64_t *openings,
                           const uint64_t *proof, const uint64_t sponge_state[12], const uint64_t *pending_inputs, uint32_t num_pending);

/* ---- circuits and whole proofs ------------------------------------------------------------------
 * glp_circuit_desc carries the parts of plonky2's CommonCircuitData / ProverOnlyCircuitData /
 * VerifierOnlyCircuitData that `prove` reads (plonk/circuit_data.rs), i.e. what
 * `builder.build::<C>()` returns at [REF src/ecdsa/gadgets/ecdsa.rs:298].  Scope of this build:
 * no lookup tables, zero_knowledge = false unless asked for (glp_circuit_create_ex), quotient_degree_factor a power of two <= 2^rate_bits,
 * D = 2, Poseidon hashing (PoseidonGoldilocksConfig, the `type C` of every reference driver but
 * one [REF src/hash/keccak256.rs:281]).  Gate types a circuit may contain: see GLP_GATE_* (0..18 and 20..22; any other
 * type is GLP_ERR_UNSUPPORTED: the lookup gates, Poseidon2Gate -- unless it comes as GLP_GATE_PROGRAM through glp_circuit_create_prog). */
enum {
    GLP_GATE_NOOP = 0,             /* plonky2 gates/noop.rs */
    GLP_GATE_CONSTANT = 1,         /* gates/constant.rs, p0 = num_consts */
    GLP_GATE_PUBLIC_INPUT = 2,     /* gates/public_input.rs */
    GLP_GATE_ARITHMETIC = 3,       /* gates/arithmetic_base.rs, p0 = num_ops */
    GLP_GATE_POSEIDON = 4,         /* gates/poseidon.rs */
    GLP_GATE_U32_INTERLEAVE = 5,   /* [REF src/u32/gates/interleave_u32.rs:33-82,84-135], p0 = num_ops */
    GLP_GATE_UNINTERLEAVE_U32 = 6, /* [REF src/u32/gates/uninterleave_to_u32.rs:30-91,93-150], p0 = num_ops */
    GLP_GATE_UNINTERLEAVE_B32 = 7, /* [REF src/u32/gates/uninterleave_to_b32.rs:95-150], p0 = num_ops */
    /* the gate set of the secp256k1 circuit [REF src/ecdsa/gadgets/ecdsa.rs:72-96]; sources absent from the
     * reference (plonky2, plonky2_u32 @552acaec [REF Cargo.lock:1001-1009]), restated from the published crates */
    GLP_GATE_U32_ARITHMETIC = 8,   /* plonky2_u32 gates/arithmetic_u32.rs, p0 = num_ops */
    GLP_GATE_U32_ADD_MANY = 9,     /* plonky2_u32 gates/add_many_u32.rs, p0 = num_addends, p1 = num_ops */
    GLP_GATE_U32_SUBTRACTION = 10, /* plonky2_u32 gates/subtraction_u32.rs, p0 = num_ops */
    GLP_GATE_U32_RANGE_CHECK = 11, /* plonky2_u32 gates/range_check_u32.rs, p0 = num_input_limbs */
    GLP_GATE_COMPARISON = 12,      /* plonky2_u32 gates/comparison.rs, p0 = num_bits, p1 = num_chunks */
    GLP_GATE_BASE_SUM = 13,        /* plonky2 gates/base_sum.rs, p0 = num_limbs, p1 = base */
    GLP_GATE_RANDOM_ACCESS = 14,   /* plonky2 gates/random_access.rs, p0 = bits, p1 = num_copies | num_extra_constants << 16 */
    /* plonky2's extension-field arithmetic (D = 2: an F_p^2 value occupies two consecutive wires), what the builder emits for
     * every `*_extension` operation and for `reduce` / `reduce_ext` (recursion and aggregation circuits) */
    GLP_GATE_ARITHMETIC_EXTENSION = 15, /* gates/arithmetic_extension.rs, p0 = num_ops (>= 1) */
    GLP_GATE_MUL_EXTENSION = 16,        /* gates/multiplication_extension.rs, p0 = num_ops (>= 1) */
    GLP_GATE_REDUCING = 17,             /* gates/reducing.rs, p0 = num_coeffs (>= 1, 6 + num_coeffs <= num_routed_wires) */
    GLP_GATE_REDUCING_EXTENSION = 18,   /* gates/reducing_extension.rs, p0 = num_coeffs (>= 1, 6 + 2 num_coeffs <= num_routed_wires) */
    /* 19 is unassigned and stays GLP_ERR_UNSUPPORTED (callers probe it as "a type this build does not know") */
    /* the rest of the recursive verifier's gate set: exp_from_bits, the FRI fold step, Poseidon's linear layer on ext targets */
    GLP_GATE_EXPONENTIATION = 20,       /* gates/exponentiation.rs, p0 = num_power_bits (>= 1, p0 + 2 <= num_routed_wires) */
    GLP_GATE_COSET_INTERPOLATION = 21,  /* gates/coset_interpolation.rs, p0 = subgroup_bits (1..5), p1 = degree (2 <= p1 <= 2^p0) */
    GLP_GATE_POSEIDON_MDS = 22,         /* gates/poseidon_mds.rs, no parameters (48 wires, all routed) */
    /* a caller-defined gate: its constraints are program p0 of the list handed to glp_circuit_create_prog (GATE PROGRAMS IN A
     * CIRCUIT, below), p1 = 0, num_constraints = the program's EMIT count.  glp_circuit_create / _ex have no program list and answer
     * GLP_ERR_UNSUPPORTED for it, as for every type they do not know. */
    GLP_GATE_PROGRAM = 23
};

typedef struct {
    uint32_t type;
    uint32_t selector_index;           /* SelectorsInfo.selector_indices[gate] */
    uint32_t group_start, group_end;   /* SelectorsInfo.groups[selector_index] */
    uint32_t row;                      /* index of the gate in CommonCircuitData.gates */
    uint32_t num_constraints;
    uint32_t p0, p1;                   /* gate parameters (see GLP_GATE_*) */
} glp_gate;

typedef struct {
    uint32_t degree_bits;
    uint32_t num_wires, num_routed_wires;
    uint32_t num_constants;            /* all constant polynomials: selectors first, then gate constants */
    uint32_t num_selectors;
    uint32_t num_challenges;
    uint32_t quotient_degree_factor;
    uint32_t num_partial_products;
    uint32_t num_gate_constraints;
    uint32_t rate_bits, cap_height, proof_of_work_bits, num_query_rounds;
    uint32_t num_reductions;
    uint32_t reduction_arity_bits[16];
    uint32_t num_gates;
    uint32_t num_public_inputs;
    const glp_gate *gates;
    const uint64_t *k_is;              /* [num_routed_wires] */
    uint64_t circuit_digest[4];        /* verifier_only.circuit_digest; all-zero = let the library derive it */
    const uint64_t *constants;         /* [num_constants][n]    values on H (constant_vecs) */
    const uint64_t *sigmas;            /* [num_routed_wires][n] values on H (sigma_vecs) */
    uint32_t hasher;                   /* GLP_HASH_POSEIDON (0) or GLP_HASH_KECCAK25: `GenericConfig::Hasher` of the proof (Merkle trees,
                                          transcript, proof of work).  The public-input hash is the InnerHasher, Poseidon in both.
                                          With GLP_HASH_KECCAK25 every digest in caps, paths and circuit_digest is a 25-byte value in
                                          a 4-word slot (see GLP_HASH_KECCAK25 above) */
} glp_circuit_desc;

typedef struct glp_circuit glp_circuit;

/* Uploads the description and does the prover-side part of `build()`: commits constants ++ sigmas
 * (`constants_sigmas_commitment`) and, if desc->circuit_digest is all zero, derives the digest as
 * hash_no_pad(cap.flatten() ++ hash_pad([]) ++ [degree_bits]) (plonk/circuit_builder.rs). */
GLP_API int glp_circuit_create(glp_ctx *ctx, const glp_circuit_desc *desc, glp_circuit **out);
/* CircuitConfig { zero_knowledge: true, .. } (recalled from plonky2 0.1.x plonk/prover.rs, unpinned): the wires,
 * plonk_zs_partial_products and quotient commitments are salted (blinding = true; constants_sigmas is not).  The salts are never
 * opened at zeta; each query round's initial-tree proof carries the full salted leaves of oracles 1..3, salts last, so
 * glp_proof_words / glp_proof_bytes_len grow by 3 * 4 * num_query_rounds.  Transcript, proof of work and circuit digest do not
 * change.  The circuit itself must carry plonky2's blinding rows (the Rust builder and synth.py's zk configs add them).
 * glp_circuit_create(..) = glp_circuit_create_ex(.., 0).  Every path honours the flag: glp_prove, glp_prove_device,
 * glp_prove_staged (full witnesses only: the blinding rows' random advice wires come from no generator, so GLP_WITNESS_ROUTED_ONLY
 * is GLP_ERR_ARG), the session, glp_prove_batch (member k salts with seed3 + k), glp_verify / _n, glp_verify_batch and the byte
 * format.  Salt rule and seed: glp_batch_from_values_salted, glp_ctx_set_salt_seed. */
#define GLP_CIRCUIT_ZERO_KNOWLEDGE 1u
GLP_API int glp_circuit_create_ex(glp_ctx *ctx, const glp_circuit_desc *desc, uint32_t flags, glp_circuit **out);
/* GATE PROGRAMS IN A CIRCUIT.  A gate of type GLP_GATE_PROGRAM brings its unfiltered constraints as a gate program (the instruction
 * word of GLP_GP_INSTR, "caller-defined gate constraints at the commitment seam" above); every path of the circuit handle honours it:
 * glp_prove, glp_prove_device, glp_prove_staged, the session, glp_prove_batch, glp_verify / _n, glp_verify_batch and glp_witness_check.
 * This is the fifth reading of that format, for one gate at one point (a point of the quotient's coset, zeta, or a row of H):
 *     GLP_GP_COL       num_oracles = 2.  Oracle 0, polynomial c: constant polynomial c of the circuit, selectors first (c < num_constants;
 *                      the sigmas are not readable).  Oracle 1, polynomial j: wire j (j < num_wires)
 *     GLP_GP_PARAM     num_params <= 4: word j of the Poseidon hash of the public inputs
 *     GLP_GP_IMM, GLP_GP_REG, ADD / SUB / MUL / MOV   as in every reading
 *     GLP_GP_COL_NEXT, GLP_GP_X   refused: a plonky2 gate sees neither the next row nor the point
 *     EMIT             constraint k of the gate, k = the number of EMITs before it; at most GLP_GATE_PROGRAM_MAX_CONSTRAINTS
 *     END              exactly one, the last instruction, operand IMM of a pool word 1 (the shape glp_gate_program_rows asks for).  The
 *                      selector filter is NOT part of the program: the library multiplies by its own, made from the gate's
 *                      selector_index, group_start, group_end and row as for every built-in gate
 * The degree of a program is found by walking the code: COL is 1; IMM, PARAM and a register never written 0; ADD, SUB and MOV the
 * larger of their operands'; MUL the sum; the gate's degree is the largest over its EMIT operands.
 *
 * glp_gate_program_circuit_check (host only, no context) states these rules once: it refuses what glp_gate_program_check refuses and,
 * naming the instruction and the field, num_oracles other than 2, num_params above 4, COL_NEXT, X, an END that is not the last
 * instruction, an END operand other than IMM of a pool word 1, more than GLP_GATE_PROGRAM_MAX_CONSTRAINTS EMITs.  Outputs (each may be
 * null): the EMIT count, the degree, and one more than the largest wire / constant polynomial index read (0: none is read).
 *
 * glp_circuit_create_prog is glp_circuit_create_ex with a program list (num_programs = 0: exactly glp_circuit_create_ex, type 23
 * included).  Beyond the refusals of both it refuses, with GLP_ERR_ARG naming the gate index and the field and before anything is
 * launched or *out is written: p0 >= num_programs; p1 != 0; num_constraints different from the program's EMIT count; a wire index
 * >= num_wires or a constant index >= num_constants; degree + selector-filter degree > quotient_degree_factor + 1 (the rule the
 * recursion gates are held to; the filter has one factor per other gate of the group and one more when the circuit has several
 * selectors).  The programs are copied: the descriptions may be freed after the call.
 * Witness generation has no built-in generator for a program gate: glp_witness_fill leaves its rows alone and glp_witness_num_units
 * is 0, so glp_witness_plan_create_prog treats them as it treats NoopGate rows and the caller's unit programs write them.
 * The circuit hand-off file (below) does not carry programs: a description with a gate of type 23 is written and read like any other,
 * and its reader passes the programs to glp_circuit_create_prog from elsewhere. */
#define GLP_GATE_PROGRAM_MAX_CONSTRAINTS 4096u   /* = GLP_GP_MAX_CONSTRAINTS: the kernel's accumulators are Acc160 (2^32 terms); built-in gates hold 512 */
GLP_API int glp_gate_program_circuit_check(const glp_gate_program_desc *desc, uint32_t *num_constraints_out, uint32_t *degree_out,
                                           uint32_t *wires_used_out, uint32_t *consts_used_out);
GLP_API int glp_circuit_create_prog(glp_ctx *ctx, const glp_circuit_desc *desc, uint32_t flags, const glp_gate_program_desc *programs,
                                    uint32_t num_programs, glp_circuit **out);
/* 1 if the circuit was created with GLP_CIRCUIT_ZERO_KNOWLEDGE, else 0 */
GLP_API int glp_circuit_zero_knowledge(const glp_circuit *circuit);
GLP_API void glp_circuit_free(glp_circuit *circuit);
GLP_API int glp_circuit_digest(const glp_circuit *circuit, uint64_t digest_out[4]);
GLP_API int glp_circuit_constants_sigmas_cap(const glp_circuit *circuit, uint64_t *cap_out);
/* Number of uint64_t words of a proof of this circuit (layout below). */
GLP_API size_t glp_proof_words(const glp_circuit *circuit);

/* ---- circuit hand-off file --------------------------------------------------------------
 * The reference persists circuits with `CircuitData::to_bytes(&gate_serializer, &generator_serializer)` and reloads them
 * with `from_bytes` [REF src/ecdsa/gadgets/ecdsa.rs:298-316; serializer tables REF src/ecdsa/gadgets/ecdsa.rs:68-135,
 * src/ecdsa/serialization.rs:7-46].  That byte layout belongs to the absent plonky2 crate and carries the generator list,
 * which the GPU prover does not need.  The file below is this library's own flat dump of glp_circuit_desc (+ optionally one
 * witness and its public inputs): versioned header, little-endian sections, FNV-1a checksum; the exact layout is at the top
 * of plonky2-lib_amd/csrc/circuit_file.hip, the Rust writer that fills it from `data.common` / `data.prover_only` is in
 * INTEGRATION.md.  Host-only calls (no GPU needed); glp_circuit_file_open maps the file (GB-sized circuits are not copied)
 * and the descriptor's pointers stay valid until glp_circuit_file_close. */
typedef struct glp_circuit_file glp_circuit_file;
GLP_API int glp_circuit_file_write(const char *path, const glp_circuit_desc *desc, const uint64_t *wires /* [num_wires][n] or NULL */,
                                   const uint64_t *public_inputs /* [num_public_inputs], with wires */);
GLP_API int glp_circuit_file_open(const char *path, int verify_checksum, glp_circuit_file **out);
GLP_API void glp_circuit_file_close(glp_circuit_file *file);
GLP_API const glp_circuit_desc *glp_circuit_file_desc(const glp_circuit_file *file);       /* feed to glp_circuit_create */
GLP_API const uint64_t *glp_circuit_file_wires(const glp_circuit_file *file);              /* NULL if the file has no witness */
GLP_API const uint64_t *glp_circuit_file_public_inputs(const glp_circuit_file *file);

/* `CircuitData::prove` after witness generation (plonk/prover.rs `prove_with_partition_witness`,
 * steps "compute wires commitment" .. "compute opening proofs").
 *   wires          [num_wires][n] full witness (`witness.wire_values`), host or (…_device) HBM resident
 *   public_inputs  [num_public_inputs]
 *   proof_out      glp_proof_words() words, field order of plonky2's `Buffer::write_proof`:
 *     wires_cap | plonk_zs_partial_products_cap | quotient_polys_cap           each [2^cap_height][4]
 *     openings: constants, plonk_sigmas, wires, plonk_zs, plonk_zs_next, partial_products, quotient_polys   (ext each)
 *     commit_phase_merkle_caps [num_reductions][2^cap_height][4]
 *     query_round_proofs [num_query_rounds]: 4 x (leaf values, merkle path) then per reduction (evals, merkle path);
 *                        a zk circuit's leaves of oracles 1..3 end with their 4 salts
 *     final_poly (ext coefficients) | pow_witness | public_inputs
 * The FRI proof-of-work witness is the SMALLEST valid one (the Rust prover's rayon `find_any`
 * returns an arbitrary valid one; every other word of the proof is a deterministic function of
 * the inputs and of that witness).
 * A word >= p: wires and public_inputs in host memory are refused naming column and index (glp_prove, and the public inputs of
 * glp_prove_device and glp_prove_staged); dev_wires are reduced as they are loaded, so the proof is that of dev_wires % p. */
GLP_API int glp_prove(glp_ctx *ctx, const glp_circuit *circuit, const uint64_t *wires, const uint64_t *public_inputs,
                      uint64_t *proof_out);
GLP_API int glp_prove_device(glp_ctx *ctx, const glp_circuit *circuit, const uint64_t *dev_wires,
                             const uint64_t *public_inputs, uint64_t *proof_out);

/* ---- witnesses that start in host memory, pipelined -------------------------------------------------------------------
 * `data.prove(pw)` starts from a witness the CPU has just generated [REF src/ecdsa/gadgets/ecdsa.rs:332-349: set the targets, then
 * prove].  glp_prove(host wires) uploads it inside the call; a caller that proves witness after witness hides the upload behind
 * the previous proof instead:
 *     glp_witness_stage(ctx, circuit, wires[i+1], flags, &w_next);        returns at once: the copy runs on the ctx's copy stream
 *     glp_prove_staged(ctx, circuit, w_cur, public_inputs, proof_out);    the compute stream waits for w_cur's copy, then proves
 *     glp_witness_free(w_cur);
 * For the copy to overlap anything the host buffer must be page-locked: glp_host_alloc hands out such memory (have witness
 * generation write into it); pageable memory works and is staged by the HIP runtime, synchronously.  Either way host_wires must stay
 * valid and unchanged until glp_prove_staged has returned for that witness (or glp_witness_free has).
 * GLP_WITNESS_ROUTED_ONLY: host_wires holds only the routed columns [num_routed_wires][n] (= the first columns of the full
 * [num_wires][n] layout, so the full array may be passed as well); the advice columns are zero-filled on the device and derived
 * there by glp_witness_fill(only_advice) before the proof starts -- for the secp256k1 trace 56 of 136 columns (41 %) never cross
 * PCIe.  The proof is word for word the proof of the complete witness provided every advice wire of the witness is either
 * written by a row-local generator or zero (true for witnesses of plonky2's generators; tests/test_gpu_witness.py). */
/* glp_witness_stage: a word >= p in the columns it copies (all, or the routed ones with GLP_WITNESS_ROUTED_ONLY) is refused (host array). */
typedef struct glp_witness glp_witness;
#define GLP_WITNESS_ROUTED_ONLY 1u
GLP_API int glp_host_alloc(glp_ctx *ctx, size_t bytes, void **host_out);      /* page-locked host memory */
GLP_API int glp_host_free(glp_ctx *ctx, void *host);
GLP_API int glp_witness_stage(glp_ctx *ctx, const glp_circuit *circuit, const uint64_t *host_wires, uint32_t flags, glp_witness **out);
GLP_API int glp_prove_staged(glp_ctx *ctx, const glp_circuit *circuit, glp_witness *witness, const uint64_t *public_inputs,
                             uint64_t *proof_out);
GLP_API void glp_witness_free(glp_witness *witness);

/* Many independent proofs of ONE circuit in lock step (BASELINE config 5: a batch of zkdsa simple-signature proofs, the unit
 * [REF src/zkdsa/circuits/mod.rs:24-43,322-339] proves one at a time).  Small circuits are bound by launch and host round-trip
 * latency when proved one by one; here every device stage is one launch over all num_proofs proofs and every host round trip
 * carries all their caps / openings, while the num_proofs Fiat-Shamir transcripts run on host threads (environment variable GLP_HOST_THREADS; default: the
 * cores this process may use -- affinity mask capped by the cgroup CPU quota -- up to 32; every context has its own pool).  proofs_out[k] is word for word what glp_prove returns for witness k.
 *   wires          [num_proofs][num_wires][n], host memory, or (wires_on_device != 0) an HBM pointer on the ctx's GPU.  A word >= p:
 *                  host: refused naming proof, column and index; device: reduced as it is loaded
 *   public_inputs  [num_proofs][num_public_inputs], host: a word >= p is refused naming proof and index
 *   proofs_out     [num_proofs][glp_proof_words(circuit)]
 * Scope: num_challenges = 2 (every CircuitConfig the reference uses). */
GLP_API int glp_prove_batch(glp_ctx *ctx, const glp_circuit *circuit, uint32_t num_proofs, const uint64_t *wires, int wires_on_device,
                            const uint64_t *public_inputs, uint64_t *proofs_out);

/* ---- witness generation, the row-local half ------------------------------------------
 * plonky2 `iop/generator.rs::generate_partial_witness` interleaves two kinds of work: the copy-constraint dataflow
 * between rows (stays with the reference's CPU gadget code) and the row-local `SimpleGenerator`s that derive the rest
 * of a row from that row's own inputs.  glp_witness_fill applies every row-local generator of the gate library once,
 * one GPU thread per trace row, in place on an HBM-resident witness [num_wires][n]:
 *   the reference's own generators  U32InterleaveGenerator [REF src/u32/gates/interleave_u32.rs:289-318],
 *     UninterleaveToU32Generator [REF src/u32/gates/uninterleave_to_u32.rs:332-369], UninterleaveToB32Generator
 *     [REF src/u32/gates/uninterleave_to_b32.rs:335-372];
 *   plonky2_u32 (recalled) U32Arithmetic / U32AddMany / U32Subtraction / U32RangeCheck / Comparison generators;
 *   plonky2 (recalled)     BaseSplitGenerator, ArithmeticBaseGenerator, RandomAccessGenerator, PoseidonGenerator,
 *                          ConstantGenerator, ArithmeticExtensionGenerator, MulExtensionGenerator, ReducingGenerator,
 *                          ReducingExtensionGenerator, ExponentiationGenerator, InterpolationGenerator (CosetInterpolationGate),
 *                          PoseidonMdsGenerator.
 * Each generator reads its dependencies (glp_witness_columns role 2) from the row and writes its outputs (role 1):
 * bits, base-4 limbs, inverses, S-box traces, u32 results.  only_advice != 0: only non-routed columns
 * (index >= num_routed_wires) are written, for a caller whose CPU pass already resolved every routed wire -- then the
 * GPU derives the 56 limb columns of the secp256k1 trace (41 % of the witness) and they never cross PCIe.
 * The row's gate is read from the circuit's selector polynomials.  Asynchronous on the ctx stream.
 * Inputs outside a gate's domain (plonky2's generators panic or write an unsatisfiable row there) never fault; what is written is
 * fixed: inputs are reduced mod p as they are loaded (a cell that is not written keeps its word), and a limb or bit generator decomposes only the bits it has wires for -- the low 32 bits
 * of a u32 result (the result and carry wires themselves get the full field value), num_chunks * chunk_bits bits of a ComparisonGate
 * input (its result wire is the top bit of 2^chunk_bits + most significant difference), num_limbs digits of a BaseSum value; a
 * RandomAccessGate copy whose access index is >= 2^bits writes nothing for that copy (the extra constants are still written); a
 * CosetInterpolationGate row with shift 0 gets shifted point 0.  Such a row fails glp_witness_check, which names it.
 * tests/witness_fill_restate.py restates all of this, tests/witness_edge_rows.py holds the rows that exercise it. */
GLP_API int glp_witness_fill(glp_ctx *ctx, const glp_circuit *circuit, uint64_t *dev_wires, int only_advice);
/* role_out[col] for rows of gate `gate_index`: 1 = written by glp_witness_fill, 2 = read as a generator input, 0 = untouched */
GLP_API int glp_witness_columns(const glp_circuit *circuit, uint32_t gate_index, uint8_t *role_out /* [num_wires] */);

/* ---- witness generation, the dataflow half ----------------------------------------------------------------------
 * The other half of `generate_partial_witness`: values travel between rows along the copy constraints, and a generator runs once its
 * inputs are known.  The caller hands over only the values it sets itself -- the `pw.set_target` values; generators that belong to no
 * gate run as FREE UNITS, below -- and the GPU derives every other reachable cell in HBM, for num_proofs witnesses of one
 * circuit in lock step.  The result is what glp_prove_device / glp_prove_batch (wires_on_device) / glp_witness_check consume.
 *
 * UNITS.  A unit is one independent generator of a row (the loops of glp_witness_fill, one by one):
 *   ConstantGate 1 (no inputs) | ArithmeticGate p0 (unit i reads wires 4i..4i+2, writes 4i+3) | PoseidonGate 1 | U32Interleave p0 |
 *   UninterleaveToU32 / ToB32 p0 | U32Arithmetic p0 (each owns its limb range) | U32AddMany p1 | U32Subtraction p0 |
 *   U32RangeCheck p0 (one per input) | Comparison 1 | BaseSum 1 | RandomAccess copies + 1 (the last writes the extra constants, no
 *   inputs) | ArithmeticExtension, MulExtension p0 | Reducing, ReducingExtension 1 | Exponentiation, CosetInterpolation, PoseidonMds 1 |
 *   Noop, PublicInput 0.
 * glp_witness_unit_columns gives a unit's roles as glp_witness_columns does for the row; the union over a gate's units is exactly
 * glp_witness_columns and no column is written by two units.  glp_witness_num_units is 0 for a bad index.
 *
 * THE PLAN (host, once per circuit and input set).  A cell is named by its flat position col * n + row, col < num_wires (the encoding
 * of the decoded sigmas).  The copy classes are the cycles of the decoded permutation; a non-routed cell is a class of its own.
 *   Class wave.   The wave of a class is the minimum over its members of: 0 for an input cell; 0 for a random cell (RANDOM CELLS,
 *                 below: a wave-0 source exactly as an input cell is); the wave of the unit that writes the member.  A class with none
 *                 of these is never known.
 *   Source.       The class's source is the member that attains the minimum.  Ties go to the smallest flat position, with inputs and
 *                 random cells alike.
 *   Unit wave.    The wave of a unit is 1 + the maximum wave of the classes of the cells it reads.  It is 1 for a unit with no inputs.
 *                 Gate constants and selectors are always known.
 *   Stuck units.  A unit that reads a never-known class is stuck, and so is everything downstream of it.  Dependency cycles are
 *                 included.  Stuck units are counted.  The first stuck unit is named.  Stuck units are never run.
 *   Order within wave w.  Wave 0 is the scatter of the inputs and the draw of the random cells.  In every other wave, first every unit of wave w runs.  Then every
 *                 class whose wave is w is copied from its source to all its other members.
 *   cell_waves.   The unit's wave for a cell a unit writes (a unit that is not stuck); the class's wave for any other known cell; -1
 *                 for a cell that is never known.
 * An input cell whose class also contains a unit's output is allowed (plonky2 allows setting such a target too); if the two values
 * disagree, glp_witness_check reports the broken copy.  The stuck-unit report tells a caller which inputs it forgot: the named unit
 * reads a cell (glp_witness_unit_columns role 2, cell_waves -1) that nothing provides.
 * Refusals of glp_witness_plan_create (GLP_ERR_ARG, each names the field; all but the last two, which need the decoded permutation, are decided before any launch): a null pointer; a
 * circuit of another context; num_wires * n >= 2^32 (the bound of the decoded sigma, less the one position the planner keeps for
 * "none"); a cell out of range; a cell listed twice; two input
 * cells in one copy class (both named); a malformed sigma (as glp_witness_check).  The plan keeps its lists in HBM (per wave the units
 * (row, gate, unit) sorted by row and the copies (source, destination), the wave offsets, the input positions) and refers to the
 * circuit, which must outlive it; free it before its context is destroyed.  The planner is host code: at 2^20 rows x 80 routed
 * columns it walks 84 M cells, and it holds about 40 bytes of host memory per cell of num_wires * n while it runs (5-6 GB at 2^20 x
 * 136; GLP_ERR_UNSUPPORTED if that cannot be had) and 4 bytes per cell afterwards (cell_waves).
 *
 * GENERATION.  glp_witness_generate scatters input_values (host, [num_proofs][num_inputs] in the order of input_cells, canonical: a
 * word >= p is refused by proof and index) and runs the waves on the ctx stream.  The call first waits for the work queued on that
 * stream before it and copies the input values (so input_values may be reused at once); the kernels are then asynchronous, like
 * glp_witness_fill.  A plan holds the value buffer of the generation in flight: it serves one glp_witness_generate at a time, not two
 * callers at once, although it is passed as const.  num_proofs is 1..4096, the size cap is glp_witness_check's.  Cells the plan never reaches keep what the buffer
 * held, or are 0 with GLP_WITNESS_GEN_ZERO_FIRST.  For inputs consistent with the circuit the result is a deterministic function of
 * the inputs; for inconsistent inputs nothing faults and every cell holds a value that one of its sources produced.  Two forms run the
 * same per-unit body: walked waves (one 256-lane workgroup per proof walks a run of consecutive waves, a block barrier between the
 * units and the copies of a wave) and wide waves (one launch for a wave's units, one for its copies, grid.y = proof).  A wave is wide
 * while num_proofs is below the CU count and it holds more than GLP_WITNESS_NARROW_MAX units (environment variable, read when a plan
 * is made; default 256; 0 makes every wave wide, a value above any wave walks them all).  No workgroup hands anything to another
 * inside a launch.
 * glp_witness_read_cells (synchronous) reads cells of generated witnesses back: the public inputs of a generated witness are
 * themselves outputs (zkdsa's public key and signature), and glp_prove_batch needs them on the host.
 *
 * FREE UNITS.  A generator that belongs to no gate -- plonky2's `EqualityGenerator` (recalled, unpinned) and the BigUint / nonnative
 * generators of the secp256k1 gadgets [REF src/ecdsa/gadgets/nonnative.rs:453-830, biguint.rs:322-349, glv.rs:106-133] -- is a free
 * unit of glp_witness_plan_create_ex: a kind (GLP_WGEN_*), an index into moduli[] and a run of cells[]: the input cells, then the
 * output cells, operands in the kind's order, limbs little-endian, len[] cells per operand.  A virtual target is named through any
 * wire it was placed on; an output operand's cell may be GLP_WGEN_NO_CELL (a target that was placed nowhere: it is not written).  With
 * them a secp256k1 witness comes from the 40 words a caller sets per signature (msg, r, s, pk.x, pk.y; a builder that leaves the unused
 * operations of partly filled rows unwired, as the Python builders do, also lists their cells as inputs of value 0).  The rule extends to them:
 *   a free unit reads the classes of its input cells and is the writer of its output cells; its wave is 1 + the maximum wave of the
 *   classes it reads, 1 if it reads none; it is stuck under the same rule as a gate unit; class wave, source (ties to the smallest
 *   flat position), copies and cell_waves treat a free writer exactly like a gate writer; within a wave gate units and free units both
 *   run before the copies.  In glp_witness_plan_info num_units, num_stuck_units, widest_wave_units and stuck_* keep counting gate units
 *   only; num_waves is the highest wave that holds any unit; glp_witness_plan_free_info has the free counts (first_stuck_free_unit: an
 *   index into units[], iff num_stuck_free_units).
 * Semantics are the reference's `run_once` bodies.  The nonnative kinds first reduce every operand modulo m
 * (`from_noncanonical_biguint`); NONNATIVE_ADD overflows when a + b > m, strictly (a + b = m gives sum = m, overflow = 0); NONNATIVE_INV's
 * div is floor(x inv / m); GLV_SECP256K1 is `decompose_secp256k1_scalar` (rounding division by n, signs by comparison with n / 2).
 * Outside a generator's domain (the Rust code panics there) nothing faults and the result is fixed: an operand cell >= 2^32 is read as
 * its low 32 bits; a divisor of 0 gives div = rem = 0; x = 0 (mod m) or gcd(x, m) != 1 gives inv = div = 0; a result wider than the cells
 * the unit has for it is written truncated to those limbs; MULTI_ADD's overflow is the low limb of the quotient; EQUALITY is field
 * arithmetic, inv = 1 / (x - y) or 0 when x = y.  Such witnesses fail glp_witness_check, which names the row.  Every loop of the limb
 * arithmetic (csrc/biguint_dev.h, one text for device and host) has a trip count fixed by limb counts or a compile-time bound, and no
 * value read from a witness becomes a cell position (one count is taken from values: BIGUINT_DIV_REM divides by the divisor's limbs up
 * to its highest non-zero one, bounded by the declared count, at most 8).  One lane runs one free unit, in the units step of either form (walked waves: before
 * the first barrier; wide waves: a launch of their own); a wave counts as wide by its gate and free units together.  The per-wave free
 * list (offsets, unit records, cell runs, moduli) lies in HBM beside the units and the copies.  An 8-limb modulus with 8-limb operands
 * runs a fully unrolled instance, a device function of its own that keeps its limbs in registers (no scratch, no spills in the
 * compiler's report); every other shape runs a general-length instance, also a function of its own, whose arrays lie in scratch.
 * Refusals of glp_witness_plan_create_ex beyond those above (GLP_ERR_ARG, each names the unit and the field, none needs a launch): an
 * unknown kind; a len outside the kind's shape (EQUALITY: four operands of 1 cell; an overflow cell count other than 1 for ADD,
 * MULTI_ADD, SUB; GLV: 8, 4, 4, 1, 1; unused entries not 0); an operand longer than GLP_WGEN_MAX_LIMBS; a divisor (BIGUINT_DIV_REM's b)
 * longer than 8 limbs; modulus >= num_moduli for kinds 2..6, modulus != 0 otherwise; a modulus that is even or below 3 (a modulus has
 * no declared length: its limbs run to its highest non-zero one); an input cell out of range; an output cell out of range that is not
 * GLP_WGEN_NO_CELL; a run that leaves cells[]; an output cell written by two free units; an output cell that a gate unit of that row
 * also writes.  An output cell whose class holds an input is allowed, as above.  glp_witness_plan_create is the num_units = 0 case.
 *
 * UNIT PROGRAMS.  A generator this library does not know -- plonky2's small non-gate generators (`WireSplitGenerator`,
 * `LowHighGenerator`, quotient), or the generator of a caller-defined gate whose rows the caller declares as NoopGate in the circuit it
 * plans with (a Noop row has no units) -- is stated as the caller states a constraint: a straight-line program in the instruction word
 * of GLP_GP_INSTR (opcode, dst, a, b and the 27-bit operands as there, bit 63 zero), run as a free unit of kind GLP_WGEN_PROGRAM by
 * glp_witness_plan_create_prog.  This is the fourth reading of that format, for one unit of one proof:
 *     GLP_GP_REG, GLP_GP_IMM       as in a gate program
 *     GLP_GP_COL                   oracle 0 only; payload j < num_inputs: the canonical 64-bit value of the unit's j-th input cell (the
 *                                  whole word, not its low 32 bits)
 *     GLP_GP_COL_NEXT, _PARAM, _X  refused
 *     ADD, SUB, MUL, MOV           as in a gate program
 *     EMIT a                       writes a to the unit's output cell number t, t counting the EMITs from the start of the program; the
 *                                  number of EMITs is num_outputs
 *     END                          exactly one, the last instruction, operand IMM of a pool word 1 (the shape glp_gate_program_rows asks for)
 *     GLP_WP_OP_INV0 dst, a        1 / a, or 0 when a = 0 (a^(p-2), a fixed-length exponentiation)
 *     GLP_WP_OP_BITS dst, a, b     b an IMM whose pool word is lo + 256 * width (GLP_WP_BITS_RANGE), width >= 1, lo + width <= 64:
 *                                  (a >> lo) & (2^width - 1) on the canonical integer of a
 *     GLP_WP_OP_LT   dst, a, b     1 if canonical a < canonical b, else 0
 * Every result is canonical.  There are no branches and no loops, and nothing read from a witness becomes an address or a trip count.
 * Left out on purpose: integer products wider than the field (the U32 gate generators are gate units already).
 * glp_witness_program_check refuses (GLP_ERR_ARG, "instruction <i>, field <op|dst|a|b>: ...", or naming the description's field): an
 * unknown opcode or bit 63; a destination or a second operand in an instruction that has none; a register >= num_regs; a register read
 * before it is written; a pool index out of range; COL with a non-zero oracle or j >= num_inputs; COL_NEXT, PARAM, X or an unknown
 * operand kind; a BITS operand b that is not an IMM, or whose pool word has width 0, lo + width > 64 or bits above bit 15; a number of
 * EMITs other than num_outputs; a last instruction that is not END IMM(1); an END before the last instruction; a non-canonical pool
 * word; num_instructions outside 1..GLP_GP_MAX_INSTRUCTIONS, num_regs outside 1..GLP_GP_MAX_REGS, num_inputs or num_outputs outside
 * 1..GLP_WP_MAX_CELLS, num_pool above 2^24.
 * A program unit names its program in `modulus` and has len[0] = num_inputs, len[1] = num_outputs, len[2..5] = 0; its run is the input
 * cells, then the output cells (GLP_WGEN_NO_CELL: not written).  It is a free unit in every respect of the rule above (wave, stuck,
 * writer of its outputs, the two "also written" refusals, glp_witness_plan_free_info).  glp_witness_plan_create_prog refuses beyond
 * glp_witness_plan_create_ex, before any launch, naming the unit and the field: modulus >= num_programs; len[0] or len[1] different from
 * the program's counts; len[2..5] not 0; a program that glp_witness_program_check refuses ("programs[<p>]: ..." and its message).
 * glp_witness_plan_create_ex is the num_programs = 0 case of the same body and keeps refusing kind 9 as an unknown kind.
 * A wave that holds program units is always a wide wave, with one launch more between its units and its copies: the planner sorts the
 * wave's program units by program and cuts them into chunks of at most 64 units of one program, and one 64-lane workgroup runs one
 * chunk (grid.y = proof), so that the instruction stream is uniform across the lanes; instruction words and pool come through scalar
 * loads, the register file lies in LDS.  Walked runs stop before such a wave and resume after it: the walked kernels hold nothing of the
 * interpreter.  The programs (code and pool, concatenated, with an offset table) lie in HBM with the plan.
 *
 * RANDOM CELLS.  The random advice of a zero-knowledge circuit's blinding rows (plonky2 `blind`: rows of random wires, and pairs of rows
 * whose routed wires are random and copy-constrained to each other) comes from no generator and need not come from the caller either: a
 * blinding value only has to be unpredictable, as a salt does.  glp_witness_plan_create_rand takes, after input_cells and num_inputs,
 * random_cells[num_random] (flat positions), and glp_witness_generate fills them on the device from the PRF stated beside
 * GLP_SALT_TAG_WITNESS: cell number i of the caller's list gets word i & 7 of the permutation of block i >> 3.  A random cell is a wave-0
 * source exactly as an input cell is: its class has wave 0, the copies of wave 0 carry the value to the rest of the class (the second
 * row of a blinding pair: list only the first), cell_waves is 0 for it, num_cells_known counts it; a random cell whose class also holds
 * a unit's output is allowed, as for inputs, and glp_witness_check reports the broken copy.  For a plan with random cells
 * glp_witness_generate draws one seed per call, the way the provers draw their salt seed (OS entropy, or the fixed seed of
 * glp_ctx_set_salt_seed for tests; proof k uses seed3 + k); nothing else about the call changes, input_values stays
 * [num_proofs][num_inputs], and a plan without random cells draws no seed and launches what it always launched.  One kernel runs once
 * per call, one lane per block of eight cells (grid.y = proof), with the scatter of the inputs and before the copies of wave 0 in both
 * forms; wave 0 counts as wide by its inputs and random cells together (its copies are the blinding pairs' second rows).  A zkdsa witness under standard_recursion_zk_config then still comes from 8 words per proof.
 * Refusals of glp_witness_plan_create_rand beyond those above (GLP_ERR_ARG, each names the field, decided with the input cells'):
 * random_cells null with num_random > 0; a random cell out of range; listed twice; also listed as an input cell; two random cells, or a
 * random cell and an input cell, in one copy class (both named).  glp_witness_plan_create_prog is the num_random = 0 case of the same body.
 *
 * NOT done here: glp_witness_stage(GLP_WITNESS_ROUTED_ONLY) on a zero-knowledge circuit (refused as before: glp_witness_fill knows no
 * random cells); a device-side planner; integer products wider than the field in a unit program.
 * tests/witness_plan_restate.py restates the units, the classes, the rule and generation; tests/witness_free_restate.py the free units;
 * tests/witness_program_restate.py the unit programs. */
typedef struct glp_witness_plan glp_witness_plan;
struct glp_witness_plan_info {           /* a struct tag, not a typedef: the accessor below carries the same name */
    uint32_t num_waves;                  /* highest wave that holds a unit; 0 if none */
    uint64_t num_units, num_stuck_units, num_copies, num_cells_known;
    uint64_t widest_wave_units;
    uint64_t stuck_row; uint32_t stuck_gate, stuck_unit;   /* first stuck unit in (row, unit) order, iff num_stuck_units */
};
#define GLP_WITNESS_GEN_ZERO_FIRST 1u   /* zero the buffers first: plonky2's full_witness leaves every unset wire 0 */
GLP_API uint32_t glp_witness_num_units(const glp_circuit *c, uint32_t gate_index);   /* 0 for a bad index */
GLP_API int glp_witness_unit_columns(const glp_circuit *c, uint32_t gate_index, uint32_t unit,
                                     uint8_t *role_out /* [num_wires], roles of glp_witness_columns */);
GLP_API int  glp_witness_plan_create(glp_ctx *ctx, const glp_circuit *c, const uint64_t *input_cells, uint32_t num_inputs,
                                     glp_witness_plan **out);
#define GLP_WGEN_EQUALITY            1u  /* in: x, y (1 cell each)   out: equal, inv                       (plonky2, recalled) */
#define GLP_WGEN_NONNATIVE_ADD       2u  /* in: a, b                 out: sum, overflow (1 cell)            nonnative.rs:475-490 */
#define GLP_WGEN_NONNATIVE_MULTI_ADD 3u  /* in: len[0] summands of len[1] limbs   out: sum, overflow (1 cell, u32)  :553-576 */
#define GLP_WGEN_NONNATIVE_SUB       4u  /* in: a, b                 out: diff, overflow (1 cell)           :648-663 */
#define GLP_WGEN_NONNATIVE_MUL       5u  /* in: a, b                 out: prod, overflow (limbs)            :727-740 */
#define GLP_WGEN_NONNATIVE_INV       6u  /* in: x                    out: inv, div                          :797-809 */
#define GLP_WGEN_BIGUINT_DIV_REM     7u  /* in: a, b                 out: div, rem            biguint.rs:342-349 */
#define GLP_WGEN_GLV_SECP256K1       8u  /* in: k (8 limbs)          out: k1, k2 (4 limbs each), k1_neg, k2_neg   glv.rs */
#define GLP_WGEN_MAX_LIMBS          18u  /* an operand; a modulus or a divisor has at most 8 */
#define GLP_WGEN_NO_CELL 0xFFFFFFFFFFFFFFFFull   /* an output cell that is not written */
typedef struct {
    uint32_t kind, modulus;      /* modulus: index into moduli[] for kinds 2..6, otherwise 0 */
    uint32_t cell_begin;         /* this unit's run in cells[]: operands in the kind's order, inputs first, limbs little-endian */
    uint16_t len[6];             /* limb (cell) count per operand in that order; unused entries 0 */
} glp_witness_free_unit;
struct glp_witness_plan_free_info {      /* a struct tag, as glp_witness_plan_info */
    uint64_t num_free_units, num_stuck_free_units;
    uint64_t first_stuck_free_unit;      /* index into units[], iff num_stuck_free_units */
    uint64_t widest_wave_free_units;
};
GLP_API int glp_witness_plan_create_ex(glp_ctx *ctx, const glp_circuit *c, const uint64_t *input_cells, uint32_t num_inputs,
                                       const glp_witness_free_unit *units, uint32_t num_units, const uint64_t *cells, size_t num_cells,
                                       const uint32_t *moduli /* [num_moduli][8], little-endian u32 limbs */, uint32_t num_moduli,
                                       glp_witness_plan **out);
/* UNIT PROGRAMS: see the block above.  Opcodes 7..9 exist in unit programs only (glp_gate_program_check keeps refusing them). */
#define GLP_WP_OP_INV0 7u                /* dst, a:     1 / a, or 0 when a = 0 */
#define GLP_WP_OP_BITS 8u                /* dst, a, b:  b an IMM whose pool word is lo + 256 * width; (a >> lo) & (2^width - 1) */
#define GLP_WP_OP_LT   9u                /* dst, a, b:  1 if canonical a < canonical b, else 0 */
#define GLP_WP_MAX_CELLS 4096u
#define GLP_WP_BITS_RANGE(lo, width) ((uint64_t)(lo) + 256u * (uint64_t)(width))
typedef struct {
    const uint64_t *code;  uint32_t num_instructions;   /* 1..GLP_GP_MAX_INSTRUCTIONS */
    const uint64_t *pool;  uint32_t num_pool;           /* canonical words */
    uint32_t num_regs;                                  /* 1..GLP_GP_MAX_REGS */
    uint32_t num_inputs, num_outputs;                   /* cells a unit of this program reads / writes; each 1..GLP_WP_MAX_CELLS */
} glp_witness_program_desc;
GLP_API int glp_witness_program_check(const glp_witness_program_desc *d);   /* host only, no context */
#define GLP_WGEN_PROGRAM 9u   /* modulus = index into programs[]; len[0] = num_inputs, len[1] = num_outputs, len[2..5] = 0 */
GLP_API int glp_witness_plan_create_prog(glp_ctx *ctx, const glp_circuit *c, const uint64_t *input_cells, uint32_t num_inputs,
                                         const glp_witness_free_unit *units, uint32_t num_units, const uint64_t *cells, size_t num_cells,
                                         const uint32_t *moduli /* [num_moduli][8] */, uint32_t num_moduli,
                                         const glp_witness_program_desc *programs, uint32_t num_programs, glp_witness_plan **out);
/* RANDOM CELLS: see the block above.  The new pair follows input_cells, num_inputs; everything else is glp_witness_plan_create_prog. */
GLP_API int glp_witness_plan_create_rand(glp_ctx *ctx, const glp_circuit *c, const uint64_t *input_cells, uint32_t num_inputs,
                                         const uint64_t *random_cells, uint32_t num_random,
                                         const glp_witness_free_unit *units, uint32_t num_units, const uint64_t *cells, size_t num_cells,
                                         const uint32_t *moduli /* [num_moduli][8] */, uint32_t num_moduli,
                                         const glp_witness_program_desc *programs, uint32_t num_programs, glp_witness_plan **out);
GLP_API uint32_t glp_witness_plan_num_random(const glp_witness_plan *p);   /* 0 for a null plan */
GLP_API int glp_witness_plan_free_info(const glp_witness_plan *p, struct glp_witness_plan_free_info *out);
GLP_API int  glp_witness_plan_info(const glp_witness_plan *p, struct glp_witness_plan_info *out);
GLP_API int  glp_witness_plan_cell_waves(const glp_witness_plan *p, int32_t *waves_out /* [num_wires][n] */);
GLP_API void glp_witness_plan_free(glp_witness_plan *p);
GLP_API int glp_witness_generate(glp_ctx *ctx, const glp_witness_plan *p, uint32_t num_proofs,
                                 const uint64_t *input_values /* host [num_proofs][num_inputs], order of input_cells, canonical */,
                                 uint64_t *dev_wires /* HBM [num_proofs][num_wires][n] */, uint32_t flags);
GLP_API int glp_witness_read_cells(glp_ctx *ctx, const glp_circuit *c, uint32_t num_proofs, const uint64_t *dev_wires,
                                   const uint64_t *cells, uint32_t num_cells, uint64_t *out /* host [num_proofs][num_cells] */);

/* ---- witness checker: which gate, row, constraint or copy does a witness break ----------------------------------
 * A witness that does not satisfy its circuit goes through glp_prove without complaint and yields a proof that every verifier
 * rejects with "Mismatch between evaluation and opening of quotient polynomial".  glp_witness_check evaluates, on the rows of H,
 * every gate's unfiltered constraints (the bodies the quotient kernels evaluate on the LDE) and every copy constraint, for
 * num_proofs witnesses [num_proofs][num_wires][n] of one circuit in one call, and names what fails.  GLP_OK = the check ran; the
 * verdict is in the reports (as with glp_fri_verify_many): a witness satisfies the circuit iff its three counts are 0.
 *   constraints  the gate of a row is read as glp_witness_fill reads it (the selector polynomial of its group holds the gate index,
 *                every other selector UNUSED; a row whose selectors name no gate is skipped); constraint k is the gate's k-th
 *                constraint in its own order, k < glp_gate.num_constraints.  PublicInputGate is checked against the Poseidon hash
 *                of public_inputs[k], the hash glp_prove computes.
 *   copies       routed position (column j, row i), j < num_routed_wires, fails iff wires[j][i] != wires[j'][i'] where
 *                sigmas[j][i] == k_is[j'] * w_n^i'.
 * Refusals (all GLP_ERR_ARG, before the first gate launch): a null pointer; num_proofs outside 1..4096; public_inputs == NULL for a
 * circuit with public inputs; a host wire word >= p, named by proof and word index (device wires are reduced as they are loaded);
 * a sigma value that is k_is[j'] * w_n^i' for no (j', i'), named as sigmas[j][i] -- a malformed circuit, not a bad witness.
 * The witness is only read.  The first check of a circuit decodes its sigmas into positions and keeps them with the circuit (4 bytes per
 * routed position, freed by glp_circuit_free); later checks of any number of witnesses reuse them.  rows_failed_by_gate_out (NULL or [num_proofs][num_gates]) counts the failing rows per gate. */
typedef struct {
    uint64_t failed_constraints;  /* (row, constraint) pairs whose unfiltered value is not 0 mod p */
    uint64_t failed_rows;         /* rows with at least one of them */
    uint64_t failed_copies;       /* routed positions (column, row) whose wire differs from the wire at sigma(column, row) */
    /* first failing constraint in (row, constraint) order; meaningful iff failed_constraints != 0 */
    uint64_t row;  uint32_t gate, constraint;  uint64_t value;      /* value canonical, != 0 */
    /* first failing copy in (row, column) order; meaningful iff failed_copies != 0 */
    uint64_t copy_row;  uint32_t copy_col, to_col;  uint64_t to_row, copy_value, to_value;
} glp_witness_report;
GLP_API int glp_witness_check(glp_ctx *ctx, const glp_circuit *circuit, uint32_t num_proofs,
                              const uint64_t *wires /* [num_proofs][num_wires][n] */, int wires_on_device,
                              const uint64_t *public_inputs /* [num_proofs][num_public_inputs] or NULL if the circuit has none */,
                              glp_witness_report *reports_out /* [num_proofs] */,
                              uint64_t *rows_failed_by_gate_out /* NULL or [num_proofs][num_gates] */);

/* ---- the same proof, stepped by the caller's own transcript -------------------------------------------------
 * `prove_with_partition_witness` is Fiat-Shamir glue around six device stages.  A Rust integration that keeps
 * plonky2's own `Challenger` (so that the transcript is the fork's by construction) calls the stages one by one:
 * each call returns exactly what the Rust prover observes next, and takes exactly the challenges it draws next
 * [UPSTREAM plonky2 plonk/prover.rs: `challenger.observe_cap(..)` / `get_n_challenges` / `get_extension_challenge`;
 *  fri/prover.rs: `fri_committed_trees`, `fri_proof_of_work`, `fri_prover_query_rounds`; reached from
 *  REF src/ecdsa/gadgets/ecdsa.rs:349].  Order (enforced; GLP_ERR_ARG otherwise):
 *
 *   glp_session_begin              wires -> iNTT, LDE, Merkle           out: wires cap, hash of the public inputs
 *   glp_session_partial_products   in: betas, gammas [num_challenges]   out: plonk_zs_partial_products cap
 *   glp_session_quotient           in: alphas [num_challenges]          out: quotient_polys cap
 *   glp_session_open               in: zeta (ext)                       out: OpeningSet, 2 words per opening, proof order
 *   glp_session_fri_combine        in: FRI alpha (ext)
 *   num_reductions x { glp_session_fri_commit (out: layer cap) ; glp_session_fri_fold (in: beta, ext) }
 *   glp_session_fri_final_poly     out: final polynomial coefficients (ext)
 *   glp_pow_search                 (stateless) in: the challenger's sponge state + pending inputs   out: witness
 *   glp_session_queries            in: pow witness, query indices x_index in [0, 2^(degree_bits+rate_bits))
 *   glp_session_proof              out: the assembled proof words (same layout as glp_prove)
 *   glp_session_end
 *
 * glp_prove() is this sequence driven by the library's built-in transcript; tests/test_gpu_prove.py drives it with the
 * oracle's Challenger and requires the identical proof. */
typedef struct glp_session glp_session;
/* wires: [num_wires][n]; wires_on_device != 0: an HBM pointer that must stay valid until glp_session_end.  A word >= p: host wires
 * and public_inputs are refused by name, no session is made; device wires are reduced as they are loaded.  The pow_witness of
 * glp_session_queries (and of glp_fri_queries, glp_fri_queries_many) is a field element of the proof: >= p is refused. */
GLP_API int glp_session_begin(glp_ctx *ctx, const glp_circuit *circuit, const uint64_t *wires, int wires_on_device,
                              const uint64_t *public_inputs, glp_session **out, uint64_t *wires_cap_out /* [2^cap_height][4] */,
                              uint64_t public_inputs_hash_out[4]);
GLP_API int glp_session_partial_products(glp_session *s, const uint64_t *betas, const uint64_t *gammas, uint64_t *zs_cap_out);
GLP_API int glp_session_quotient(glp_session *s, const uint64_t *alphas, uint64_t *quotient_cap_out);
/* openings_out: 2 * glp_num_openings(circuit) words: constants, plonk_sigmas, wires, plonk_zs, plonk_zs_next,
 * partial_products, quotient_polys (the order `OpeningSet::to_fri_openings` / the proof uses) */
GLP_API size_t glp_num_openings(const glp_circuit *circuit);
GLP_API int glp_session_open(glp_session *s, const uint64_t zeta[2], uint64_t *openings_out);
GLP_API int glp_session_fri_combine(glp_session *s, const uint64_t alpha[2]);
GLP_API int glp_session_fri_commit(glp_session *s, uint64_t *cap_out);
GLP_API int glp_session_fri_fold(glp_session *s, const uint64_t beta[2]);
GLP_API size_t glp_final_poly_len(const glp_circuit *circuit);          /* ext coefficients */
GLP_API int glp_session_fri_final_poly(glp_session *s, uint64_t *coeffs_out /* [2 * glp_final_poly_len] */);
/* smallest w such that a duplex sponge in `sponge_state` with `num_pending` (< 8) buffered inputs, after also
 * observing w, squeezes an element with `bits` leading zero bits (fri_proof_of_work).  The twelve state words and the pending
 * inputs are field elements, canonical as every field argument of this API: a word >= p is GLP_ERR_ARG naming sponge_state[i] or
 * pending_inputs[i], decided on the host before any launch (the permutations take canonical words). */
GLP_API int glp_pow_search(glp_ctx *ctx, const uint64_t sponge_state[12], const uint64_t *pending_inputs, uint32_t num_pending,
                           uint32_t bits, uint64_t *witness_out);
/* the same, with the same refusals, for a transcript whose permutation is that of `hasher` (GLP_HASH_KECCAK25: KeccakPermutation) */
GLP_API int glp_pow_search_h(glp_ctx *ctx, uint32_t hasher, const uint64_t sponge_state[12], const uint64_t *pending_inputs,
                             uint32_t num_pending, uint32_t bits, uint64_t *witness_out);
/* The session's committed oracles, index 0..3: constants_sigmas, wires, zs and partial products, quotient.  Valid once the stage that
 * commits that oracle has run (0, 1: after begin; 2: partial_products; 3: quotient); GLP_ERR_ARG before that or for another index.
 * The handle is borrowed until glp_session_end: read it (glp_batch_coeffs of Z or of the quotient) or hand it to glp_fri_*. */
GLP_API int glp_session_oracle(glp_session *s, uint32_t index, const glp_batch **out);
GLP_API int glp_session_queries(glp_session *s, uint64_t pow_witness, const uint64_t *indices, uint32_t num_indices);
GLP_API int glp_session_proof(glp_session *s, uint64_t *proof_out /* glp_proof_words(circuit) */);
GLP_API void glp_session_end(glp_session *s);

/* `CircuitData::verify(proof)` [REF src/ecdsa/gadgets/ecdsa.rs:352, src/zkdsa/circuits/mod.rs:346]: checks a proof in
 * the word layout above against the circuit (gate table, coset shifts, digest, constants/sigmas cap): transcript,
 * proof of work, vanishing polynomial at zeta against the quotient openings, every FRI query (Merkle paths, initial
 * combination, arity-2^k consistency, final polynomial).  Host computation (a few thousand Poseidon permutations), no
 * device work.  GLP_OK = accepted; GLP_ERR_PROVE with the reason in glp_last_error() = rejected. */
GLP_API int glp_verify(const glp_circuit *circuit, const uint64_t *proof_words);
/* The same with the buffer length stated (num_words must equal glp_proof_words(circuit)): for callers that hold a proof of
 * unknown provenance; a wrong length is GLP_ERR_ARG, not a read past the buffer. */
GLP_API int glp_verify_n(const glp_circuit *circuit, const uint64_t *proof_words, size_t num_words);

/* `data.verify(proof)` for K proofs of one circuit, the query rounds on the GPU (a verifier for batch
 * self-checking behind glp_prove_batch; the reference proves and then verifies every proof [REF src/zkdsa/circuits/mod.rs:341-347,
 * src/ecdsa/gadgets/ecdsa.rs:349-352]).  Per proof, host threads run the transcript, the proof-of-work check and the
 * vanishing-polynomial identity at zeta; every FRI query round of every proof (Merkle paths of the four initial oracles and of each
 * commit-phase layer, `fri_combine_initial`, the arity-2^k consistency checks, the final polynomial) is one device launch over
 * K x num_query_rounds 16-lane groups.  Accepts and rejects exactly what glp_verify does, with the same reason.
 *   proofs       [K][glp_proof_words(circuit)], host memory
 *   status_out   [K]: GLP_OK = accepted, GLP_ERR_PROVE = rejected
 *   reasons_out  NULL, or [K][GLP_REASON_LEN] chars: the rejection reason of proof k (empty string if accepted)
 * Under PoseidonGoldilocksConfig the K transcripts run on the device too (the batch prover's kernels over the uploaded proofs); the host keeps
 * the canonical-form scan and the identity at zeta.  Environment variable GLP_VERIFY_HOST_TRANSCRIPT=1 (read per call): transcripts on host
 * threads, as under KeccakGoldilocksConfig.
 * Returns GLP_OK when the batch was checked (whatever the verdicts), an error code for bad arguments / HIP failures. */
GLP_API int glp_verify_batch(glp_ctx *ctx, const glp_circuit *circuit, uint32_t num_proofs, const uint64_t *proofs, int32_t *status_out,
                             char *reasons_out);

/* plonky2 `ProofWithPublicInputs::to_bytes()` (util/serialization.rs `Buffer::write_proof_with_public_inputs`):
 * every field element as 8 little-endian bytes in the word order above, plus the one-byte sibling
 * count that `write_merkle_proof` puts in front of every Merkle path.  This is the wire format the
 * reference round-trips at [REF src/ecdsa/gadgets/ecdsa.rs:298-316] for circuits and that a Rust
 * `ProofWithPublicInputs::from_bytes(bytes, &data.common)` consumes.  (Recalled format: not pinned by
 * a fixture, see DESIGN.md.) */
GLP_API size_t glp_proof_bytes_len(const glp_circuit *circuit);
GLP_API int glp_proof_to_bytes(const glp_circuit *circuit, const uint64_t *proof_words, uint8_t *bytes_out, size_t bytes_len);
GLP_API int glp_proof_from_bytes(const glp_circuit *circuit, const uint8_t *bytes, size_t bytes_len, uint64_t *proof_words_out);

#ifdef __cplusplus
}
#endif
#endif /* GLP_H */
