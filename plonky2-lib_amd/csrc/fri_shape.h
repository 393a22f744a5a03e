// fri_shape.h -- the shape rules of a FriInstanceInfo and its FriParams, one set for the prover (fri_check in fri_openings.inc,
// which adds what only a glp_batch can answer) and the verifier (fri_verify.inc, which holds caps and no batch); the word layout of
// a FriProof, one statement for the plonk proof (make_layout, circuit_common.h), the prover's handle (glp_fri, fri_openings.inc) and
// the verifier's plan (fv_plan, fri_verify.inc); and the status word of a query round, which the kernel (verify_dev.h) and the host
// restatement (verify_host.h) both speak.  Host only, no context.  A change to the proof format belongs in fri_proof_layout and in
// binding.fri_proof_words, the caller-side restatement.
#pragma once
#include "host_check.h"

namespace glp {
// One bound for glp_circuit_create, glp_pow_search and the FRI descriptions: with the search capped at 2^40 candidates, 32 bits
// leaves a failure probability of exp(-2^8).
constexpr u32 POW_MAX_BITS = 32;

// status word of one (proof, query): 0 = accepted, else check | detail << 8 (detail: oracle for 4, point for 3, reduction for 5 and 6);
// the check numbers are those of tests/fri_restate.py::verify_fri_proof
constexpr u32 FV_POINT = 3, FV_INITIAL = 4, FV_FOLD = 5, FV_LAYER = 6, FV_FINAL = 7;

// One FriProof in words: the caps of the reduction layers | per query round the initial leaves and paths of every oracle, then per
// reduction the 2^arity evaluations (ext) and the path of its layer | the final polynomial (ext) | the proof-of-work witness.
// Offsets count from the first layer cap; leaf_off[o] is where oracle o's leaf starts inside a query record.  The shape rules above
// have held for the arguments: the sums and shifts here cannot wrap.
struct FriProofLayout {
    u32 depth0 = 0, step_depth[16] = {0}, final_len = 0;
    size_t leaf_off[GLP_FRI_MAX_ORACLES] = {0}, query_stride = 0, queries = 0, final_poly = 0, pow = 0, total = 0;
};
inline FriProofLayout fri_proof_layout(u32 lgN, u32 rate_bits, u32 cap_height, const u32 *leaf_len, u32 num_oracles, const u32 *arity_bits,
                                       u32 num_reductions, u32 num_query_rounds) {
    FriProofLayout f;
    f.depth0 = lgN - cap_height;
    size_t q = 0;
    for (u32 o = 0; o < num_oracles; o++) { f.leaf_off[o] = q; q += leaf_len[o] + 4 * (size_t)f.depth0; }
    u32 lg = lgN;
    for (u32 r = 0; r < num_reductions; r++) {
        lg -= arity_bits[r];
        f.step_depth[r] = lg - cap_height;
        q += 2 * ((size_t)1 << arity_bits[r]) + 4 * (size_t)f.step_depth[r];
    }
    f.query_stride = q;
    f.final_len = 1u << (lg - rate_bits);
    f.queries = (size_t)num_reductions * ((size_t)4 << cap_height);
    f.final_poly = f.queries + q * num_query_rounds;
    f.pow = f.final_poly + 2 * (size_t)f.final_len;
    f.total = f.pow + 1;
    return f;
}

inline int fri_shape_counts(u32 num_oracles, const void *oracles, u32 num_points, const glp_fri_point *points) {
    GLP_REQUIRE(num_oracles >= 1 && num_oracles <= GLP_FRI_MAX_ORACLES, "num_oracles = %u outside 1..%d", num_oracles, GLP_FRI_MAX_ORACLES);
    GLP_REQUIRE(oracles, "oracles is null");
    GLP_REQUIRE(num_points >= 1 && num_points <= GLP_FRI_MAX_POINTS, "num_points = %u outside 1..%d", num_points, GLP_FRI_MAX_POINTS);
    GLP_REQUIRE(points, "points is null");
    return GLP_OK;
}
// ncols[o]: polynomials of oracle o (salts are not polynomials); lg = log_n.  points_canonical: also require canonical .point words,
// for a caller that reads its points from the description.  No caller sets it today: the prover (fri_check) and the verifier take
// their points from an array [K][num_points][2] and check that.
inline int fri_shape_rules(const u32 *ncols, u32 num_oracles, u32 lg, u32 rate_bits, u32 cap_height, u32 num_points, const glp_fri_point *points,
                           bool points_canonical, u32 num_reductions, const u32 *arity_bits, u32 proof_of_work_bits, u32 num_query_rounds) {
    const u32 lgN = lg + rate_bits;
    size_t nopen = 0;
    for (u32 p = 0; p < num_points; p++) {
        const glp_fri_point &pt = points[p];
        GLP_REQUIRE(pt.num_ranges <= GLP_FRI_MAX_RANGES, "points[%u].num_ranges = %u above %d", p, pt.num_ranges, GLP_FRI_MAX_RANGES);
        GLP_REQUIRE(pt.ranges || pt.num_ranges == 0, "points[%u].ranges is null", p);
        GLP_REQUIRE(!points_canonical || (pt.point[0] < glf::P && pt.point[1] < glf::P), "points[%u].point is not canonical", p);
        size_t len = 0;
        for (u32 r = 0; r < pt.num_ranges; r++) {
            const glp_fri_range &rg = pt.ranges[r];
            GLP_REQUIRE(rg.oracle < num_oracles, "points[%u].ranges[%u].oracle = %u, there are %u oracles", p, r, rg.oracle, num_oracles);
            const u32 nc = ncols[rg.oracle];
            GLP_REQUIRE(rg.col_begin <= nc && rg.num_cols <= nc - rg.col_begin,
                        "points[%u].ranges[%u]: columns [%u, %u + %u) run past ncols = %u of oracle %u (salts are not polynomials)", p, r, rg.col_begin,
                        rg.col_begin, rg.num_cols, nc, rg.oracle);
            len += rg.num_cols;
        }
        GLP_REQUIRE(len > 0, "points[%u] names no polynomial", p);
        GLP_REQUIRE((nopen += len) <= 0x7FFFFFFFu, "points name too many polynomials");
    }
    GLP_REQUIRE(num_reductions <= 16, "num_reductions = %u above 16", num_reductions);
    u32 sum_ab = 0;
    for (u32 i = 0; i < num_reductions; i++) {
        GLP_REQUIRE(arity_bits[i] >= 1 && arity_bits[i] <= 4, "reduction_arity_bits[%u] = %u outside 1..4", i, arity_bits[i]);
        sum_ab += arity_bits[i];
    }
    GLP_REQUIRE(sum_ab <= lg, "reduction_arity_bits sum to %u, above log_n = %u", sum_ab, lg);
    GLP_REQUIRE(lgN - sum_ab >= cap_height, "reduction_arity_bits: the last layer has fewer leaves than the cap (cap_height = %d)", (int)cap_height);
    GLP_REQUIRE(proof_of_work_bits <= POW_MAX_BITS, "proof_of_work_bits=%u: this build searches at most 2^40 candidates and accepts up to %u bits",
                proof_of_work_bits, POW_MAX_BITS);
    GLP_REQUIRE(num_query_rounds >= 1, "num_query_rounds = 0");
    return GLP_OK;
}
}  // namespace glp
