// verify_dev.h -- the query-round kernel of both GPU verifiers and its helpers: plonky2 `fri/verifier.rs::verify_fri_proof` from the
// initial Merkle paths to the final polynomial for any FriInstanceInfo (up to 8 oracles, up to 4 points, a range program), one
// 16-lane group per (proof, query): sums and flags across the group, verify_merkle_proof_to_cap on a group, the argument block
// (FVArgs), the status word (FV_*) and k_fri_verify_queries.  glp_verify_batch (verifier.hip) launches it on the plonk instance
// of a circuit, glp_fri_verify* (fri_verify.inc) on the caller's instance.  The per-proof table it reads is FT_* (prover_types.h).
#pragma once
#include "fri_shape.h"      // the status word, FV_*
#include "prover_types.h"

namespace {
using pos::shfl64;
using pos::shfl_xor64;
__device__ __forceinline__ ext2 group_sum(ext2 v) {         // sum over the 16 lanes of a group, result on every lane
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v = e_add(v, e_make(shfl_xor64(v.a, m), shfl_xor64(v.b, m)));
    return v;
}
__device__ __forceinline__ u32 group_or(u32 v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v |= (u32)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ u64 dvpow(u64 b, u64 e) {
    u64 r = 1;
    while (e) { if (e & 1) r = mul(r, b); b = sqr(b); e >>= 1; }
    return r;
}
// verify_merkle_proof_to_cap on one 16-lane group: true (on every lane of the group) if the leaf does NOT hash to the cap entry.
// Every lane of the wave must call it (shuffles); len, depth are the same for all groups of a launch.
template <int HASHER>
__device__ __forceinline__ bool merkle_bad(const u64 *leaf, u32 len, size_t index, const u64 *path, u32 depth, const u64 *cap, int l, int gb) {
    u32 bad = 0;
    if (HASHER == GLP_HASH_KECCAK25) {
        if (l == 0) {                                     // Keccak is 64-bit logic at full rate: one lane walks the path
            u64 cur[4] = {0, 0, 0, 0};
            if (8 * len <= 25) { for (u32 i = 0; i < len; i++) cur[i] = leaf[i]; }
            else {
                kec::Sponge sp;
                kec::sponge_init(sp);
                for (u32 i = 0; i < len; i++) kec::sponge_absorb(sp, leaf[i]);
                kec::sponge_finish(sp);
                kec::sponge_digest25(sp, cur);
            }
            for (u32 dd = 0; dd < depth; dd++) {
                u64 nxt[4];
                if (index & 1) kec::two_to_one(path + 4 * dd, cur, nxt); else kec::two_to_one(cur, path + 4 * dd, nxt);
                cur[0] = nxt[0]; cur[1] = nxt[1]; cur[2] = nxt[2]; cur[3] = nxt[3];
                index >>= 1;
            }
            for (int i = 0; i < 4; i++) bad |= cur[i] != cap[4 * index + i];
        }
    } else {
        u64 x = 0;
        if (len <= 4) x = (u32)l < len ? leaf[l] : 0;     // hash_or_noop: copied, zero padded
        else
            for (u32 c0 = 0; c0 < len; c0 += 8) {         // sponge, overwrite mode: lanes past the chunk keep their state
                if (l < 8 && c0 + (u32)l < len) x = leaf[c0 + l];
                x = pos::permute_coop(x, l, gb);
            }
        for (u32 dd = 0; dd < depth; dd++) {              // two_to_one(left, right) = permute(left || right || 0000)[0..4]
            const u64 sib = path[4 * dd + (l & 3)];
            const u64 cur = shfl64(x, gb + (l & 3));
            const bool right = index & 1;
            u64 nx = 0;
            if (l < 4) nx = right ? sib : cur; else if (l < 8) nx = right ? cur : sib;
            x = pos::permute_coop(nx, l, gb);
            index >>= 1;
        }
        if (l < 4) bad = x != cap[4 * index + l];
    }
    return group_or(bad) != 0;
}
__device__ __forceinline__ ext2 rd2(const u64 *p) { return e_make(p[0], p[1]); }

struct FVArgs {
    const u64 *proofs;      // [K][total]
    const u64 *table;       // [K][tstride]
    const u32 *prog;        // the range program, shared by all proofs: per range (leaf offset in the query record, col_begin, num_cols), points in order
    const u64 *caps[GLP_FRI_MAX_ORACLES];       // oracle o of proof k: caps[o] + k * cap_stride[o]
    u32 *status;            // [K][nq]
    size_t total, queries, query_stride, final_poly;
    u32 tstride, nq, K, lgN, cap_height, depth0, nred, final_len, nor, npts;
    u32 leaf_len[GLP_FRI_MAX_ORACLES], cap_stride[GLP_FRI_MAX_ORACLES];     // polynomials + salts; words from one proof's cap to the next's, 0 for a shared cap
    u32 nranges[GLP_FRI_MAX_POINTS];
    u32 ab[16], step_depth[16];
    u64 wN, gA[16];         // root_of_unity(lgN), root_of_unity(ab[r])
};

template <int HASHER>
__global__ __launch_bounds__(256) void k_fri_verify_queries(FVArgs a) {
    const int tid = threadIdx.x, l = tid & 15, lane = tid & 63, gb = lane & ~15;
    const size_t grp0 = (size_t)blockIdx.x * 16 + (tid >> 4), ngrp = (size_t)a.K * a.nq;
    const bool live = grp0 < ngrp;
    const size_t grp = live ? grp0 : 0;                   // idle groups redo group 0 (the shuffles need every lane) and write nothing
    const u32 k = (u32)(grp / a.nq), q = (u32)(grp % a.nq);
    const u64 *proof = a.proofs + (size_t)k * a.total, *tb = a.table + (size_t)k * a.tstride;
    const u64 *rec = proof + a.queries + (size_t)q * a.query_stride;
    const u64 *w = rec;
    size_t x_index = (size_t)tb[FT_XIDX + q];
    const ext2 alpha = rd2(tb + FT_ALPHA);
    const u32 capn4 = 4u << a.cap_height;
    u32 code = 0;
#define FV_FAIL(C, DETAIL) do { if (code == 0) code = (C) | ((u32)(DETAIL) << 8); } while (0)
    // ---- initial trees: the path covers the whole leaf, salts included; the evaluations stay where they are in the proof image
    for (u32 o = 0; o < a.nor; o++) {
        const u32 leaf_len = a.leaf_len[o];
        const u64 *cap = a.caps[o] + (size_t)k * a.cap_stride[o];
        if (merkle_bad<HASHER>(w, leaf_len, x_index, w + leaf_len, a.depth0, cap, l, gb)) FV_FAIL(FV_INITIAL, o);
        w += leaf_len + 4 * (size_t)a.depth0;
    }
    // ---- fri_combine_initial: sum <- sum alpha^(len_b) + (sum_j alpha^j eval_{b,j} - red_b) / (x - z_b), j across the point's ranges in order
    ext2 a16 = alpha;
#pragma unroll
    for (int i = 0; i < 4; i++) a16 = e_sqr(a16);
    const ext2 al = e_pow(alpha, (u64)l);
    u64 subgroup_x = mul(GEN, dvpow(a.wN, (u64)(__brevll((unsigned long long)x_index) >> (64 - a.lgN))));
    ext2 old_eval = e_from(0);
    {
        const u32 *pe = a.prog;
        for (u32 b = 0; b < a.npts; b++) {
            ext2 mine = e_from(0), off = e_from(1);       // this lane's share of sum_j alpha^j eval_j; alpha^(polynomials of the point so far)
            for (u32 i = 0; i < a.nranges[b]; i++, pe += 3) {
                const u32 ncols = pe[2];
                const u64 *ev = rec + pe[0] + pe[1];
                ext2 part = e_from(0);                    // lane l: sum_i ev[l + 16 i] (alpha^16)^i, Horner from the top
                if ((u32)l < ncols)
                    for (int j = (int)(((ncols - 1 - (u32)l) >> 4) << 4) + l; j >= 0; j -= 16) part = e_add(e_mul(part, a16), e_from(ev[j]));
                mine = e_add(mine, e_mul(off, part));
                off = e_mul(off, e_pow(alpha, (u64)ncols));
            }
            const ext2 r = group_sum(e_mul(mine, al));
            const ext2 d = e_sub(e_from(subgroup_x), rd2(tb + FT_Z + 2 * b));
            if (d.a == 0 && d.b == 0) FV_FAIL(FV_POINT, b);       // reject, never divide by zero
            old_eval = e_add(e_mul(old_eval, off), e_mul(e_sub(r, rd2(tb + FT_RED + 2 * b)), e_inv(d)));
        }
    }
    // ---- reductions: consistency with the previous layer, interpolation of the coset at beta, Merkle path of the layer
    for (u32 r = 0; r < a.nred; r++) {
        const u32 ab = a.ab[r], arity = 1u << ab;
        const u64 *ev = w, *path = w + 2 * (size_t)arity;
        const size_t coset_index = x_index >> ab, within = x_index & (arity - 1);
        if (!e_eq(rd2(ev + 2 * within), old_eval)) FV_FAIL(FV_FOLD, r);
        {   // compute_evaluation: sum_i vals_i prod_{j != i} (beta - p_j) / (p_i - p_j), p_j = coset_start gA^j; lane l takes i = l
            const u64 gA = a.gA[r];
            const u32 rw = (u32)(__brev((unsigned)within) >> (32 - ab));
            const u64 coset_start = mul(subgroup_x, dvpow(gA, (u64)(arity - rw)));
            const ext2 beta = rd2(tb + FT_BETAS + 2 * r);
            ext2 acc = e_from(0);
            for (u32 i = (u32)l; i < arity; i += 16) {
                const u64 pi = mul(coset_start, dvpow(gA, (u64)i));
                ext2 num = e_from(1);
                u64 den = 1, pj = coset_start;
                for (u32 j = 0; j < arity; j++) {
                    if (j != i) { num = e_mul(num, e_sub(beta, e_from(pj))); den = mul(den, sub(pi, pj)); }
                    pj = mul(pj, gA);
                }
                const u32 bi = (u32)(__brev((unsigned)i) >> (32 - ab));                   // reverse_index_bits(evals)
                acc = e_add(acc, e_scale(e_mul(rd2(ev + 2 * bi), num), glf::inv(den)));
            }
            old_eval = group_sum(acc);
        }
        const u64 *cap = proof + (size_t)r * capn4;
        if (merkle_bad<HASHER>(ev, 2 * arity, coset_index, path, a.step_depth[r], cap, l, gb)) FV_FAIL(FV_LAYER, r);
        for (u32 i = 0; i < ab; i++) subgroup_x = sqr(subgroup_x);
        x_index = coset_index;
        w += 2 * (size_t)arity + 4 * (size_t)a.step_depth[r];
    }
    {   // final_poly.eval(subgroup_x)
        ext2 acc = e_from(0);
        for (u32 i = a.final_len; i-- > 0;) acc = e_add(e_scale(acc, subgroup_x), rd2(proof + a.final_poly + 2 * (size_t)i));
        if (!e_eq(acc, old_eval)) FV_FAIL(FV_FINAL, 0);
    }
#undef FV_FAIL
    if (live && l == 0) a.status[grp] = code;
}
}  // namespace
