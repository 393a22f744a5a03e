// verify_dev.h -- device helpers of the query-round kernels (k_verify_queries in verifier.hip, k_fri_verify_queries in
// fri_verify.inc): one 16-lane group per (proof, query), sums and flags across the group, verify_merkle_proof_to_cap on a group.
#pragma once
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
}  // namespace
