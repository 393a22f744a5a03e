// common.h -- context, device-memory pool, error plumbing and stage timers shared by the
// translation units of libglprover.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../include/glp.h"
#include "glf.h"
#include "host_check.h"    // set_error, GLP_TRY, GLP_REQUIRE, first_noncanonical

namespace glp {

extern thread_local std::string g_last_error;

#define GLP_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return glp::set_error(GLP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                  __FILE__, __LINE__);                                         \
    } while (0)

struct NttPlan;
struct LdePlan;

struct Stage {
    std::string name;
    hipEvent_t beg, end;
    double bytes;
};

}  // namespace glp

struct glp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;   // host->device witness chunks, overlapped with the transforms of earlier chunks
    int num_cus = 256;
    // size-keyed free lists: commit buffers are GB-sized and recur with identical sizes every proof
    std::multimap<size_t, void *> pool;
    std::map<void *, size_t> live;
    size_t pool_bytes = 0;
    bool pool_poison = false;            // GLP_POOL_POISON = 0..255: alloc and release fill the block with that byte (a test switch; api.hip)
    int pool_poison_byte = 0;
    std::map<int, glp::NttPlan *> ntt_plans;                       // key: log_n
    std::map<std::pair<std::pair<int, int>, u64>, glp::LdePlan *> lde_plans;  // key: ((log_n, rate_bits), shift)
    unsigned long long lde_clock = 0;                              // LRU stamps for lde_plans
    int two_pass_lg = 22;                // largest log_n transformed in two passes (ntt.h NTT_2PASS_LG; GLP_NTT_2PASS_LG overrides, 20..22)
    int strided32_tl = 8;                // tiles (planes) a k_strided32 block walks, software-pipelined (GLP_NTT_STRIDED32_TL: 1..64; 1 = no pipelining)
    int strided32_lw = 4;                // log2 columns of a k_strided32 tile (GLP_NTT_STRIDED32_LW: 3 = 64-byte row segments, 4 = 128-byte)
    size_t merkle_coop_max = 4096;       // leaf hash: up to this many leaves per launch one leaf per 16-lane group (GLP_MERKLE_COOP_MAX), ...
    size_t merkle_quad_max = 32768;      // ... up to this many one leaf per quad of lanes (GLP_MERKLE_QUAD_MAX), above it one leaf per lane (merkle.hip)
    void *host_pool = nullptr;           // HostPool of prover_batch.inc (host threads for the transcripts of a batch), made on first use
    void (*host_pool_free)(void *) = nullptr;
    bool profiling = false;
    std::vector<glp::Stage> stages;
    bool salt_seed_fixed = false;        // glp_ctx_set_salt_seed: a fixed seed for every zk proof, else a fresh OS seed per call
    u64 salt_seed[4] = {0, 0, 0, 0};

    int alloc(void **p, size_t bytes);
    void release(void *p);
    void trim();
    int stage_begin(const char *name, double bytes);
    int stage_end();
};

namespace glp {
struct StageScope {
    glp_ctx *c;
    StageScope(glp_ctx *ctx, const char *name, double bytes) : c(ctx) { c->stage_begin(name, bytes); }
    ~StageScope() { c->stage_end(); }
};
// the salt seed of one zk proof or batch call: the context's fixed seed, or 4 fresh words from getrandom, reduced mod p (api.hip)
int salt_seed_draw(glp_ctx *c, u64 out[4]);
inline int bind(glp_ctx *c) {
    hipError_t e = hipSetDevice(c->device);
    return e == hipSuccess ? GLP_OK : set_error(GLP_ERR_HIP, "hipSetDevice(%d): %s", c->device, hipGetErrorString(e));
}
// Synchronising copies: the host side is usually a stack or std::vector temporary that must not outlive the copy.
inline int d2h(glp_ctx *c, void *dst, const void *src, size_t bytes) {
    GLP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}
inline int h2d(glp_ctx *c, void *dst, const void *src, size_t bytes) {
    GLP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}
// The pool blocks of one call: released, once the stream has drained, however the call returns.  Sizes are counts of elements,
// never bytes: words() counts 64-bit words, array() elements of T.
struct Scratch {
    glp_ctx *c;
    std::vector<void *> ptrs;
    explicit Scratch(glp_ctx *ctx) : c(ctx) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() {
        if (ptrs.empty()) return;           // nothing to release: a call on the caller's own device buffers stays asynchronous
        (void)hipStreamSynchronize(c->stream);
        for (void *p : ptrs) c->release(p);
    }
    template <class T> int array(T **p, size_t count) {
        void *v = nullptr;
        GLP_TRY(c->alloc(&v, count * sizeof(T)));
        ptrs.push_back(v);
        *p = (T *)v;
        return GLP_OK;
    }
    int words(u64 **p, size_t count) { return array(p, count); }
    // host or device input -> a device pointer: the caller's own, or a block of this scratch filled from the host.  The copy is
    // asynchronous on the ctx stream: `in` is a caller's buffer that outlives the call (h2d above for stack and vector sources).
    int input(const u64 *in, int on_device, size_t count, const u64 **dev) {
        if (on_device) { *dev = in; return GLP_OK; }
        u64 *d;
        GLP_TRY(words(&d, count));
        GLP_HIP(hipMemcpyAsync(d, in, count * 8, hipMemcpyHostToDevice, c->stream));
        *dev = d;
        return GLP_OK;
    }
};
}  // namespace glp
