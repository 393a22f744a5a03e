// host_pool.h -- fork-join over persistent host threads: the K Fiat-Shamir transcripts of glp_prove_batch between two device stages,
// and the K transcripts + vanishing-polynomial checks of glp_verify_batch.  One pool per context, made on first use.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <sched.h>
#include <thread>
#include "common.h"

namespace glp {

// fork-join over [0, count) on persistent host threads (the transcripts of a batch between two device stages)
class HostPool {
public:
    explicit HostPool(unsigned nthreads) {
        for (unsigned t = 1; t < nthreads; t++) workers.emplace_back([this] { loop(); });
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> l(m); stop = true; }
        cv.notify_all();
        for (auto &w : workers) w.join();
    }
    void run(size_t count, const std::function<void(size_t)> &fn) {
        if (workers.empty() || count < 2) { for (size_t i = 0; i < count; i++) fn(i); return; }
        {
            std::lock_guard<std::mutex> l(m);
            job = &fn; total = count; next = 0; pending = workers.size(); gen++;
        }
        cv.notify_all();
        drain();
        std::unique_lock<std::mutex> l(m);
        done_cv.wait(l, [this] { return pending == 0; });
        job = nullptr;
    }
private:
    void drain() {
        for (;;) {
            size_t i;
            { std::lock_guard<std::mutex> l(m); if (!job || next >= total) return; i = next++; }
            (*job)(i);
        }
    }
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
            }
            drain();
            { std::lock_guard<std::mutex> l(m); if (--pending == 0) done_cv.notify_all(); }
        }
    }
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv, done_cv;
    const std::function<void(size_t)> *job = nullptr;
    size_t total = 0, next = 0, pending = 0;
    unsigned long long gen = 0;
    bool stop = false;
};

// Host threads for the transcripts of a batch: GLP_HOST_THREADS if set, else the cores this PROCESS may use -- the affinity
// mask capped by the cgroup CPU quota (a GPU box hands out one GPU's share of a large host; hardware_concurrency() reports
// the whole machine and every context has its own pool) -- at most 32.
inline unsigned usable_cores() {
    unsigned t = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int k = CPU_COUNT(&set); if (k > 0) t = std::min(t ? t : (unsigned)k, (unsigned)k); }
    auto read_two = [](const char *path, long long &a, long long &b) -> int {
        FILE *f = fopen(path, "r");
        if (!f) return 0;
        char s0[32] = {0};
        const int got = fscanf(f, "%31s %lld", s0, &b);
        fclose(f);
        if (got < 1 || strcmp(s0, "max") == 0) return -1;
        a = atoll(s0);
        return got;
    };
    long long quota = 0, period = 0;
    if (read_two("/sys/fs/cgroup/cpu.max", quota, period) == 2 && quota > 0 && period > 0) {          // cgroup v2: "<quota> <period>" or "max <period>"
        t = std::min<unsigned>(t, (unsigned)std::max<long long>(1, (quota + period / 2) / period));
    } else {
        long long q = 0, per = 0, dummy = 0;                                                          // cgroup v1
        if (read_two("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", q, dummy) >= 1 && read_two("/sys/fs/cgroup/cpu/cpu.cfs_period_us", per, dummy) >= 1 && q > 0 && per > 0)
            t = std::min<unsigned>(t, (unsigned)std::max<long long>(1, (q + per / 2) / per));
    }
    return std::max(1u, t);
}
inline unsigned host_threads() {
    unsigned t = usable_cores();
    if (const char *e = getenv("GLP_HOST_THREADS")) { const int v = atoi(e); if (v > 0) t = (unsigned)v; }
    return std::max(1u, std::min(t, 32u));
}

inline HostPool &ctx_host_pool(glp_ctx *c) {
    if (!c->host_pool) { c->host_pool = new HostPool(host_threads()); c->host_pool_free = [](void *q) { delete static_cast<HostPool *>(q); }; }
    return *static_cast<HostPool *>(c->host_pool);       // persistent: thread start-up costs more than a small batch
}

// first_noncanonical (host_check.h) of a large host array -- a witness, the input of a commitment -- in pieces on the context's host
// threads, so that the pass stays small beside the upload that follows.  One thread scans 4 MB in well under a millisecond: below a
// few pieces the fork-join would cost more than it saves.
inline size_t first_noncanonical_pooled(glp_ctx *c, const u64 *v, size_t count) {
    constexpr size_t PIECE = (size_t)1 << 19;            // words
    if (count < 4 * PIECE) return first_noncanonical(v, count);
    const size_t pieces = (count + PIECE - 1) / PIECE;
    std::vector<size_t> bad(pieces);
    ctx_host_pool(c).run(pieces, [&](size_t i) {
        const size_t i0 = i * PIECE, len = std::min(PIECE, count - i0);
        const size_t b = first_noncanonical(v + i0, len);
        bad[i] = b == len ? count : i0 + b;
    });
    return *std::min_element(bad.begin(), bad.end());
}
// A field array in the caller's host memory, [K][ncols][n] words (K == 0: no proof index; ncols == 0: no column index): every word
// canonical, or GLP_ERR_ARG naming the function, the parameter, the position and the value.  The rule of glp.h's conventions
// paragraph for host arrays; the callers run it before they allocate or launch anything.
inline int host_field_check(glp_ctx *c, const char *fn, const char *name, const u64 *v, size_t K, size_t ncols, size_t n) {
    const size_t count = (K ? K : 1) * (ncols ? ncols : 1) * n, bad = first_noncanonical_pooled(c, v, count);
    if (bad == count) return GLP_OK;
    char where[96];
    const size_t per_proof = (ncols ? ncols : 1) * n;
    int at = 0;
    if (K) at += snprintf(where + at, sizeof(where) - at, "proof %zu, ", bad / per_proof);
    if (ncols) at += snprintf(where + at, sizeof(where) - at, "column %zu, ", bad % per_proof / n);
    snprintf(where + at, sizeof(where) - at, "index %zu", bad % n);
    return set_error(GLP_ERR_ARG, "%s: %s: %s = 0x%016llx is not a canonical field element (>= p)", fn, name, where, (unsigned long long)v[bad]);
}
}  // namespace glp
