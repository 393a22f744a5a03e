// api.hip -- the extern "C" boundary of libglprover.so (declared in include/glp.h): context,
// device-memory pool, stage timers, primitive entry points and PolynomialBatch.
#include <stdarg.h>
#include <errno.h>
#include <sys/random.h>
#include <string.h>
#include "batch.h"
#include "common.h"
#include "host_pool.h"   // host_field_check: the canonical-form scan of host field arrays
#include "keccak.h"
#include "merkle.h"
#include "ntt.h"

namespace glp {
thread_local std::string g_last_error;
int set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
}  // namespace glp
using namespace glp;

// ------------------------------------------------------------------------------------------ ctx
// GLP_POOL_POISON: every byte of a block is the poison byte when it is handed out and again when it comes back, so no kernel's
// result can rest on what a fresh hipMalloc block or the block's last user happened to hold.  Only `stream` is drained, never
// copy_stream: the fill must not order the two streams for a caller that forgot to.
static int poison_fill(glp_ctx *c, void *p, size_t bytes) {
    GLP_HIP(hipMemsetAsync(p, c->pool_poison_byte, bytes, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}
int glp_ctx::alloc(void **p, size_t bytes) {
    if (bytes == 0) bytes = 8;
    bytes = (bytes + 255) & ~(size_t)255;
    auto it = pool.find(bytes);
    if (it != pool.end()) {
        *p = it->second;
        pool.erase(it);
        pool_bytes -= bytes;
        live[*p] = bytes;
        return pool_poison ? poison_fill(this, *p, bytes) : GLP_OK;
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        trim();  // drop cached blocks of other sizes and retry once
        e = hipMalloc(p, bytes);
    }
    if (e != hipSuccess) return set_error(GLP_ERR_HIP, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    live[*p] = bytes;
    return pool_poison ? poison_fill(this, *p, bytes) : GLP_OK;
}
void glp_ctx::release(void *p) {
    if (!p) return;
    auto it = live.find(p);
    if (it == live.end()) return;
    if (pool_poison) (void)poison_fill(this, p, it->second);  // the callers have drained the stream: a reader that outlives the release sees poison
    pool.insert({it->second, p});
    pool_bytes += it->second;
    live.erase(it);
}
void glp_ctx::trim() {
    (void)hipStreamSynchronize(stream);
    for (auto &kv : pool) (void)hipFree(kv.second);
    pool.clear();
    pool_bytes = 0;
}
int glp_ctx::stage_begin(const char *name, double bytes) {
    if (!profiling) return GLP_OK;
    Stage s;
    s.name = name; s.bytes = bytes;
    if (hipEventCreate(&s.beg) != hipSuccess || hipEventCreate(&s.end) != hipSuccess) return GLP_ERR_HIP;
    (void)hipEventRecord(s.beg, stream);
    stages.push_back(s);
    return GLP_OK;
}
int glp_ctx::stage_end() {
    if (!profiling || stages.empty()) return GLP_OK;
    (void)hipEventRecord(stages.back().end, stream);
    return GLP_OK;
}

extern "C" {

const char *glp_last_error(void) { return g_last_error.c_str(); }
const char *glp_version(void) { return "glprover 0.1 (gfx950)"; }

int glp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int glp_ctx_create(int device_id, glp_ctx **out) {
    GLP_REQUIRE(out != nullptr, "glp_ctx_create: out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return set_error(GLP_ERR_NOGPU, "no HIP device visible (%s); libglprover has no CPU fallback",
                         e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    GLP_REQUIRE(device_id >= 0 && device_id < n, "device_id %d out of range (0..%d)", device_id, n - 1);
    GLP_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    GLP_HIP(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_error(GLP_ERR_NOGPU, "device %d is %s; this library carries gfx950 code objects only", device_id,
                         prop.gcnArchName);
    std::unique_ptr<glp_ctx> c(new glp_ctx());
    c->device = device_id;
    c->num_cus = prop.multiProcessorCount;
    GLP_TRY(ntt_init_device(c.get()));
    // tuning switches (profiles/ A-B runs; documented in include/glp.h): the defaults are what ships
    if (const char *e1 = getenv("GLP_NTT_2PASS_LG")) { const int v = atoi(e1); if (v >= NTT_INNER_LG && v <= NTT_2PASS_LG) c->two_pass_lg = v; }
    if (const char *e2 = getenv("GLP_NTT_STRIDED32_TL")) { const int v = atoi(e2); if (v >= 1 && v <= 64) c->strided32_tl = v; }
    if (const char *e3 = getenv("GLP_NTT_STRIDED32_LW")) { const int v = atoi(e3); if (v == 3 || v == 4) c->strided32_lw = v; }
    if (const char *e4 = getenv("GLP_MERKLE_COOP_MAX")) c->merkle_coop_max = (size_t)strtoull(e4, nullptr, 10);
    if (const char *e5 = getenv("GLP_MERKLE_QUAD_MAX")) c->merkle_quad_max = (size_t)strtoull(e5, nullptr, 10);
    if (const char *e6 = getenv("GLP_POOL_POISON")) {
        char *end = nullptr;
        const long v = strtol(e6, &end, 10);
        if (end != e6 && *end == 0 && v >= 0 && v <= 255) { c->pool_poison = true; c->pool_poison_byte = (int)v; }
    }
    GLP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    {
        hipError_t e2 = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
        if (e2 != hipSuccess) {
            (void)hipStreamDestroy(c->stream);
            return set_error(GLP_ERR_HIP, "hipStreamCreateWithFlags (copy stream): %s", hipGetErrorString(e2));
        }
    }
    *out = c.release();
    return GLP_OK;
}

void glp_ctx_destroy(glp_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    glp_ctx_stage_reset(c);
    if (c->host_pool && c->host_pool_free) c->host_pool_free(c->host_pool);
    free_plans(c);
    c->trim();
    for (auto &kv : c->live) (void)hipFree(kv.first);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int glp_ctx_synchronize(glp_ctx *c) {
    GLP_REQUIRE(c, "null ctx");
    GLP_TRY(bind(c));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}
void *glp_ctx_stream(glp_ctx *c) { return c ? (void *)c->stream : nullptr; }

int glp_dev_alloc(glp_ctx *c, size_t bytes, void **dev_out) {
    GLP_REQUIRE(c && dev_out && bytes > 0, "null argument or zero size");
    *dev_out = nullptr;
    GLP_TRY(bind(c));
    return c->alloc(dev_out, bytes);
}
int glp_dev_free(glp_ctx *c, void *dev) {
    GLP_REQUIRE(c, "null context");
    if (!dev) return GLP_OK;
    GLP_TRY(bind(c));
    GLP_REQUIRE(c->live.count(dev), "pointer was not allocated by glp_dev_alloc on this context");
    GLP_HIP(hipStreamSynchronize(c->stream));
    c->release(dev);
    return GLP_OK;
}
// the live block of this context that contains [p, p + bytes), or an error: a copy never runs past an allocation
static int check_dev_range(glp_ctx *c, const void *p, size_t bytes) {
    auto it = c->live.upper_bound(const_cast<void *>(p));
    GLP_REQUIRE(it != c->live.begin(), "device pointer is not inside an allocation of this context");
    --it;
    const char *b0 = (const char *)it->first, *q = (const char *)p;
    GLP_REQUIRE(q >= b0 && (size_t)(q - b0) <= it->second && bytes <= it->second - (size_t)(q - b0),
                "%zu bytes at offset %zu run past the end of a %zu-byte device block", bytes, (size_t)(q - b0), it->second);
    return GLP_OK;
}
int glp_dev_upload(glp_ctx *c, void *dev_dst, const void *host_src, size_t bytes) {
    GLP_REQUIRE(c && dev_dst && host_src, "null argument");
    GLP_TRY(bind(c));
    GLP_TRY(check_dev_range(c, dev_dst, bytes));
    GLP_HIP(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}
int glp_dev_download(glp_ctx *c, void *host_dst, const void *dev_src, size_t bytes) {
    GLP_REQUIRE(c && host_dst && dev_src, "null argument");
    GLP_TRY(bind(c));
    GLP_TRY(check_dev_range(c, dev_src, bytes));
    GLP_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}
int glp_ctx_set_profiling(glp_ctx *c, int on) {
    GLP_REQUIRE(c, "null ctx");
    c->profiling = on != 0;
    return GLP_OK;
}
int glp_ctx_stage_reset(glp_ctx *c) {
    GLP_REQUIRE(c, "null ctx");
    (void)hipStreamSynchronize(c->stream);
    for (auto &s : c->stages) { (void)hipEventDestroy(s.beg); (void)hipEventDestroy(s.end); }
    c->stages.clear();
    return GLP_OK;
}
int glp_ctx_stage_count(glp_ctx *c) { return c ? (int)c->stages.size() : 0; }
int glp_ctx_stage_get(glp_ctx *c, int index, const char **name, float *ms, double *bytes) {
    GLP_REQUIRE(c && index >= 0 && index < (int)c->stages.size(), "stage index out of range");
    Stage &s = c->stages[index];
    GLP_HIP(hipEventSynchronize(s.end));
    float t = 0;
    GLP_HIP(hipEventElapsedTime(&t, s.beg, s.end));
    if (name) *name = s.name.c_str();
    if (ms) *ms = t;
    if (bytes) *bytes = s.bytes;
    return GLP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ primitives
// What the primitive entry points share: `in` goes up into a block of the call's scratch, `run(scratch, dev_in, &dev_result)`
// transforms it (in further blocks of that scratch, if it needs them) and names where the result is, and that comes back into `out`.
template <class F>
static int on_device_copy(glp_ctx *c, const u64 *in, size_t in_words, u64 *out, size_t out_words, F run) {
    Scratch s(c);
    u64 *a, *res = nullptr;
    GLP_TRY(s.words(&a, in_words));
    GLP_HIP(hipMemcpyAsync(a, in, in_words * 8, hipMemcpyHostToDevice, c->stream));
    GLP_TRY(run(s, a, &res));
    return d2h(c, out, res, out_words * 8);
}

extern "C" {

int glp_poseidon_permute(glp_ctx *c, uint64_t *states, size_t count) {
    GLP_REQUIRE(c && (states || !count), "null argument");
    GLP_TRY(bind(c));
    if (!count) return GLP_OK;
    {
        const size_t bad = first_noncanonical_pooled(c, states, count * 12);
        GLP_REQUIRE(bad == count * 12, "glp_poseidon_permute: states: state %zu, index %zu = 0x%016llx is not a canonical field element (>= p)", bad / 12,
                    bad % 12, (unsigned long long)states[bad == count * 12 ? 0 : bad]);
    }
    return on_device_copy(c, states, count * 12, states, count * 12, [&](Scratch &, u64 *a, u64 **res) {
        *res = a;
        return poseidon_permute_states(c, a, count);
    });
}

int glp_fft(glp_ctx *c, uint64_t *cols, uint32_t ncols, uint32_t log_n) {
    GLP_REQUIRE(c && (cols || !ncols), "null argument");
    GLP_TRY(bind(c));
    if (!ncols) return GLP_OK;
    if (log_n > (uint32_t)NTT_MAX_LG) return set_error(GLP_ERR_UNSUPPORTED, "log_n=%u > %d", log_n, NTT_MAX_LG);
    const size_t tot = (size_t)ncols << log_n;
    GLP_TRY(host_field_check(c, "glp_fft", "cols", cols, 0, ncols, (size_t)1 << log_n));
    return on_device_copy(c, cols, tot, cols, tot, [&](Scratch &s, u64 *a, u64 **res) {
        u64 *b;
        GLP_TRY(s.words(&b, tot));
        GLP_TRY(bitrev_copy(c, a, b, ncols, (int)log_n));
        *res = a;
        return ntt_coeffs_to_values(c, b, a, ncols, (int)log_n);
    });
}

int glp_ifft(glp_ctx *c, uint64_t *cols, uint32_t ncols, uint32_t log_n) {
    GLP_REQUIRE(c && (cols || !ncols), "null argument");
    GLP_TRY(bind(c));
    if (!ncols) return GLP_OK;
    if (log_n > (uint32_t)NTT_MAX_LG) return set_error(GLP_ERR_UNSUPPORTED, "log_n=%u > %d", log_n, NTT_MAX_LG);
    const size_t tot = (size_t)ncols << log_n;
    GLP_TRY(host_field_check(c, "glp_ifft", "cols", cols, 0, ncols, (size_t)1 << log_n));
    return on_device_copy(c, cols, tot, cols, tot, [&](Scratch &s, u64 *a, u64 **res) {
        u64 *b;
        GLP_TRY(s.words(&b, tot));
        GLP_TRY(intt_values_to_coeffs(c, a, b, ncols, (int)log_n));
        *res = a;
        return bitrev_copy(c, b, a, ncols, (int)log_n);
    });
}

int glp_lde(glp_ctx *c, const uint64_t *coeffs, uint32_t ncols, uint32_t log_n, uint32_t rate_bits, uint64_t shift,
            uint64_t *out) {
    GLP_REQUIRE(c && ((coeffs && out) || !ncols), "null argument");
    GLP_REQUIRE(shift != 0 && shift < glf::P, "shift must be a nonzero canonical field element");
    if (rate_bits > 4) return set_error(GLP_ERR_UNSUPPORTED, "rate_bits=%u outside 0..4", rate_bits);
    GLP_TRY(bind(c));
    if (!ncols) return GLP_OK;
    if (log_n > (uint32_t)NTT_MAX_LG) return set_error(GLP_ERR_UNSUPPORTED, "log_n=%u > %d", log_n, NTT_MAX_LG);
    const size_t tot = (size_t)ncols << log_n, TOT = tot << rate_bits;
    GLP_TRY(host_field_check(c, "glp_lde", "coeffs", coeffs, 0, ncols, (size_t)1 << log_n));
    return on_device_copy(c, coeffs, tot, out, TOT, [&](Scratch &s, u64 *a, u64 **res) {
        u64 *b, *l;
        GLP_TRY(s.words(&b, tot));
        GLP_TRY(s.words(&l, TOT));
        GLP_TRY(s.words(res, TOT));
        GLP_TRY(bitrev_copy(c, a, b, ncols, (int)log_n));
        GLP_TRY(lde_coeffs(c, b, l, ncols, (int)log_n, (int)rate_bits, shift));
        return lde_to_natural(c, l, *res, ncols, (int)log_n, (int)rate_bits);
    });
}

// PolynomialValues::coset_ifft(shift): the transform of glp_batch_from_coset_values at one plane (sub_bits = 0), on its own
int glp_coset_ifft(glp_ctx *c, uint64_t *cols, uint32_t ncols, uint32_t log_n, uint64_t shift) {
    GLP_REQUIRE(c && (cols || !ncols), "null argument");
    GLP_REQUIRE(shift != 0 && shift < glf::P, "shift must be a nonzero canonical field element");
    GLP_TRY(bind(c));
    if (!ncols) return GLP_OK;
    if (log_n > (uint32_t)NTT_MAX_LG) return set_error(GLP_ERR_UNSUPPORTED, "log_n=%u > %d", log_n, NTT_MAX_LG);
    const size_t tot = (size_t)ncols << log_n;
    GLP_TRY(host_field_check(c, "glp_coset_ifft", "cols", cols, 0, ncols, (size_t)1 << log_n));
    return on_device_copy(c, cols, tot, cols, tot, [&](Scratch &s, u64 *a, u64 **res) {
        u64 *b;
        GLP_TRY(s.words(&b, tot));
        GLP_TRY(coset_planes_to_chunk_coeffs(c, a, b, b, ncols, (int)log_n, 0, shift));
        *res = a;
        return bitrev_copy(c, b, a, ncols, (int)log_n);
    });
}

}  // extern "C"

__global__ void k_fill_random(u64 *out, size_t count, u64 seed) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    u64 z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    out[i] = glf::canon(z);
}

// one message per thread, bytes packed into lanes on the fly
__global__ void k_keccak256(const uint8_t *msgs, size_t count, size_t len, uint8_t *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint8_t *m = msgs + i * len;
    kec::Sponge s;
    kec::sponge_init(s);
    size_t off = 0;
    for (; off + 8 <= len; off += 8) {
        u64 lane = 0;
        for (int b = 0; b < 8; b++) lane |= (u64)m[off + b] << (8 * b);
        kec::sponge_absorb(s, lane);
    }
    u64 extra = 0;
    for (size_t b = 0; off + b < len; b++) extra |= (u64)m[off + b] << (8 * b);
    kec::sponge_finish(s, extra, (int)(len - off));
    for (int w = 0; w < 4; w++) for (int b = 0; b < 8; b++) out[i * 32 + 8 * w + b] = (uint8_t)(s.a[w] >> (8 * b));
}
extern "C" int glp_keccak256(glp_ctx *c, const uint8_t *msgs, size_t count, size_t len, uint8_t *digests_out) {
    GLP_REQUIRE(c && digests_out && (msgs || !len), "null argument");
    GLP_REQUIRE(len == 0 || count <= ((size_t)1 << 40) / len, "count * len = %zu * %zu bytes is more than this entry point stages (2^40)", count, len);
    GLP_TRY(bind(c));
    if (!count) return GLP_OK;
    Scratch s(c);
    u64 *dm, *dd;
    GLP_TRY(s.words(&dm, (count * len + 7) / 8 + 1));
    GLP_TRY(s.words(&dd, count * 4));
    if (len) GLP_HIP(hipMemcpyAsync(dm, msgs, count * len, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_keccak256, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, c->stream, (const uint8_t *)dm, count, len, (uint8_t *)dd);
    GLP_HIP(hipGetLastError());
    GLP_HIP(hipMemcpyAsync(digests_out, dd, count * 32, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

namespace glp {
int salt_seed_draw(glp_ctx *c, u64 out[4]) {
    if (c->salt_seed_fixed) { memcpy(out, c->salt_seed, 32); return GLP_OK; }
    u64 w[4];
    size_t got = 0;
    while (got < sizeof(w)) {
        const ssize_t r = getrandom(reinterpret_cast<char *>(w) + got, sizeof(w) - got, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return set_error(GLP_ERR_PROVE, "getrandom failed (errno %d): no salt seed for a zero-knowledge proof", errno);
        }
        got += (size_t)r;
    }
    for (int i = 0; i < 4; i++) out[i] = glf::canon(w[i]);
    return GLP_OK;
}
}  // namespace glp

extern "C" int glp_ctx_set_salt_seed(glp_ctx *c, const uint64_t seed[4]) {
    GLP_REQUIRE(c, "null context");
    c->salt_seed_fixed = seed != nullptr;
    for (int i = 0; i < 4; i++) c->salt_seed[i] = seed ? glf::canon(seed[i]) : 0;
    return GLP_OK;
}

extern "C" int glp_fill_random_device(glp_ctx *c, uint64_t *dev_out, size_t count, uint64_t seed) {
    GLP_REQUIRE(c && (dev_out || !count), "null argument");
    GLP_TRY(bind(c));
    if (!count) return GLP_OK;
    hipLaunchKernelGGL(k_fill_random, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, dev_out, count, seed);
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}

// ------------------------------------------------------------------------------------------ PolynomialBatch

namespace glp {

void batch_destroy(glp_batch *b) {
    if (!b) return;
    if (b->view) { delete b; return; }
    glp_ctx *c = b->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->release(b->coeffs);
    c->release(b->lde);
    c->release(b->digests);
    delete b;
}

int batch_shape_check(const char *fn, u32 K, size_t ncols, u32 log_n, u32 rate_bits, u32 cap_height, u32 hasher, size_t max_bytes) {
    const std::string at = fn ? std::string(fn) + ": " : std::string();
    const char *p = at.c_str();
    GLP_REQUIRE(K >= 1 && K <= 65535, "%sbatch of %u trees outside 1..65535", p, K);
    if (log_n > (u32)NTT_MAX_LG) return set_error(GLP_ERR_UNSUPPORTED, "%slog_n=%u > %d", p, log_n, NTT_MAX_LG);
    GLP_REQUIRE(rate_bits <= 4, "%srate_bits=%u outside 0..4", p, rate_bits);
    GLP_REQUIRE(cap_height <= log_n + rate_bits, "%scap_height=%u should be at most log2(leaves)=%u", p, cap_height, log_n + rate_bits);
    GLP_REQUIRE(ncols > 0, "%sncols must be positive", p);
    GLP_REQUIRE(ncols <= 0x7FFFFFFFu / K, "%sbatch too wide (num_proofs * ncols = %u * %zu columns)", p, K, ncols);
    GLP_REQUIRE(!max_bytes || (size_t)K * ncols <= max_bytes >> (3 + log_n + rate_bits),
                "%sbatch too large (num_proofs * ncols * 2^(log_n + rate_bits) words)", p);
    if (hasher != GLP_HASH_POSEIDON && hasher != GLP_HASH_KECCAK25) return set_error(GLP_ERR_UNSUPPORTED, "%shasher %u is not one of GLP_HASH_*", p, hasher);
    return GLP_OK;
}

// dev_in [K * ncols][n]: values in natural order (BATCH_VALUES), or coefficients in natural or bit-reversed order.
// host_src != nullptr (BATCH_VALUES, K = 1): the values are still in host memory; they are copied into dev_in in column
// chunks on the copy stream while the transforms of the chunks already on the device run on the compute stream.
int batch_build(glp_ctx *c, const u64 *dev_in, int input_kind, u32 ncols, int lg, int rate_bits, int cap_height,
                glp_batch **out, const u64 *host_src, u32 K, int hasher, const u64 *salt_seed, u32 salt_tag) {
    GLP_REQUIRE(out, "out is null");
    *out = nullptr;
    GLP_TRY(batch_shape_check(nullptr, K, ncols, (u32)lg, (u32)rate_bits, (u32)cap_height, (u32)hasher));
    GLP_REQUIRE(host_src == nullptr || (K == 1 && input_kind == BATCH_VALUES), "bad batch arguments");
    // K oracles of one shape: the transforms see K * ncols independent columns, the salts and the trees get a proof index
    const size_t n = (size_t)1 << lg, N = n << rate_bits, tot = (size_t)K * ncols;
    std::unique_ptr<glp_batch, void (*)(glp_batch *)> b(new glp_batch(), batch_destroy);
    b->ctx = c; b->ncols = ncols; b->lg = lg; b->rate_bits = rate_bits; b->cap_height = cap_height; b->K = K; b->hasher = hasher;
    b->salt = salt_seed ? SALT_SIZE : 0;
    b->ndigests = merkle_num_digests(N, cap_height);
    const size_t leaf_len = ncols + b->salt;
    GLP_TRY(c->alloc((void **)&b->coeffs, tot * n * 8));
    GLP_TRY(c->alloc((void **)&b->lde, (size_t)K * leaf_len * N * 8));
    GLP_TRY(c->alloc((void **)&b->digests, (size_t)K * b->ndigests * 32));
    {
        // The salt columns of proof k sit between its polynomial columns and those of proof k + 1.  One member: they follow its columns and
        // the LDE goes straight into place.  Several: one wide LDE into scratch, then one strided copy into place (K LDE calls of one
        // proof each underfill the device: profiles/r05_zero_knowledge.txt).
        Scratch sc(c);
        const bool strided = b->salt && K > 1;
        u64 *lde = b->lde;
        if (strided) GLP_TRY(sc.words(&lde, tot * N));
        // The column ranges the coefficients and the LDE are made in: every column at once, or the chunks of a host upload.  Chunking pays
        // when a chunk's copy is long against a few launches: below 64 MB the witness goes up in one piece.
        const size_t nchunks = !host_src || tot * n * 8 < ((size_t)64 << 20) ? 1 : std::min<size_t>(8, tot), per = (tot + nchunks - 1) / nchunks;
        std::vector<hipEvent_t> evs;
        int rc = GLP_OK;
        for (size_t c0 = 0; c0 < tot && rc == GLP_OK; c0 += per) {
            const u32 cn = (u32)std::min(per, tot - c0);
            const u64 *in = dev_in + c0 * n;
            u64 *co = b->coeffs + c0 * n;
            if (host_src) {
                hipEvent_t ev = nullptr;
                hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
                if (e == hipSuccess) evs.push_back(ev);
                if (e == hipSuccess) e = hipMemcpyAsync(const_cast<u64 *>(in), host_src + c0 * n, (size_t)cn * n * 8, hipMemcpyHostToDevice, c->copy_stream);
                if (e == hipSuccess) e = hipEventRecord(ev, c->copy_stream);
                if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev, 0);
                if (e != hipSuccess) { rc = set_error(GLP_ERR_HIP, "witness upload: %s", hipGetErrorString(e)); break; }
            }
            if (input_kind == BATCH_VALUES) {
                StageScope st(c, "intt", 16.0 * n * cn);
                rc = intt_values_to_coeffs(c, in, co, cn, lg);
            } else if (input_kind == BATCH_COEFFS_NATURAL) {
                StageScope st(c, "bitrev_coeffs", 16.0 * n * cn);
                rc = bitrev_copy(c, in, co, cn, lg);
            } else {
                StageScope st(c, "copy_coeffs", 16.0 * n * cn);
                const hipError_t e = hipMemcpyAsync(co, in, (size_t)cn * n * 8, hipMemcpyDeviceToDevice, c->stream);
                if (e != hipSuccess) rc = set_error(GLP_ERR_HIP, "coefficient copy: %s", hipGetErrorString(e));
            }
            if (rc == GLP_OK) {
                StageScope st(c, "lde", (8.0 * n + 8.0 * N) * cn);
                rc = lde_coeffs(c, co, lde + c0 * N, cn, lg, rate_bits, glf::GEN);
                if (rc == GLP_OK && strided) {
                    const hipError_t e = hipMemcpy2DAsync(b->lde, leaf_len * N * 8, lde, (size_t)ncols * N * 8, (size_t)ncols * N * 8, K,
                                                          hipMemcpyDeviceToDevice, c->stream);
                    if (e != hipSuccess) rc = set_error(GLP_ERR_HIP, "strided LDE copy: %s", hipGetErrorString(e));
                }
            }
        }
        if (host_src) {         // on every exit: the copy stream drained, its events gone
            (void)hipStreamSynchronize(c->copy_stream);
            for (hipEvent_t ev : evs) (void)hipEventDestroy(ev);
        }
        GLP_TRY(rc);
    }
    if (b->salt) GLP_TRY(merkle_fill_salts(c, b->lde, ncols, lg, rate_bits, salt_seed, salt_tag, K, leaf_len * N));
    GLP_TRY(merkle_from_lde(c, b->lde, (u32)leaf_len, lg, rate_bits, cap_height, b->digests, K, leaf_len * N, b->ndigests * 4, hasher));
    *out = b.release();
    return GLP_OK;
}

// the single-batch entry points that take host memory
static int batch_from_host(const char *fn, glp_ctx *c, const u64 *host, bool from_values, u32 ncols, u32 log_n, u32 rate_bits, u32 cap_height,
                           glp_batch **out, int hasher = GLP_HASH_POSEIDON, const u64 *salt_seed = nullptr, u32 salt_tag = 0) {
    GLP_REQUIRE(c && host && out, "null argument");
    *out = nullptr;
    GLP_TRY(batch_shape_check(nullptr, 1, ncols, log_n, rate_bits, cap_height, (u32)hasher));
    GLP_TRY(host_field_check(c, fn, from_values ? "values" : "coeffs", host, 0, ncols, (size_t)1 << log_n));
    GLP_TRY(bind(c));
    Scratch s(c);
    const size_t tot = (size_t)ncols << log_n;
    if (from_values) {       // not copied here: the upload is batch_build's own, pipelined with the transforms
        u64 *d;
        GLP_TRY(s.words(&d, tot));
        return batch_build(c, d, BATCH_VALUES, ncols, (int)log_n, (int)rate_bits, (int)cap_height, out, host, 1, hasher, salt_seed, salt_tag);
    }
    const u64 *d;
    GLP_TRY(s.input(host, 0, tot, &d));
    return batch_build(c, d, BATCH_COEFFS_NATURAL, ncols, (int)log_n, (int)rate_bits, (int)cap_height, out, nullptr, 1, hasher);
}

// glp_batch_many_from_*: K batches of one shape from [K][ncols][n], host or device memory
static int batch_many(const char *fn, glp_ctx *c, const u64 *in, int on_device, bool from_values, u32 K, u32 ncols, u32 log_n, u32 rate_bits, u32 cap_height,
                      u32 hasher, const u64 *seed, glp_batch **out) {
    GLP_REQUIRE(c && in && out, "null argument");
    *out = nullptr;
    GLP_REQUIRE(K >= 1 && K <= 4096, "num_proofs = %u outside 1..4096", K);
    GLP_TRY(batch_shape_check(nullptr, K, ncols, log_n, rate_bits, cap_height, hasher, BATCH_MAX_BYTES));
    if (!on_device) GLP_TRY(host_field_check(c, fn, from_values ? "values" : "coeffs", in, K, ncols, (size_t)1 << log_n));
    GLP_TRY(bind(c));
    u64 sd[4];
    if (seed) for (int i = 0; i < 4; i++) sd[i] = glf::canon(seed[i]);
    Scratch s(c);
    const u64 *d;
    GLP_TRY(s.input(in, on_device, ((size_t)K * ncols) << log_n, &d));
    return batch_build(c, d, from_values ? BATCH_VALUES : BATCH_COEFFS_NATURAL, ncols, (int)log_n, (int)rate_bits, (int)cap_height, out, nullptr, K,
                       (int)hasher, seed ? sd : nullptr, GLP_SALT_TAG_BATCH);
}

}  // namespace glp

// the single-batch accessors read one tree: a many-proofs batch is taken apart with glp_batch_member first
#define GLP_BATCH_SINGLE(B) \
    GLP_REQUIRE((B)->K == 1, "a many-proof batch (K = %u): take one member with glp_batch_member, or all caps with glp_batch_caps", (B)->K)

extern "C" {

int glp_batch_many_from_values(glp_ctx *c, const uint64_t *values, int values_on_device, uint32_t num_proofs, uint32_t ncols, uint32_t log_n,
                               uint32_t rate_bits, uint32_t cap_height, uint32_t hasher, const uint64_t *seed, glp_batch **out) {
    return batch_many("glp_batch_many_from_values", c, values, values_on_device, true, num_proofs, ncols, log_n, rate_bits, cap_height, hasher, seed, out);
}
int glp_batch_many_from_coeffs(glp_ctx *c, const uint64_t *coeffs, int coeffs_on_device, uint32_t num_proofs, uint32_t ncols, uint32_t log_n,
                               uint32_t rate_bits, uint32_t cap_height, uint32_t hasher, const uint64_t *seed, glp_batch **out) {
    return batch_many("glp_batch_many_from_coeffs", c, coeffs, coeffs_on_device, false, num_proofs, ncols, log_n, rate_bits, cap_height, hasher, seed, out);
}
uint32_t glp_batch_num_proofs(const glp_batch *b) { return b ? b->K : 0; }
int glp_batch_member(const glp_batch *b, uint32_t k, glp_batch **view_out) {
    GLP_REQUIRE(b && view_out, "null argument");
    *view_out = nullptr;
    GLP_REQUIRE(k < b->K, "glp_batch_member: k = %u, the batch has %u members", k, b->K);
    const size_t n = (size_t)1 << b->lg, N = n << b->rate_bits;
    glp_batch *v = new glp_batch(*b);
    v->K = 1; v->view = true;
    v->coeffs = b->coeffs + (size_t)k * b->ncols * n;
    v->lde = b->lde + (size_t)k * (b->ncols + b->salt) * N;
    v->digests = b->digests + (size_t)k * b->ndigests * 4;
    *view_out = v;
    return GLP_OK;
}
int glp_batch_caps(const glp_batch *b, uint64_t *caps_out) {
    GLP_REQUIRE(b && caps_out, "null argument");
    glp_ctx *c = b->ctx;
    GLP_TRY(bind(c));
    const size_t N = (size_t)1 << (b->lg + b->rate_bits), capb = (size_t)32 << b->cap_height;
    GLP_HIP(hipMemcpy2DAsync(caps_out, capb, b->digests + 4 * merkle_cap_offset(N, b->cap_height), b->ndigests * 32, capb, b->K,
                             hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

int glp_batch_from_values(glp_ctx *c, const uint64_t *values, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
                          uint32_t cap_height, glp_batch **out) {
    return batch_from_host("glp_batch_from_values", c, values, true, ncols, log_n, rate_bits, cap_height, out);
}
int glp_batch_from_coeffs(glp_ctx *c, const uint64_t *coeffs, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
                          uint32_t cap_height, glp_batch **out) {
    return batch_from_host("glp_batch_from_coeffs", c, coeffs, false, ncols, log_n, rate_bits, cap_height, out);
}
int glp_batch_from_values_h(glp_ctx *c, const uint64_t *values, uint32_t ncols, uint32_t log_n, uint32_t rate_bits, uint32_t cap_height,
                            uint32_t hasher, glp_batch **out) {
    return batch_from_host("glp_batch_from_values_h", c, values, true, ncols, log_n, rate_bits, cap_height, out, (int)hasher);
}
int glp_batch_from_coeffs_h(glp_ctx *c, const uint64_t *coeffs, uint32_t ncols, uint32_t log_n, uint32_t rate_bits, uint32_t cap_height,
                            uint32_t hasher, glp_batch **out) {
    return batch_from_host("glp_batch_from_coeffs_h", c, coeffs, false, ncols, log_n, rate_bits, cap_height, out, (int)hasher);
}
int glp_batch_from_values_salted(glp_ctx *c, const uint64_t *values, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
                                 uint32_t cap_height, uint32_t hasher, const uint64_t seed[4], glp_batch **out) {
    GLP_REQUIRE(c && values && seed && out, "null argument");
    GLP_TRY(bind(c));
    u64 s[4];
    for (int i = 0; i < 4; i++) s[i] = glf::canon(seed[i]);
    return batch_from_host("glp_batch_from_values_salted", c, values, true, ncols, log_n, rate_bits, cap_height, out, (int)hasher, s, GLP_SALT_TAG_BATCH);
}
int glp_batch_from_values_device(glp_ctx *c, const uint64_t *dev_values, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
                                 uint32_t cap_height, glp_batch **out) {
    GLP_REQUIRE(c && dev_values && out, "null argument");
    GLP_TRY(bind(c));
    return batch_build(c, dev_values, BATCH_VALUES, ncols, (int)log_n, (int)rate_bits, (int)cap_height, out);
}
int glp_batch_from_coeffs_device(glp_ctx *c, const uint64_t *dev_coeffs, uint32_t ncols, uint32_t log_n, uint32_t rate_bits,
                                 uint32_t cap_height, glp_batch **out) {
    GLP_REQUIRE(c && dev_coeffs && out, "null argument");
    GLP_TRY(bind(c));
    return batch_build(c, dev_coeffs, BATCH_COEFFS_NATURAL, ncols, (int)log_n, (int)rate_bits, (int)cap_height, out);
}

// ---- the caller's quotient at the commitment seam
int glp_batch_lde_values(const glp_batch *b, uint32_t col_begin, uint32_t num_cols, uint32_t sub_bits, uint64_t row_begin, uint64_t num_rows,
                         uint32_t layout, uint64_t *out, int out_on_device) {
    GLP_REQUIRE(b, "glp_batch_lde_values: b is null");
    GLP_REQUIRE(out, "glp_batch_lde_values: out is null");
    GLP_REQUIRE(num_cols > 0, "glp_batch_lde_values: num_cols is 0");
    GLP_REQUIRE(num_rows > 0, "glp_batch_lde_values: num_rows is 0");
    GLP_REQUIRE((u64)col_begin + num_cols <= b->ncols, "glp_batch_lde_values: col_begin + num_cols = %u + %u runs past ncols = %u (salts are not served)",
                col_begin, num_cols, b->ncols);
    GLP_REQUIRE(sub_bits <= (u32)b->rate_bits, "glp_batch_lde_values: sub_bits = %u is more than rate_bits = %d", sub_bits, b->rate_bits);
    const u64 M = (u64)1 << (b->lg + (int)sub_bits);
    GLP_REQUIRE(row_begin < M && num_rows <= M - row_begin, "glp_batch_lde_values: row_begin + num_rows = %llu + %llu runs past M = 2^(log_n + sub_bits) = %llu",
                (unsigned long long)row_begin, (unsigned long long)num_rows, (unsigned long long)M);
    GLP_REQUIRE(layout == GLP_LDE_ROW_MAJOR || layout == GLP_LDE_COL_MAJOR, "glp_batch_lde_values: layout = %u is not one of GLP_LDE_*", layout);
    glp_ctx *c = b->ctx;
    GLP_TRY(bind(c));
    const size_t N = (size_t)1 << (b->lg + b->rate_bits), words = (size_t)b->K * num_cols * num_rows;
    const u64 *src = b->lde + (size_t)col_begin * N;
    const bool row_major = layout == GLP_LDE_ROW_MAJOR;
    if (out_on_device)       // asynchronous on the ctx stream
        return lde_sub_coset_rows(c, src, (size_t)(b->ncols + b->salt) * N, b->K, num_cols, b->lg, b->rate_bits, (int)sub_bits, row_begin, num_rows,
                                  row_major, out);
    Scratch s(c);
    u64 *t;
    GLP_TRY(s.words(&t, words));
    GLP_TRY(lde_sub_coset_rows(c, src, (size_t)(b->ncols + b->salt) * N, b->K, num_cols, b->lg, b->rate_bits, (int)sub_bits, row_begin, num_rows,
                               row_major, t));
    GLP_HIP(hipMemcpyAsync(out, t, words * 8, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

int glp_batch_from_coset_values(glp_ctx *c, const uint64_t *values, int values_on_device, uint32_t num_proofs, uint32_t num_polys, uint32_t log_n,
                                uint32_t sub_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t hasher, const uint64_t *seed, glp_batch **out) {
    GLP_REQUIRE(c, "glp_batch_from_coset_values: ctx is null");
    GLP_REQUIRE(values, "glp_batch_from_coset_values: values is null");
    GLP_REQUIRE(out, "glp_batch_from_coset_values: out is null");
    *out = nullptr;
    GLP_REQUIRE(num_proofs >= 1 && num_proofs <= 4096, "num_proofs = %u outside 1..4096", num_proofs);
    GLP_REQUIRE(num_polys > 0, "num_polys must be positive");
    const size_t ncols = (size_t)num_polys << (sub_bits & 31);      // the mask keeps the shift defined until sub_bits is refused below
    GLP_TRY(batch_shape_check("glp_batch_from_coset_values", num_proofs, ncols, log_n, rate_bits, cap_height, hasher, BATCH_MAX_BYTES));
    GLP_REQUIRE(sub_bits <= rate_bits, "sub_bits = %u is more than rate_bits = %u", sub_bits, rate_bits);
    if (!values_on_device) GLP_TRY(host_field_check(c, "glp_batch_from_coset_values", "values", values, num_proofs, num_polys, (size_t)1 << (log_n + sub_bits)));
    GLP_TRY(bind(c));
    u64 sd[4];
    if (seed) for (int i = 0; i < 4; i++) sd[i] = glf::canon(seed[i]);
    const size_t channels = (size_t)num_proofs * num_polys, tot = (channels << sub_bits) << log_n;
    Scratch s(c);
    const u64 *planes;
    u64 *x;
    GLP_TRY(s.input(values, values_on_device, tot, &planes));
    GLP_TRY(s.words(&x, tot));
    if (sub_bits) {
        GLP_TRY(coset_values_to_planes(c, planes, x, channels, (int)log_n, (int)sub_bits));
        // the planes are in x; the coefficients go to a second block: the scratch's own copy of a host input, never the caller's device values
        u64 *y = values_on_device ? nullptr : const_cast<u64 *>(planes);
        if (!y) GLP_TRY(s.words(&y, tot));
        planes = x;
        x = y;
    }
    // planes -> x (per-plane inverse transform), combined in place: x holds the chunks' coefficients, bit-reversed
    GLP_TRY(coset_planes_to_chunk_coeffs(c, planes, x, x, (u32)channels, (int)log_n, (int)sub_bits, glf::GEN));
    return batch_build(c, x, BATCH_COEFFS_BITREV, (u32)ncols, (int)log_n, (int)rate_bits, (int)cap_height, out, nullptr, num_proofs, (int)hasher,
                       seed ? sd : nullptr, GLP_SALT_TAG_BATCH);
}

void glp_batch_free(glp_batch *b) { batch_destroy(b); }

int glp_batch_info(const glp_batch *b, uint32_t *ncols, uint32_t *log_n, uint32_t *rate_bits, uint32_t *cap_height) {
    GLP_REQUIRE(b, "null batch");
    if (ncols) *ncols = b->ncols;
    if (log_n) *log_n = (u32)b->lg;
    if (rate_bits) *rate_bits = (u32)b->rate_bits;
    if (cap_height) *cap_height = (u32)b->cap_height;
    return GLP_OK;
}

uint32_t glp_batch_leaf_len(const glp_batch *b) { return b ? b->ncols + b->salt : 0; }

int glp_batch_cap(const glp_batch *b, uint64_t *cap_out) {
    GLP_REQUIRE(b && cap_out, "null argument");
    GLP_BATCH_SINGLE(b);
    glp_ctx *c = b->ctx;
    GLP_TRY(bind(c));
    const size_t N = (size_t)1 << (b->lg + b->rate_bits);
    const size_t off = merkle_cap_offset(N, b->cap_height);
    GLP_HIP(hipMemcpyAsync(cap_out, b->digests + 4 * off, ((size_t)32) << b->cap_height, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

int glp_batch_coeffs(const glp_batch *b, uint32_t col_begin, uint32_t ncols, uint64_t *out) {
    GLP_REQUIRE(b && (out || !ncols), "null argument");
    GLP_BATCH_SINGLE(b);
    GLP_REQUIRE((u64)col_begin + ncols <= b->ncols, "column range out of bounds");
    if (!ncols) return GLP_OK;
    glp_ctx *c = b->ctx;
    GLP_TRY(bind(c));
    const size_t n = (size_t)1 << b->lg;
    Scratch s(c);
    u64 *t;
    GLP_TRY(s.words(&t, (size_t)ncols * n));
    GLP_TRY(bitrev_copy(c, b->coeffs + (size_t)col_begin * n, t, ncols, b->lg));
    GLP_HIP(hipMemcpyAsync(out, t, (size_t)ncols * n * 8, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

int glp_batch_leaf(const glp_batch *b, uint64_t leaf_index, uint64_t *out) {
    GLP_REQUIRE(b && out, "null argument");
    GLP_BATCH_SINGLE(b);
    const size_t N = (size_t)1 << (b->lg + b->rate_bits);
    GLP_REQUIRE(leaf_index < N, "leaf_index out of range");
    glp_ctx *c = b->ctx;
    GLP_TRY(bind(c));
    Scratch s(c);
    u64 *idx, *t;
    GLP_TRY(s.words(&idx, 1));
    const u32 leaf_len = b->ncols + b->salt;
    GLP_TRY(s.words(&t, leaf_len));
    GLP_HIP(hipMemcpyAsync(idx, &leaf_index, 8, hipMemcpyHostToDevice, c->stream));
    GLP_TRY(merkle_gather_lde_rows(c, b->lde, leaf_len, b->lg, b->rate_bits, idx, 1, t));
    GLP_HIP(hipMemcpyAsync(out, t, (size_t)leaf_len * 8, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

int glp_batch_merkle_proof(const glp_batch *b, uint64_t leaf_index, uint64_t *siblings_out) {
    GLP_REQUIRE(b, "null argument");
    GLP_BATCH_SINGLE(b);
    const size_t N = (size_t)1 << (b->lg + b->rate_bits);
    GLP_REQUIRE(leaf_index < N, "leaf_index out of range");
    const int depth = b->lg + b->rate_bits - b->cap_height;
    if (depth == 0) return GLP_OK;
    GLP_REQUIRE(siblings_out, "null argument");
    glp_ctx *c = b->ctx;
    GLP_TRY(bind(c));
    Scratch s(c);
    u64 *idx, *t;
    GLP_TRY(s.words(&idx, 1));
    GLP_TRY(s.words(&t, (size_t)depth * 4));
    GLP_HIP(hipMemcpyAsync(idx, &leaf_index, 8, hipMemcpyHostToDevice, c->stream));
    GLP_TRY(merkle_gather_paths(c, b->digests, N, b->cap_height, idx, 1, t));
    GLP_HIP(hipMemcpyAsync(siblings_out, t, (size_t)depth * 32, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

size_t glp_batch_num_digests(const glp_batch *b) { return b ? b->ndigests : 0; }

int glp_batch_digests(const glp_batch *b, uint64_t *out) {
    GLP_REQUIRE(b && out, "null argument");
    GLP_BATCH_SINGLE(b);
    glp_ctx *c = b->ctx;
    GLP_TRY(bind(c));
    GLP_HIP(hipMemcpyAsync(out, b->digests, b->ndigests * 32, hipMemcpyDeviceToHost, c->stream));
    GLP_HIP(hipStreamSynchronize(c->stream));
    return GLP_OK;
}

}  // extern "C"
