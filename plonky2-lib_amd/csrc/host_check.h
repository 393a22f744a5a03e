// host_check.h -- how host code refuses: set_error and the two macros that return through it, and the canonical-form scan of field
// arrays from outside.  No context and no HIP call, so the device-free headers (fri_shape.h, circuit_common.h, verify_host.h,
// proof_bytes.h) share it with the library; common.h adds the context, GLP_HIP and the thread's last message.  The library's
// set_error is api.hip's; a stand-alone host program supplies its own.
#pragma once
#include <stddef.h>
#include "../../include/glp.h"
#include "glf.h"

namespace glp {

int set_error(int code, const char *fmt, ...);

#define GLP_TRY(expr)              \
    do {                           \
        int _rc = (expr);          \
        if (_rc != GLP_OK) return _rc; \
    } while (0)
#define GLP_REQUIRE(cond, ...)                                  \
    do {                                                        \
        if (!(cond)) return glp::set_error(GLP_ERR_ARG, __VA_ARGS__); \
    } while (0)

// index of the first word >= p, or count if every word is a canonical field element (host; the inner loop vectorises).
// glf::add and glf::sub are right for canonical operands only, so no word >= p gets that far: every entry point that takes a field
// array from host memory rejects it by name with this scan (large arrays in pieces on the context's host threads: host_pool.h,
// host_field_check), and the kernels that read a caller's device words reduce them with canon() as they load them.
inline size_t first_noncanonical(const u64 *v, size_t count) {
    for (size_t i0 = 0; i0 < count; i0 += 4096) {
        const size_t i1 = i0 + 4096 < count ? i0 + 4096 : count;
        u64 bad = 0;
        for (size_t i = i0; i < i1; i++) bad |= (u64)(v[i] >= glf::P);
        if (bad) for (size_t i = i0; i < i1; i++) if (v[i] >= glf::P) return i;
    }
    return count;
}

}  // namespace glp
