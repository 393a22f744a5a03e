// gate_shapes.h -- what the HOST needs to know of each gate type, once: the list of types, the shape glp_circuit_create checks a
// description against, and the launch class and limb-column layout build_quotient_plan works from (circuit_create.inc).  No kernels
// and no HIP calls.  The constraints themselves are gate_terms (quotient_kernels.inc); DESIGN.md lists what a new gate type touches.
#pragma once
#include <stdint.h>
#include "../../include/glp.h"

typedef uint64_t u64;
typedef uint32_t u32;

// Every gate type that has constraints, in GLP_GATE_* order: stage_quotient_eval (prover_stages.inc) generates its one-launch-per-type
// switch from this list.  NoopGate has none, and 19 is unassigned.
#define GLP_CONSTRAINED_GATES(X)                                                                                              \
    X(GLP_GATE_CONSTANT) X(GLP_GATE_PUBLIC_INPUT) X(GLP_GATE_ARITHMETIC) X(GLP_GATE_POSEIDON) X(GLP_GATE_U32_INTERLEAVE)         \
    X(GLP_GATE_UNINTERLEAVE_U32) X(GLP_GATE_UNINTERLEAVE_B32) X(GLP_GATE_U32_ARITHMETIC) X(GLP_GATE_U32_ADD_MANY)                \
    X(GLP_GATE_U32_SUBTRACTION) X(GLP_GATE_U32_RANGE_CHECK) X(GLP_GATE_COMPARISON) X(GLP_GATE_BASE_SUM) X(GLP_GATE_RANDOM_ACCESS) \
    X(GLP_GATE_ARITHMETIC_EXTENSION) X(GLP_GATE_MUL_EXTENSION) X(GLP_GATE_REDUCING) X(GLP_GATE_REDUCING_EXTENSION)               \
    X(GLP_GATE_EXPONENTIATION) X(GLP_GATE_COSET_INTERPOLATION) X(GLP_GATE_POSEIDON_MDS)

// A type this build knows: NoopGate or one of the list.  A gate of any other type is GLP_ERR_UNSUPPORTED; a known type whose
// parameters gate_shape rejects is GLP_ERR_ARG.
inline bool gate_type_known(u32 type) {
    switch (type) {
    case GLP_GATE_NOOP:
#define GLP_GATE_CASE(T) case T:
    GLP_CONSTRAINED_GATES(GLP_GATE_CASE)
#undef GLP_GATE_CASE
        return true;
    default: return false;
    }
}

constexpr u32 COSET_MAX_BITS = 5;     // CosetInterpolationGate: largest subgroup_bits (sizes coset_table, prover_types.h)

// The base-4 limb columns of a limb gate (U32Arithmetic, U32AddMany, U32Subtraction, U32RangeCheck), as k_quotient_limbs' column
// program needs them.  Op i owns the columns first + limbs * i + j, j < limbs, and the constraints kstride * i + ..: limb j's
// range check is klimb + j (descending: klimb + limbs - 1 - j); limbs 0..15 sum (base 4) to wire ref_stride * i + ref0 in
// constraint ksum, limbs 16.. to the wire after it in constraint ksum + 1.
struct LimbBlock { u32 first, limbs, ops, kstride, klimb, ksum, ref_stride, ref0; bool descending; };
enum GateLaunch { GATE_LAUNCH_OWN = 0, GATE_LAUNCH_LIGHT, GATE_LAUNCH_LIMB };
struct GateShape {
    u32 wires = 0, consts = 0, constraints = 0;   // wire columns, gate constants and constraints the quotient kernels touch
    u32 routed = 0;                               // inputs that must lie in routed columns (0: nothing required)
    u32 degree = 0;                               // constraint degree, checked against quotient_degree_factor (0: not checked)
    GateLaunch launch = GATE_LAUNCH_OWN;          // LIGHT: HBM-bound, rides with k_quotient; LIMB: may share k_quotient_limbs
    LimbBlock limb = {};                          // GATE_LAUNCH_LIMB only
};
// false: the parameters are outside what the kernels take (the bounds also keep the counts below from wrapping)
inline bool gate_shape(const glp_gate &g, GateShape &s) {
    const u32 p0 = g.p0, p1 = g.p1;
    s = GateShape();
    switch (g.type) {
    case GLP_GATE_NOOP: return true;
    case GLP_GATE_CONSTANT: s.wires = p0; s.consts = p0; s.constraints = p0; s.launch = GATE_LAUNCH_LIGHT; return true;
    case GLP_GATE_PUBLIC_INPUT: s.wires = 4; s.constraints = 4; s.launch = GATE_LAUNCH_LIGHT; return true;
    case GLP_GATE_ARITHMETIC: s.wires = 4 * p0; s.consts = 2; s.constraints = p0; s.launch = GATE_LAUNCH_LIGHT; return true;
    case GLP_GATE_POSEIDON: s.wires = 135; s.constraints = 123; return true;
    case GLP_GATE_U32_INTERLEAVE: s.wires = 34 * p0; s.constraints = 34 * p0; return true;
    case GLP_GATE_UNINTERLEAVE_U32: case GLP_GATE_UNINTERLEAVE_B32: s.wires = 67 * p0; s.constraints = 67 * p0; return true;
    // the limb gates: head wires per op (6 / addends + 3 / 5 / 1), then the limb columns of all ops
    case GLP_GATE_U32_ARITHMETIC:
        s.wires = 38 * p0; s.constraints = 36 * p0; s.launch = GATE_LAUNCH_LIMB; s.limb = {6 * p0, 32, p0, 36, 2, 34, 6, 3, true};
        return true;
    case GLP_GATE_U32_ADD_MANY:
        s.wires = (p0 + 3 + 18) * p1; s.constraints = 21 * p1; s.launch = GATE_LAUNCH_LIMB; s.limb = {(p0 + 3) * p1, 18, p1, 21, 1, 19, p0 + 3, p0 + 1, true};
        return p0 >= 1 && p0 <= 16;
    case GLP_GATE_U32_SUBTRACTION:
        s.wires = 21 * p0; s.constraints = 19 * p0; s.launch = GATE_LAUNCH_LIMB; s.limb = {5 * p0, 16, p0, 19, 1, 17, 5, 3, true};
        return true;
    case GLP_GATE_U32_RANGE_CHECK:
        s.wires = 17 * p0; s.constraints = 17 * p0; s.launch = GATE_LAUNCH_LIMB; s.limb = {p0, 16, p0, 17, 1, 0, 1, 0, false};
        return true;
    case GLP_GATE_COMPARISON: {
        if (p1 == 0 || p0 == 0 || p0 > 64) return false;
        const u32 cb = (p0 + p1 - 1) / p1;
        if (cb > 4) return false;
        s.wires = 4 + 5 * p1 + cb + 1; s.constraints = 2 + 5 * p1 + 1 + (cb + 1) + 2; return true;
    }
    case GLP_GATE_BASE_SUM: s.wires = 1 + p0; s.constraints = 1 + p0; s.launch = GATE_LAUNCH_LIGHT; return p1 >= 2 && p1 <= 16;
    case GLP_GATE_RANDOM_ACCESS: {
        const u32 copies = p1 & 0xFFFF, nextra = p1 >> 16;
        if (p0 < 1 || p0 > 5) return false;
        s.wires = (2 + (1u << p0)) * copies + nextra + p0 * copies; s.consts = nextra; s.constraints = copies * (p0 + 2) + nextra;
        s.launch = GATE_LAUNCH_LIGHT;
        return true;
    }
    // the extension-field gates: p0 = num_ops / num_coeffs.  Reducing: output, alpha, old_acc and the coefficients are routed
    case GLP_GATE_ARITHMETIC_EXTENSION: s.wires = 8 * p0; s.consts = 2; s.constraints = 2 * p0; return p0 >= 1 && p0 <= 4096;
    case GLP_GATE_MUL_EXTENSION: s.wires = 6 * p0; s.consts = 1; s.constraints = 2 * p0; return p0 >= 1 && p0 <= 4096;
    case GLP_GATE_REDUCING: s.wires = 3 * p0 + 4; s.constraints = 2 * p0; s.routed = 6 + p0; return p0 >= 1 && p0 <= 4096;
    case GLP_GATE_REDUCING_EXTENSION: s.wires = 4 * p0 + 4; s.constraints = 2 * p0; s.routed = 6 + 2 * p0; return p0 >= 1 && p0 <= 4096;
    // the recursion gates.  Exponentiation: base, p0 bits, output (routed), p0 intermediates.  CosetInterpolation: shift, 2^p0 values,
    // point, value (routed), I evals, I prods, shifted point (pairs), I = (2^p0 - 2) div (p1 - 1); at most 2 (2 + 2 * 30) = 124
    // constraints.  PoseidonMds: every wire is routed.
    case GLP_GATE_EXPONENTIATION:
        s.wires = 2 * p0 + 2; s.constraints = p0 + 1; s.routed = p0 + 2; s.degree = 4;
        return p0 >= 1 && p0 <= 4096;
    case GLP_GATE_COSET_INTERPOLATION: {
        if (p0 < 1 || p0 > COSET_MAX_BITS || p1 < 2 || p1 > (1u << p0)) return false;
        const u32 ni = ((1u << p0) - 2) / (p1 - 1);
        s.wires = 7 + (2u << p0) + 4 * ni; s.constraints = 2 * (2 + 2 * ni); s.routed = 5 + (2u << p0); s.degree = p1;
        return true;
    }
    case GLP_GATE_POSEIDON_MDS: s.wires = 48; s.constraints = 24; s.routed = 48; s.degree = 1; return p0 == 0 && p1 == 0;
    default: return false;
    }
}
