// witness.hip -- witness generation on the GPU: the row-local half (glp_witness_fill) and, over the same
// per-unit body, the dataflow half (glp_witness_plan_*, glp_witness_generate: second part of this file; caller-defined generators as
// unit programs: witness_program.inc).
//
// plonky2's `generate_partial_witness` (iop/generator.rs) runs every gate's `SimpleGenerator`s as their
// dependencies become known.  Two kinds of work hide in it: the copy-constraint DATAFLOW between rows (irregular:
// planned once per circuit on the host, then walked wave by wave on the GPU) and the ROW-LOCAL generators that derive a row's
// remaining wires from that row's own inputs -- bit and limb decompositions, inverses, S-box traces.  The second
// kind is most of the witness by volume (56 of 136 columns of the secp256k1 trace are base-4 limbs) and is
// embarrassingly row-parallel: one thread per trace row here, written straight into the HBM witness that
// glp_prove_device consumes, so those columns never cross PCIe.
//
// Generators restated (one `case` each below; wire layouts = the gate definitions in quotient_kernels.inc `gate_terms`):
//   the reference's own     U32InterleaveGenerator      [REF src/u32/gates/interleave_u32.rs:289-318]
//                           UninterleaveToU32Generator  [REF src/u32/gates/uninterleave_to_u32.rs:332-369]
//                           UninterleaveToB32Generator  [REF src/u32/gates/uninterleave_to_b32.rs:335-372]
//   plonky2_u32 (crate absent, recalled)  U32ArithmeticGenerator, U32AddManyGenerator, U32SubtractionGenerator,
//                           U32RangeCheckGenerator, ComparisonGenerator
//   plonky2 (crate absent, recalled)      BaseSplitGenerator (gates/base_sum.rs), ArithmeticBaseGenerator,
//                           RandomAccessGenerator, PoseidonGenerator, ConstantGenerator (gates/constant.rs and the
//                           extra constants of RandomAccessGate), ArithmeticExtensionGenerator, MulExtensionGenerator,
//                           ReducingGenerator, ReducingExtensionGenerator (F_p^2 values on wire pairs),
//                           ExponentiationGenerator, InterpolationGenerator (CosetInterpolationGate), PoseidonMdsGenerator
// Every value written is a canonical field element; inputs are read as canonical u64 exactly as
// `to_canonical_u64()` hands them to the Rust generators.
#include <stdlib.h>
#include <new>
#include "common.h"
#include "poseidon.h"
#include "prover_types.h"
#include "biguint_dev.h"

namespace {

struct WArgs {
    u64 *wires;              // [num_wires][n]
    const u64 *consts;       // [num_constants][n] values on H (selectors first)
    const DevGate *gates;
    u32 lg, nsel, num_gates, only_advice, nr;
};

__device__ __forceinline__ u64 winv(u64 a) {          // a != 0
    u64 r = 1, b = a, e = P - 2;
    while (e) { if (e & 1) r = mul(r, b); b = sqr(b); e >>= 1; }
    return r;
}

// How many independent generators (units) a row of a gate has; the table of include/glp.h ("witness generation, the dataflow half").
GLF_HD u32 witness_gate_units(u32 type, u32 p0, u32 p1) {
    switch (type) {
    case GLP_GATE_ARITHMETIC: case GLP_GATE_U32_INTERLEAVE: case GLP_GATE_UNINTERLEAVE_U32: case GLP_GATE_UNINTERLEAVE_B32:
    case GLP_GATE_U32_ARITHMETIC: case GLP_GATE_U32_SUBTRACTION: case GLP_GATE_U32_RANGE_CHECK:
    case GLP_GATE_ARITHMETIC_EXTENSION: case GLP_GATE_MUL_EXTENSION: return p0;
    case GLP_GATE_U32_ADD_MANY: return p1;
    case GLP_GATE_RANDOM_ACCESS: return (p1 & 0xFFFF) + 1;
    case GLP_GATE_NOOP: case GLP_GATE_PUBLIC_INPUT: return 0;
    case GLP_GATE_CONSTANT: case GLP_GATE_POSEIDON: case GLP_GATE_COMPARISON: case GLP_GATE_BASE_SUM: case GLP_GATE_REDUCING:
    case GLP_GATE_REDUCING_EXTENSION: case GLP_GATE_EXPONENTIATION: case GLP_GATE_COSET_INTERPOLATION: case GLP_GATE_POSEIDON_MDS: return 1;
    default: return 0;
    }
}

// One unit of one row: generator `unit` (< witness_gate_units) of gate g on the row W points at (wire j -> W[j * n], gate constant
// i -> GC[i * n]).  k_witness_fill runs every unit of a row; the wave kernels below run the units a plan lists.  WHICH = 1 keeps only
// the gates with one unit per op, WHICH = 2 only those with one unit per row (k_witness_fill loops over the first kind alone, so that
// nothing of a PoseidonGate row is hoisted out of a loop it runs once); 0 keeps all.
template <int WHICH = 0>
__device__ __forceinline__ void witness_unit(const WArgs &a, const DevGate &g, u64 *W, const u64 *GC, size_t n, u32 unit) {
    const u32 nr = a.only_advice ? a.nr : 0xFFFFFFFFu;         // only_advice: columns < nr (routed) are never written
    constexpr bool ONE = WHICH != 1, PER_OP = WHICH != 2;      // which cases this instance keeps: gates of one unit per row, gates of one per op
    const u32 i = unit;                                        // the op of a gate with one generator per op
#define WR(col, val) do { const u32 _c = (col); if (!a.only_advice || _c >= nr) W[(size_t)_c * n] = (val); } while (0)
#define RD(col) W[(size_t)(col) * n]
    switch (g.type) {
    case GLP_GATE_CONSTANT: if (!ONE) break;
        for (u32 k = 0; k < g.p0; k++) WR(k, GC[(size_t)k * n]);
        break;
    case GLP_GATE_ARITHMETIC: if (!PER_OP) break; {
        const u64 c0 = GC[0], c1 = GC[n];
        WR(4 * i + 3, add(mul(mul(RD(4 * i), RD(4 * i + 1)), c0), mul(RD(4 * i + 2), c1)));
        break;
    }
    case GLP_GATE_POSEIDON: if (!ONE) break; {
        // gates/poseidon.rs PoseidonGenerator: swap -> delta, then the round-by-round trace; the wires hold the S-box INPUTS
        u64 st[12];
        const u64 swap = RD(24);
        for (u32 i = 0; i < 4; i++) {
            const u64 lhs = RD(i), rhs = RD(i + 4);
            const u64 dl = mul(swap, sub(rhs, lhs));
            WR(25 + i, dl);
            st[i] = add(lhs, dl); st[i + 4] = sub(rhs, dl);
        }
        for (u32 i = 8; i < 12; i++) st[i] = RD(i);
        u32 rc = 0;
        for (u32 r = 0; r < 4; r++) {
            for (u32 i = 0; i < 12; i++) st[i] = add(st[i], pos::RC[rc + i]);
            rc += 12;
            if (r != 0) for (u32 i = 0; i < 12; i++) WR(29 + 12 * (r - 1) + i, st[i]);
            for (u32 i = 0; i < 12; i++) st[i] = pos::sbox7(st[i]);
            pos::mds_layer(st);
        }
        for (u32 r = 0; r < 22; r++) {
            for (u32 i = 0; i < 12; i++) st[i] = add(st[i], pos::RC[rc + i]);
            rc += 12;
            WR(65 + r, st[0]);
            st[0] = pos::sbox7(st[0]);
            pos::mds_layer(st);
        }
        for (u32 r = 0; r < 4; r++) {
            for (u32 i = 0; i < 12; i++) st[i] = add(st[i], pos::RC[rc + i]);
            rc += 12;
            for (u32 i = 0; i < 12; i++) WR(87 + 12 * r + i, st[i]);
            for (u32 i = 0; i < 12; i++) st[i] = pos::sbox7(st[i]);
            pos::mds_layer(st);
        }
        for (u32 i = 0; i < 12; i++) WR(12 + i, st[i]);
        break;
    }
    case GLP_GATE_U32_INTERLEAVE: if (!PER_OP) break;
        // [REF src/u32/gates/interleave_u32.rs:289-318]: bit wire k = bit (31 - k) of x (big-endian), x_interleaved = sum bit 4^(31-k)
        {
            const u64 x = RD(2 * i);
            u64 xi = 0;
            for (u32 k = 0; k < 32; k++) {
                const u64 bit = (x >> (31 - k)) & 1;
                WR(2 * g.p0 + 32 * i + k, bit);
                xi += bit << (2 * (31 - k));
            }
            WR(2 * i + 1, canon(xi));
        }
        break;
    case GLP_GATE_UNINTERLEAVE_U32:
    case GLP_GATE_UNINTERLEAVE_B32: if (!PER_OP) break;
        // [REF src/u32/gates/uninterleave_to_u32.rs:332-369, uninterleave_to_b32.rs:335-372]: 64 big-endian bits of
        // x_interleaved; even-position bits (shift + 1) -> x_evens, odd -> x_odds, weights 2^(31-j) (U32) or 4^(31-j) (B32)
        {
            const u64 x = RD(3 * i);
            u64 ev = 0, od = 0;
            for (u32 j = 0; j < 32; j++) {
                const u32 shift = 2 * (31 - j);
                const u64 be = (x >> (shift + 1)) & 1, bo = (x >> shift) & 1;
                WR(3 * g.p0 + 64 * i + 2 * j, be);
                WR(3 * g.p0 + 64 * i + 2 * j + 1, bo);
                const u32 cs = g.type == GLP_GATE_UNINTERLEAVE_U32 ? (31 - j) : 2 * (31 - j);
                ev += be << cs; od += bo << cs;
            }
            WR(3 * i + 1, canon(ev));
            WR(3 * i + 2, canon(od));
        }
        break;
    case GLP_GATE_U32_ARITHMETIC: if (!PER_OP) break;
        // plonky2_u32 arithmetic_u32.rs U32ArithmeticGenerator: output = m0 m1 + addend in the field, as a canonical u64
        {
            const u64 out = add(mul(RD(6 * i), RD(6 * i + 1)), RD(6 * i + 2));
            const u64 lo = out & 0xFFFFFFFFull, hi = out >> 32;
            WR(6 * i + 3, lo);
            WR(6 * i + 4, hi);
            const u64 diff = 0xFFFFFFFFull - hi;
            WR(6 * i + 5, diff ? winv(diff) : 0);
            for (u32 j = 0; j < 32; j++) WR(6 * g.p0 + 32 * i + j, (out >> (2 * j)) & 3);
        }
        break;
    case GLP_GATE_U32_ADD_MANY: if (!PER_OP) break; {
        // plonky2_u32 add_many_u32.rs U32AddManyGenerator: sum of the addends and the carry, split at bit 32
        const u32 na = g.p0, nops = g.p1, wd = na + 3;
        {
            u64 sum = RD(wd * i + na);
            for (u32 j = 0; j < na; j++) sum = add(sum, RD(wd * i + j));
            const u64 res = sum & 0xFFFFFFFFull, car = sum >> 32;
            WR(wd * i + na + 1, res);
            WR(wd * i + na + 2, car);
            for (u32 j = 0; j < 16; j++) WR(wd * nops + 18 * i + j, (res >> (2 * j)) & 3);
            for (u32 j = 0; j < 2; j++) WR(wd * nops + 18 * i + 16 + j, (car >> (2 * j)) & 3);
        }
        break;
    }
    case GLP_GATE_U32_SUBTRACTION: if (!PER_OP) break;
        // plonky2_u32 subtraction_u32.rs U32SubtractionGenerator: x - y - borrow in the field; a wrapped result (> 2^32)
        // means a borrow, and 2^32 is added back
        {
            const u64 r0 = sub(sub(RD(5 * i), RD(5 * i + 1)), RD(5 * i + 2));
            const u64 bo = r0 > (1ull << 32) ? 1 : 0;
            const u64 res = add(r0, bo << 32);
            WR(5 * i + 3, res);
            WR(5 * i + 4, bo);
            for (u32 j = 0; j < 16; j++) WR(5 * g.p0 + 16 * i + j, (res >> (2 * j)) & 3);
        }
        break;
    case GLP_GATE_U32_RANGE_CHECK: if (!PER_OP) break;
        // plonky2_u32 range_check_u32.rs U32RangeCheckGenerator: 16 base-4 limbs per input, little-endian
        {
            const u64 v = RD(i);
            for (u32 j = 0; j < 16; j++) WR(g.p0 + 16 * i + j, (v >> (2 * j)) & 3);
        }
        break;
    case GLP_GATE_COMPARISON: if (!ONE) break; {
        // plonky2_u32 comparison.rs ComparisonGenerator (first <= second): chunks, equality dummies, chunk-equal flags,
        // intermediate values, most significant diff, its bits, result
        const u32 nb = g.p0, ncx = g.p1, cb = (nb + ncx - 1) / ncx;
        const u64 first = RD(0), second = RD(1);
        const u32 o_a = 4, o_b = o_a + ncx, o_ed = o_b + ncx, o_ce = o_ed + ncx, o_iv = o_ce + ncx, o_mb = o_iv + ncx;
        u64 msd = 0;
        for (u32 i = 0; i < ncx; i++) {
            const u64 ca = (first >> (cb * i)) & ((1ull << cb) - 1), cbv = (second >> (cb * i)) & ((1ull << cb) - 1);
            WR(o_a + i, ca);
            WR(o_b + i, cbv);
            const u64 diff = sub(cbv, ca);
            const u64 eq = diff == 0 ? 1 : 0;
            WR(o_ed + i, eq ? 1 : winv(diff));
            WR(o_ce + i, eq);
            const u64 inter = mul(eq, msd);
            WR(o_iv + i, inter);
            msd = add(inter, mul(sub(1, eq), diff));
        }
        WR(3, msd);
        const u64 top = add((u64)1 << cb, msd);
        for (u32 j = 0; j <= cb; j++) WR(o_mb + j, (top >> j) & 1);
        WR(2, (top >> cb) & 1);
        break;
    }
    case GLP_GATE_BASE_SUM: if (!ONE) break; {
        // gates/base_sum.rs BaseSplitGenerator: little-endian digits of the sum in base B
        u64 v = RD(0);
        for (u32 j = 0; j < g.p0; j++) { WR(1 + j, v % g.p1); v /= g.p1; }
        break;
    }
    case GLP_GATE_RANDOM_ACCESS: if (!PER_OP) break; {
        // gates/random_access.rs RandomAccessGenerator: index bits (little-endian) and the claimed element list[index];
        // the gate's extra constants are plain ConstantGenerators
        const u32 bits = g.p0, copies = g.p1 & 0xFFFF, nextra = g.p1 >> 16, vs = 1u << bits;
        const u32 routed = (2 + vs) * copies + nextra;
        if (unit < copies) {
            const u32 cpy = unit, o = (2 + vs) * cpy;
            const u64 idx = RD(o);
            if (idx < vs) {                       // the Rust generator indexes the list: an out-of-range index panics there
                WR(o + 1, RD(o + 2 + (u32)idx));
                for (u32 b = 0; b < bits; b++) WR(routed + bits * cpy + b, (idx >> b) & 1);
            }
        } else {                                  // the last unit: the extra constants
            for (u32 e = 0; e < nextra; e++) WR((2 + vs) * copies + e, GC[(size_t)e * n]);
        }
        break;
    }
    case GLP_GATE_ARITHMETIC_EXTENSION: if (!PER_OP) break; {
        // gates/arithmetic_extension.rs ArithmeticExtensionGenerator: output = c0 m0 m1 + c1 addend over F_p^2
        const u64 c0 = GC[0], c1 = GC[n];
        {
            const u32 o = 8 * i;
            const ext2 t = e_add(e_scale(e_mul(e_make(RD(o), RD(o + 1)), e_make(RD(o + 2), RD(o + 3))), c0), e_scale(e_make(RD(o + 4), RD(o + 5)), c1));
            WR(o + 6, t.a);
            WR(o + 7, t.b);
        }
        break;
    }
    case GLP_GATE_MUL_EXTENSION: if (!PER_OP) break; {
        // gates/multiplication_extension.rs MulExtensionGenerator: output = c0 m0 m1 over F_p^2
        const u64 c0 = GC[0];
        {
            const u32 o = 6 * i;
            const ext2 t = e_scale(e_mul(e_make(RD(o), RD(o + 1)), e_make(RD(o + 2), RD(o + 3))), c0);
            WR(o + 4, t.a);
            WR(o + 5, t.b);
        }
        break;
    }
    case GLP_GATE_REDUCING:
    case GLP_GATE_REDUCING_EXTENSION: if (!ONE) break; {
        // gates/reducing.rs ReducingGenerator, gates/reducing_extension.rs ReducingExtensionGenerator: acc_i = acc_{i-1} alpha +
        // coeff_i from acc_{-1} = old_acc; acc_0 .. acc_{N-2} from wire 6 + cw N (routed or advice), acc_{N-1} = output (wires 0, 1)
        const u32 nco = g.p0, cw = g.type == GLP_GATE_REDUCING ? 1u : 2u, accs = 6 + cw * nco;
        const ext2 alpha = e_make(RD(2), RD(3));
        ext2 acc = e_make(RD(4), RD(5));
        for (u32 i = 0; i < nco; i++) {
            const u32 co = 6 + cw * i;
            acc = e_add(e_mul(acc, alpha), e_make(RD(co), cw == 2 ? RD(co + 1) : 0));
            const u32 dst = i + 1 < nco ? accs + 2 * i : 0;
            WR(dst, acc.a);
            WR(dst + 1, acc.b);
        }
        break;
    }
    case GLP_GATE_EXPONENTIATION: if (!ONE) break; {
        // gates/exponentiation.rs ExponentiationGenerator: square-and-multiply from the most significant bit; intermediate_i
        // at wire n + 2 + i, output = the last intermediate
        const u32 nb = g.p0;
        const u64 base = RD(0);
        u64 cur = 1;
        for (u32 i = 0; i < nb; i++) {
            cur = mul(sqr(cur), add(mul(RD(nb - i), sub(base, 1)), 1));   // bit n-1-i sits at wire 1 + (n-1-i); bit base + 1 - bit
            WR(nb + 2 + i, cur);
        }
        WR(nb + 1, cur);
        break;
    }
    case GLP_GATE_COSET_INTERPOLATION: if (!ONE) break; {
        // gates/coset_interpolation.rs InterpolationGenerator: shifted point = evaluation point / shift, then the barycentric chain
        // of quotient_kernels.inc `gate_terms` with its checkpoints (the intermediates) and the evaluation value
        const u32 np = 1u << g.p0, d = g.p1, ni = (np - 2) / (d - 1);
        const u32 o_pt = 1 + 2 * np, o_ie = o_pt + 4, o_ip = o_ie + 2 * ni, o_sp = o_ip + 2 * ni;
        const u64 *tab = coset_table(a.gates, a.num_gates, g.p0);
        const u64 sh = RD(0);
        const u64 shi = sh ? winv(sh) : 0;                         // a zero shift has no coset: the Rust generator panics there
        const ext2 x = e_scale(e_make(RD(o_pt), RD(o_pt + 1)), shi);
        WR(o_sp, x.a);
        WR(o_sp + 1, x.b);
        ext2 ev = e_from(0), pr = e_from(1);
        u32 j = 0;
        for (u32 c = 0; c <= ni; c++) {
            const u32 end = min(np, d + c * (d - 1));
            for (; j < end; j++) {
                const ext2 dx = e_make(sub(x.a, tab[2 * j]), x.b);
                ev = e_add(e_mul(ev, dx), e_scale(e_mul(e_make(RD(1 + 2 * j), RD(2 + 2 * j)), pr), tab[2 * j + 1]));
                pr = e_mul(pr, dx);
            }
            if (c < ni) { WR(o_ie + 2 * c, ev.a); WR(o_ie + 2 * c + 1, ev.b); WR(o_ip + 2 * c, pr.a); WR(o_ip + 2 * c + 1, pr.b); }
        }
        WR(o_pt + 2, ev.a);
        WR(o_pt + 3, ev.b);
        break;
    }
    case GLP_GATE_POSEIDON_MDS: if (!ONE) break; {
        // gates/poseidon_mds.rs PoseidonMdsGenerator: the MDS layer on each F_p^2 component of the 12 inputs
        for (u32 cmp = 0; cmp < 2; cmp++) {
            u64 st[12];
            for (u32 i = 0; i < 12; i++) st[i] = RD(2 * i + cmp);
            pos::mds_layer(st);
            for (u32 i = 0; i < 12; i++) WR(24 + 2 * i + cmp, st[i]);
        }
        break;
    }
    default: break;     // NoopGate; PublicInputGate (its wires are set from the public-input hash through copy constraints)
    }
#undef WR
#undef RD
}

// the row's gate: the selector polynomial of its group holds the gate index, every other selector UNUSED
__device__ __forceinline__ u32 witness_row_gate(const u64 *consts, u32 nsel, size_t n, size_t row) {
    u32 gi = 0xFFFFFFFFu;
    for (u32 s = 0; s < nsel; s++) {
        const u64 v = consts[(size_t)s * n + row];
        if (nsel == 1 || v != 0xFFFFFFFFull) gi = (u32)v;
    }
    return gi;
}

// One thread = one trace row: every unit of the row.  Rows of one gate type are contiguous in every circuit the builder emits, so a
// wave rarely sees more than one `case`.
__global__ __launch_bounds__(256) void k_witness_fill(WArgs a) {
    const size_t n = (size_t)1 << a.lg;
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const u32 gi = witness_row_gate(a.consts, a.nsel, n, row);
    if (gi >= a.num_gates) return;
    const DevGate g = a.gates[gi];
    const u32 nu = witness_gate_units(g.type, g.p0, g.p1);
    u64 *W = a.wires + row;
    const u64 *GC = a.consts + (size_t)a.nsel * n + row;
    if (nu) witness_unit<2>(a, g, W, GC, n, 0);                          // a gate with one unit per row: nothing for the others
    for (u32 u = 0; u < nu; u++) witness_unit<1>(a, g, W, GC, n, u);    // a gate with one unit per op: nothing for the others
}

}  // namespace

extern "C" int glp_witness_fill(glp_ctx *c, const glp_circuit *cc, uint64_t *dev_wires, int only_advice) {
    GLP_REQUIRE(c && cc && dev_wires, "null argument");
    GLP_REQUIRE(cc->ctx == c, "circuit belongs to another context");
    GLP_TRY(bind(c));
    WArgs a;
    a.wires = dev_wires; a.consts = cc->dev_consts; a.gates = cc->dev_gates;
    a.lg = cc->d.degree_bits; a.nsel = cc->d.num_selectors; a.num_gates = cc->d.num_gates;
    a.only_advice = only_advice ? 1u : 0u; a.nr = cc->d.num_routed_wires;
    const size_t n = (size_t)1 << a.lg;
    StageScope st(c, "witness_fill", 8.0 * n * cc->d.num_wires);
    hipLaunchKernelGGL(k_witness_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}

namespace {
constexpr u32 ALL_UNITS = 0xFFFFFFFFu;
// Which wire columns unit `unit` of a row of gate g writes (1) and which it reads as inputs (2); 0 = untouched.  ALL_UNITS: the whole
// row, what glp_witness_fill does -- the union of the units, by construction.
void witness_unit_roles(const glp_gate &g, u32 nw, u32 unit, uint8_t *role_out) {
    memset(role_out, 0, nw);
    auto out = [&](u32 c0, u32 cnt) { for (u32 i = 0; i < cnt && c0 + i < nw; i++) role_out[c0 + i] = 1; };
    auto in = [&](u32 c0, u32 cnt) { for (u32 i = 0; i < cnt && c0 + i < nw; i++) role_out[c0 + i] = 2; };
    const u32 u0 = unit == ALL_UNITS ? 0 : unit, u1 = unit == ALL_UNITS ? witness_gate_units(g.type, g.p0, g.p1) : unit + 1;   // the ops of a per-op gate
    switch (g.type) {
    case GLP_GATE_CONSTANT: out(0, g.p0); break;
    case GLP_GATE_ARITHMETIC: for (u32 i = u0; i < u1; i++) { in(4 * i, 3); out(4 * i + 3, 1); } break;
    case GLP_GATE_POSEIDON: in(0, 12); out(12, 12); in(24, 1); out(25, 110); break;
    case GLP_GATE_U32_INTERLEAVE: for (u32 i = u0; i < u1; i++) { in(2 * i, 1); out(2 * i + 1, 1); out(2 * g.p0 + 32 * i, 32); } break;
    case GLP_GATE_UNINTERLEAVE_U32: case GLP_GATE_UNINTERLEAVE_B32:
        for (u32 i = u0; i < u1; i++) { in(3 * i, 1); out(3 * i + 1, 2); out(3 * g.p0 + 64 * i, 64); } break;
    case GLP_GATE_U32_ARITHMETIC: for (u32 i = u0; i < u1; i++) { in(6 * i, 3); out(6 * i + 3, 3); out(6 * g.p0 + 32 * i, 32); } break;
    case GLP_GATE_U32_ADD_MANY: {
        const u32 wd = g.p0 + 3;
        for (u32 i = u0; i < u1; i++) { in(wd * i, g.p0 + 1); out(wd * i + g.p0 + 1, 2); out(wd * g.p1 + 18 * i, 18); }
        break;
    }
    case GLP_GATE_U32_SUBTRACTION: for (u32 i = u0; i < u1; i++) { in(5 * i, 3); out(5 * i + 3, 2); out(5 * g.p0 + 16 * i, 16); } break;
    case GLP_GATE_U32_RANGE_CHECK: for (u32 i = u0; i < u1; i++) { in(i, 1); out(g.p0 + 16 * i, 16); } break;
    case GLP_GATE_COMPARISON: { const u32 cb = (g.p0 + g.p1 - 1) / g.p1; in(0, 2); out(2, 2 + 5 * g.p1 + cb + 1); break; }
    case GLP_GATE_BASE_SUM: in(0, 1); out(1, g.p0); break;
    case GLP_GATE_RANDOM_ACCESS: {
        const u32 bits = g.p0, copies = g.p1 & 0xFFFF, nextra = g.p1 >> 16, vs = 1u << bits;
        for (u32 cpy = u0; cpy < u1 && cpy < copies; cpy++) {
            const u32 o = (2 + vs) * cpy;
            in(o, 1); out(o + 1, 1); in(o + 2, vs);
            out((2 + vs) * copies + nextra + bits * cpy, bits);
        }
        if (u1 == copies + 1) out((2 + vs) * copies, nextra);       // the last unit: the extra constants
        break;
    }
    case GLP_GATE_ARITHMETIC_EXTENSION: for (u32 i = u0; i < u1; i++) { in(8 * i, 6); out(8 * i + 6, 2); } break;
    case GLP_GATE_MUL_EXTENSION: for (u32 i = u0; i < u1; i++) { in(6 * i, 4); out(6 * i + 4, 2); } break;
    case GLP_GATE_REDUCING: case GLP_GATE_REDUCING_EXTENSION: {
        const u32 cw = g.type == GLP_GATE_REDUCING ? 1u : 2u;
        out(0, 2); in(2, 4 + cw * g.p0); out(6 + cw * g.p0, 2 * (g.p0 - 1));
        break;
    }
    case GLP_GATE_EXPONENTIATION: in(0, 1 + g.p0); out(g.p0 + 1, 1 + g.p0); break;
    case GLP_GATE_COSET_INTERPOLATION: {
        const u32 np = 1u << g.p0, ni = (np - 2) / (g.p1 - 1);
        in(0, 3 + 2 * np); out(3 + 2 * np, 2 + 4 * ni + 2);      // shift, values, point | value, intermediates, shifted point
        break;
    }
    case GLP_GATE_POSEIDON_MDS: in(0, 24); out(24, 24); break;
    default: break;
    }
}
}  // namespace

// Which wire columns glp_witness_fill writes on rows of gate `gate_index` (1) and which it reads as inputs (2); 0 = untouched.
extern "C" int glp_witness_columns(const glp_circuit *cc, uint32_t gate_index, uint8_t *role_out /* [num_wires] */) {
    GLP_REQUIRE(cc && role_out, "null argument");
    GLP_REQUIRE(gate_index < cc->d.num_gates, "gate index out of range");
    witness_unit_roles(cc->gates[gate_index], cc->d.num_wires, ALL_UNITS, role_out);
    return GLP_OK;
}

extern "C" uint32_t glp_witness_num_units(const glp_circuit *cc, uint32_t gate_index) {
    if (!cc || gate_index >= cc->d.num_gates) return 0;
    const glp_gate &g = cc->gates[gate_index];
    return witness_gate_units(g.type, g.p0, g.p1);
}

extern "C" int glp_witness_unit_columns(const glp_circuit *cc, uint32_t gate_index, uint32_t unit, uint8_t *role_out /* [num_wires] */) {
    static const char *fn = "glp_witness_unit_columns";
    GLP_REQUIRE(cc, "%s: circuit is null", fn);
    GLP_REQUIRE(role_out, "%s: role_out is null", fn);
    GLP_REQUIRE(gate_index < cc->d.num_gates, "%s: gate_index = %u, the circuit has %u gates", fn, gate_index, cc->d.num_gates);
    const glp_gate &g = cc->gates[gate_index];
    const u32 nu = witness_gate_units(g.type, g.p0, g.p1);
    GLP_REQUIRE(unit < nu, "%s: unit = %u, a row of gate %u has %u units", fn, unit, gate_index, nu);
    witness_unit_roles(g, cc->d.num_wires, unit, role_out);
    return GLP_OK;
}

// ------------------------------------------------------------------------------------------ the dataflow half
// include/glp.h, "witness generation, the dataflow half": the host plans once per circuit and input set which unit runs in which wave
// and which cell is copied from which; the kernels below walk those lists.  Every index a kernel uses was built and range-checked by the
// planner: no value read from a witness is an address (RandomAccessGate's index keeps its idx < vs guard in witness_unit).
namespace {
struct WUnit { u32 row, gu; };          // gu = gate << 16 | unit
struct WCopy { u32 src, dst; };         // flat positions col * n + row
typedef glp_witness_free_unit WFree;    // a free unit as the caller gave it; cell_begin points into the plan's 32-bit copy of cells[]
static_assert(sizeof(WFree) == 24, "glp_witness_free_unit: three u32 and six u16");
struct WGen {
    WArgs a;                            // a.wires: proof 0
    const WUnit *units;                 // wave w: units[unit_off[w] .. unit_off[w + 1]), sorted by row; wave 0 holds none
    const WCopy *copies;                // wave w: copies[copy_off[w] .. copy_off[w + 1])
    const u32 *unit_off, *copy_off, *inputs;
    const u64 *vals;                    // [K][num_inputs]
    u32 num_inputs, nw;
    const WFree *free_units;            // wave w: free_units[free_off[w] .. free_off[w + 1]), in the caller's order; null without free units
    const u32 *free_off, *free_cells;   // a unit's run: its input cells, then its output cells (NONE: not written)
    const u32 *moduli;                  // [num_moduli][8]
};
constexpr u32 NONE = 0xFFFFFFFFu;
constexpr u32 WGEN_MAX_PROOFS = 4096;   // as glp_witness_check
constexpr u32 WITNESS_NARROW_MAX_DEFAULT = 256;

// the units of wave w (wave 0: the scatter of the inputs) of one proof, lane `first` of `stride`
__device__ __forceinline__ void wg_units(const WGen &g, u64 *W, const u64 *vals, size_t n, u32 w, size_t first, size_t stride) {
    if (w == 0) {
        for (size_t i = first; i < g.num_inputs; i += stride) W[g.inputs[i]] = vals[i];
        return;
    }
    const size_t end = g.unit_off[w + 1];
    for (size_t i = g.unit_off[w] + first; i < end; i += stride) {
        const WUnit u = g.units[i];
        const DevGate gate = g.a.gates[u.gu >> 16];
        witness_unit(g.a, gate, W + u.row, g.a.consts + (size_t)g.a.nsel * n + u.row, n, u.gu & 0xFFFFu);
    }
}
// One free unit (include/glp.h, FREE UNITS) on one lane: operand limbs are the low 32 bits of the cells of its run.  The cells were
// range-checked by the planner; a value read from the witness is a limb, never a cell.  The two instances of the limb arithmetic are
// functions of their own, not inlined into the kernels: the register budget of the 8-limb one (every count a compile-time 8, its limbs
// in VGPRs) is then its own, whatever the gate units and the general-length instance beside it need, and the compiler's resource report
// names it (profiles/kernel_resources.sh witness.hip).
struct WFreeIo {                          // a unit's cells: rd(i) = limb i of its inputs, wr(i, v) = output cell i
    u64 *W; const u32 *in, *out;
    __device__ __forceinline__ u32 operator()(int i) const { return (u32)W[in[i]]; }
    __device__ __forceinline__ void operator()(int i, u32 v) const { const u32 c = out[i]; if (c != NONE) W[c] = v; }
};
__device__ __noinline__ void witness_free_unit8(u64 *W, const u32 *run, const u32 *mod, u32 kind) {
    const uint16_t len[6] = {8, 8, 8, (uint16_t)(kind == GLP_WGEN_NONNATIVE_MUL ? 8 : 1), 0, 0};
    u32 m[big::MAX_MOD];
    for (int i = 0; i < big::MAX_MOD; i++) m[i] = mod[i];
    const WFreeIo io = {W, run, run + (kind == GLP_WGEN_NONNATIVE_INV ? 8 : 16)};
    big::run_unit<true>(kind, len, m, 8, io, io, nullptr);
}
__device__ __noinline__ void witness_free_unit_any(u64 *W, const u32 *run, const u32 *mod, const WFree *u) {
    const WFree unit = *u;
    u32 m[big::MAX_MOD];
    for (int i = 0; i < big::MAX_MOD; i++) m[i] = mod ? mod[i] : 0;
    const WFreeIo io = {W, run, run + big::num_in(unit.kind, unit.len)};
    big::run_unit<false>(unit.kind, unit.len, m, big::used_limbs(m, big::MAX_MOD), io, io, nullptr);
}
__device__ __forceinline__ void witness_free_unit(const WGen &g, u64 *W, const WFree *u) {
    const u32 kind = u->kind;
    const u32 *run = g.free_cells + u->cell_begin;
    if (kind == GLP_WGEN_EQUALITY) {
        const u64 d = sub(W[run[0]], W[run[1]]);
        if (run[2] != NONE) W[run[2]] = d == 0 ? 1 : 0;
        if (run[3] != NONE) W[run[3]] = d ? winv(d) : 0;
        return;
    }
    const bool has_modulus = kind >= GLP_WGEN_NONNATIVE_ADD && kind <= GLP_WGEN_NONNATIVE_INV;
    const u32 *mod = has_modulus ? g.moduli + (size_t)u->modulus * big::MAX_MOD : nullptr;
    if (has_modulus && big::all8(kind, u->len, mod[big::MAX_MOD - 1] ? 8 : 0)) witness_free_unit8(W, run, mod, kind);
    else witness_free_unit_any(W, run, mod, u);
}
// the free units of wave w of one proof, lane `first` of `stride`; they read what earlier waves left and write cells nothing else
// of the wave touches, so they share the units step with wg_units
__device__ __forceinline__ void wg_free(const WGen &g, u64 *W, u32 w, size_t first, size_t stride) {
    if (!g.free_units || w == 0) return;
    const size_t end = g.free_off[w + 1];
    for (size_t i = g.free_off[w] + first; i < end; i += stride) witness_free_unit(g, W, g.free_units + i);
}
__device__ __forceinline__ void wg_copies(const WGen &g, u64 *W, u32 w, size_t first, size_t stride) {
    const size_t end = g.copy_off[w + 1];
    for (size_t i = g.copy_off[w] + first; i < end; i += stride) {
        const WCopy c = g.copies[i];
        W[c.dst] = W[c.src];
    }
}
// Walked waves: one workgroup per proof walks waves w0 .. w1.  All traffic of a proof stays in its workgroup, so plain global stores,
// drained, followed by the block barrier hand a wave's values to the next.
// FREE = false is the kernel of a plan without free units: nothing of the limb arithmetic is in it.
template <bool FREE>
__global__ __launch_bounds__(256) void k_witness_waves(WGen g, u32 w0, u32 w1) {
    const size_t n = (size_t)1 << g.a.lg;
    u64 *W = g.a.wires + (size_t)blockIdx.x * g.nw * n;
    const u64 *vals = g.vals + (size_t)blockIdx.x * g.num_inputs;
    for (u32 w = w0; w <= w1; w++) {
        wg_units(g, W, vals, n, w, threadIdx.x, 256);
        if (FREE) wg_free(g, W, w, threadIdx.x, 256);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        wg_copies(g, W, w, threadIdx.x, 256);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}
// Wide waves: one lane per unit (per copy), blockIdx.y = proof; the stream orders the two launches.
__global__ __launch_bounds__(256) void k_witness_units(WGen g, u32 w) {
    const size_t n = (size_t)1 << g.a.lg;
    wg_units(g, g.a.wires + (size_t)blockIdx.y * g.nw * n, g.vals + (size_t)blockIdx.y * g.num_inputs, n, w, (size_t)blockIdx.x * 256 + threadIdx.x,
             (size_t)gridDim.x * 256);
}
// the free units of a wide wave: one lane per unit, 64-lane workgroups so that the few long lanes of a wave spread over the chip
__global__ __launch_bounds__(64) void k_witness_free(WGen g, u32 w) {
    const size_t n = (size_t)1 << g.a.lg;
    wg_free(g, g.a.wires + (size_t)blockIdx.y * g.nw * n, w, (size_t)blockIdx.x * 64 + threadIdx.x, (size_t)gridDim.x * 64);
}
__global__ __launch_bounds__(256) void k_witness_copies(WGen g, u32 w) {
    const size_t n = (size_t)1 << g.a.lg;
    wg_copies(g, g.a.wires + (size_t)blockIdx.y * g.nw * n, w, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}
__global__ __launch_bounds__(256) void k_witness_read_cells(const u64 *wires, const u32 *cells, u64 *out, u32 num_cells, size_t per_proof) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < num_cells) out[(size_t)blockIdx.y * num_cells + i] = wires[(size_t)blockIdx.y * per_proof + cells[i]];
}
}  // namespace

#include "witness_program.inc"

struct glp_witness_plan {
    glp_ctx *ctx = nullptr;
    const glp_circuit *cc = nullptr;
    u32 num_inputs = 0, narrow_max = WITNESS_NARROW_MAX_DEFAULT;
    struct glp_witness_plan_info info;
    std::vector<u32> unit_off, copy_off;           // [num_waves + 2]
    std::vector<int32_t> cell_waves;               // [num_wires][n]
    WUnit *dev_units = nullptr;
    WCopy *dev_copies = nullptr;
    u32 *dev_unit_off = nullptr, *dev_copy_off = nullptr, *dev_inputs = nullptr;
    struct glp_witness_plan_free_info free_info;
    std::vector<u32> free_off;                     // [num_waves + 2]; empty without free units
    WFree *dev_free_units = nullptr;
    u32 *dev_free_off = nullptr, *dev_free_cells = nullptr, *dev_moduli = nullptr;
    std::vector<u32> prog_chunk_off;               // [num_waves + 2] into dev_prog_chunks; empty without program units
    u32 prog_lds = 0;                              // bytes of LDS a chunk's workgroup asks for: the widest register file of the programs
    WProgChunk *dev_prog_chunks = nullptr;
    WFree *dev_prog_units = nullptr;               // by wave, sorted by program
    WProgEntry *dev_prog_tab = nullptr;
    u64 *dev_prog_image = nullptr;
    mutable u64 *dev_vals = nullptr;               // [vals_cap] the input values of the generation in flight: a plan serves one at a time
    mutable size_t vals_cap = 0;
};

extern "C" void glp_witness_plan_free(glp_witness_plan *p) {
    if (!p) return;
    glp_ctx *c = p->ctx;
    if (bind(c) == GLP_OK) (void)hipStreamSynchronize(c->stream);
    c->release(p->dev_units); c->release(p->dev_copies); c->release(p->dev_unit_off); c->release(p->dev_copy_off);
    c->release(p->dev_inputs); c->release(p->dev_vals);
    c->release(p->dev_free_units); c->release(p->dev_free_off); c->release(p->dev_free_cells); c->release(p->dev_moduli);
    c->release(p->dev_prog_chunks); c->release(p->dev_prog_units); c->release(p->dev_prog_tab); c->release(p->dev_prog_image);
    delete p;
}

// The shape of a free unit's kind: which of len[0..5] are operands, which of them are single cells, which is a divisor.  0 = unknown kind.
struct WFreeShape { u32 operands; u32 single; int divisor; };     // bit i of single: len[i] must be 1
static WFreeShape witness_free_shape(u32 kind) {
    switch (kind) {
    case GLP_WGEN_EQUALITY: return {4, 0xF, -1};
    case GLP_WGEN_NONNATIVE_ADD: case GLP_WGEN_NONNATIVE_SUB: return {4, 0x8, -1};
    case GLP_WGEN_NONNATIVE_MULTI_ADD: return {4, 0x8, -1};
    case GLP_WGEN_NONNATIVE_MUL: return {4, 0, -1};
    case GLP_WGEN_NONNATIVE_INV: return {3, 0, -1};
    case GLP_WGEN_BIGUINT_DIV_REM: return {4, 0, 1};
    case GLP_WGEN_GLV_SECP256K1: return {5, 0x18, -1};
    default: return {0, 0, -1};
    }
}

// glp_witness_plan_create_prog without its allocation guard; glp_witness_plan_create_ex is its num_programs = 0 case (with_programs
// false: kind GLP_WGEN_PROGRAM stays an unknown kind there), glp_witness_plan_create its num_units = 0 case
static int witness_plan_build(const char *fn, glp_ctx *c, const glp_circuit *cc, const uint64_t *input_cells, uint32_t num_inputs,
                              const glp_witness_free_unit *funits, uint32_t nf, const uint64_t *fcells, size_t num_fcells, const uint32_t *moduli,
                              uint32_t num_moduli, const glp_witness_program_desc *programs, uint32_t num_programs, bool with_programs,
                              glp_witness_plan **out) {
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    GLP_REQUIRE(cc, "%s: circuit is null", fn);
    GLP_REQUIRE(out, "%s: out is null", fn);
    GLP_REQUIRE(input_cells || num_inputs == 0, "%s: input_cells is null, num_inputs = %u", fn, num_inputs);
    GLP_REQUIRE(funits || nf == 0, "%s: units is null, num_units = %u", fn, nf);
    GLP_REQUIRE(fcells || num_fcells == 0, "%s: cells is null, num_cells = %zu", fn, num_fcells);
    GLP_REQUIRE(moduli || num_moduli == 0, "%s: moduli is null, num_moduli = %u", fn, num_moduli);
    GLP_REQUIRE(programs || num_programs == 0, "%s: programs is null, num_programs = %u", fn, num_programs);
    GLP_REQUIRE(cc->ctx == c, "%s: circuit belongs to another ctx", fn);
    for (u32 i = 0; i < num_programs; i++) {
        char where[96];
        snprintf(where, sizeof(where), "%s: programs[%u]", fn, i);
        GLP_TRY(witness_program_check(where, programs + i));
    }
    const glp_circuit_desc &d = cc->d;
    const u32 lg = d.degree_bits, nw = d.num_wires, nr = d.num_routed_wires, ng = d.num_gates, nsel = d.num_selectors;
    const size_t n = (size_t)1 << lg, cells = (size_t)nw * n;
    // one short of the decoded sigma's 2^32: position 2^32 - 1 is the planner's "none"
    GLP_REQUIRE(cells < ((size_t)1 << 32), "%s: num_wires * 2^degree_bits = %zu positions, a plan addresses fewer than 2^32 (the bound of the decoded sigma)", fn, cells);
    GLP_REQUIRE(ng <= 0xFFFF, "%s: num_gates = %u, a plan names at most 65535 gates", fn, ng);
    for (u32 i = 0; i < num_inputs; i++)
        GLP_REQUIRE(input_cells[i] < cells, "%s: input_cells[%u] = %llu is out of range (num_wires * 2^degree_bits = %zu cells)", fn, i,
                    (unsigned long long)input_cells[i], cells);
    // which input names a cell (NONE: none); a cell listed twice is refused
    std::vector<u32> input_at(cells, NONE);
    for (u32 i = 0; i < num_inputs; i++) {
        u32 &at = input_at[(size_t)input_cells[i]];
        GLP_REQUIRE(at == NONE, "%s: input_cells[%u] = %llu is listed twice (also input_cells[%u])", fn, i, (unsigned long long)input_cells[i], at);
        at = i;
    }
    // the moduli and the free units: shapes, runs and cells
    GLP_REQUIRE(num_fcells < NONE, "%s: num_cells = %zu, a plan addresses fewer than 2^32 - 1", fn, num_fcells);
    for (u32 i = 0; i < num_moduli; i++) {
        const uint32_t *m = moduli + (size_t)i * 8;
        GLP_REQUIRE(m[0] & 1, "%s: moduli[%u] is even", fn, i);
        GLP_REQUIRE(big::used_limbs(m, 8) > 1 || m[0] >= 3, "%s: moduli[%u] = %u is below 3", fn, i, m[0]);
    }
    std::vector<u32> fcells32(num_fcells), f_ni(nf), f_no(nf);
    for (size_t i = 0; i < num_fcells; i++) fcells32[i] = fcells[i] < cells ? (u32)fcells[i] : NONE;      // outputs may be GLP_WGEN_NO_CELL; checked per run below
    for (u32 f = 0; f < nf; f++) {
        const glp_witness_free_unit &u = funits[f];
        if (with_programs && u.kind == GLP_WGEN_PROGRAM) {
            GLP_REQUIRE(u.modulus < num_programs, "%s: units[%u].modulus = %u, a program unit names its program there and num_programs = %u", fn, f, u.modulus, num_programs);
            const glp_witness_program_desc &pd = programs[u.modulus];
            GLP_REQUIRE(u.len[0] == pd.num_inputs, "%s: units[%u].len[0] = %u, programs[%u] has num_inputs = %u", fn, f, u.len[0], u.modulus, pd.num_inputs);
            GLP_REQUIRE(u.len[1] == pd.num_outputs, "%s: units[%u].len[1] = %u, programs[%u] has num_outputs = %u", fn, f, u.len[1], u.modulus, pd.num_outputs);
            for (u32 i = 2; i < 6; i++) GLP_REQUIRE(u.len[i] == 0, "%s: units[%u].len[%u] = %u, a program unit has two operands: unused entries are 0", fn, f, i, u.len[i]);
            f_ni[f] = u.len[0]; f_no[f] = u.len[1];
        } else {
            const WFreeShape sh = witness_free_shape(u.kind);
            GLP_REQUIRE(sh.operands, "%s: units[%u].kind = %u is not a GLP_WGEN_* kind", fn, f, u.kind);
            const bool has_modulus = u.kind >= GLP_WGEN_NONNATIVE_ADD && u.kind <= GLP_WGEN_NONNATIVE_INV;
            if (has_modulus) GLP_REQUIRE(u.modulus < num_moduli, "%s: units[%u].modulus = %u, num_moduli = %u", fn, f, u.modulus, num_moduli);
            else GLP_REQUIRE(u.modulus == 0, "%s: units[%u].modulus = %u, kind %u has no modulus: 0", fn, f, u.modulus, u.kind);
            for (u32 i = 0; i < 6; i++) {
                const u32 l = u.len[i];
                if (i >= sh.operands) { GLP_REQUIRE(l == 0, "%s: units[%u].len[%u] = %u, kind %u has %u operands: unused entries are 0", fn, f, i, l, u.kind, sh.operands); continue; }
                if (sh.single >> i & 1) { GLP_REQUIRE(l == 1, "%s: units[%u].len[%u] = %u, that operand of kind %u is 1 cell", fn, f, i, l, u.kind); continue; }
                if (u.kind == GLP_WGEN_NONNATIVE_MULTI_ADD && i == 0) continue;                                   // the number of summands
                if ((int)i == sh.divisor) GLP_REQUIRE(l <= 8, "%s: units[%u].len[%u] = %u, a divisor has at most 8 limbs", fn, f, i, l);
                GLP_REQUIRE(l <= GLP_WGEN_MAX_LIMBS, "%s: units[%u].len[%u] = %u, an operand has at most GLP_WGEN_MAX_LIMBS = %u limbs", fn, f, i, l, GLP_WGEN_MAX_LIMBS);
                if (u.kind == GLP_WGEN_GLV_SECP256K1) GLP_REQUIRE(l == (i ? 4u : 8u), "%s: units[%u].len[%u] = %u, GLV_SECP256K1 has k of 8 and k1, k2 of 4 limbs", fn, f, i, l);
            }
            f_ni[f] = big::num_in(u.kind, u.len); f_no[f] = big::num_out(u.kind, u.len);
        }
        GLP_REQUIRE((size_t)u.cell_begin + f_ni[f] + f_no[f] <= num_fcells, "%s: units[%u].cell_begin = %u: its run of %u cells leaves cells[] (num_cells = %zu)", fn, f,
                    u.cell_begin, f_ni[f] + f_no[f], num_fcells);
        for (u32 i = 0; i < f_ni[f] + f_no[f]; i++) {
            const uint64_t cell = fcells[(size_t)u.cell_begin + i];
            GLP_REQUIRE(cell < cells || (i >= f_ni[f] && cell == GLP_WGEN_NO_CELL), "%s: units[%u]: cells[%zu] = %llu is out of range (num_wires * 2^degree_bits = %zu cells)", fn, f,
                        (size_t)u.cell_begin + i, (unsigned long long)cell, cells);
        }
    }
    GLP_TRY(bind(c));
    // the gate of every row, as k_witness_fill reads it
    std::vector<u32> row_gate(n, NONE);
    {
        std::vector<u64> sel((size_t)nsel * n);
        GLP_TRY(d2h(c, sel.data(), cc->dev_consts, sel.size() * 8));
        for (size_t r = 0; r < n; r++) {
            u32 gi = NONE;
            for (u32 s = 0; s < nsel; s++) { const u64 v = sel[(size_t)s * n + r]; if (nsel == 1 || v != 0xFFFFFFFFull) gi = (u32)v; }
            row_gate[r] = gi < ng ? gi : NONE;
        }
    }
    // per gate and unit: the columns read and written
    std::vector<std::vector<std::vector<u32>>> g_in(ng), g_out(ng);
    {
        std::vector<uint8_t> role(nw);
        for (u32 gi = 0; gi < ng; gi++) {
            const glp_gate &g = cc->gates[gi];
            const u32 nu = witness_gate_units(g.type, g.p0, g.p1);
            GLP_REQUIRE(nu <= 0xFFFF, "%s: gate %u has %u units per row, a plan names at most 65535", fn, gi, nu);
            g_in[gi].resize(nu); g_out[gi].resize(nu);
            for (u32 u = 0; u < nu; u++) {
                witness_unit_roles(g, nw, u, role.data());
                for (u32 col = 0; col < nw; col++) { if (role[col] == 2) g_in[gi][u].push_back(col); if (role[col] == 1) g_out[gi][u].push_back(col); }
            }
        }
    }
    // the units in (row, unit) order; unit k of the plan = unit k - row_first[row] of its row; the free units follow: unit nu_total + f
    std::vector<size_t> row_first(n + 1, 0);
    for (size_t r = 0; r < n; r++) row_first[r + 1] = row_first[r] + (row_gate[r] == NONE ? 0 : g_in[row_gate[r]].size());
    const size_t nu_total = row_first[n], nk = nu_total + nf;
    GLP_REQUIRE(nk < NONE, "%s: %zu units exceed the 2^32 - 1 a plan addresses", fn, nk);
    std::vector<u32> unit_row(nu_total);
    for (size_t r = 0; r < n; r++) for (size_t k = row_first[r]; k < row_first[r + 1]; k++) unit_row[k] = (u32)r;
    auto for_in = [&](size_t k, auto &&visit) {            // the cells unit k reads / writes
        if (k < nu_total) { const size_t r = unit_row[k]; for (u32 col : g_in[row_gate[r]][k - row_first[r]]) visit((size_t)col * n + r); return; }
        const u32 f = (u32)(k - nu_total);
        for (u32 i = 0; i < f_ni[f]; i++) visit((size_t)fcells32[(size_t)funits[f].cell_begin + i]);
    };
    auto for_out = [&](size_t k, auto &&visit) {
        if (k < nu_total) { const size_t r = unit_row[k]; for (u32 col : g_out[row_gate[r]][k - row_first[r]]) visit((size_t)col * n + r); return; }
        const u32 f = (u32)(k - nu_total);
        for (u32 i = 0; i < f_no[f]; i++) { const u32 cell = fcells32[(size_t)funits[f].cell_begin + f_ni[f] + i]; if (cell != NONE) visit((size_t)cell); }
    };
    // the writer of every cell; a free unit may not write what another unit writes
    std::vector<u32> writer(cells, NONE);
    for (size_t k = 0; k < nu_total; k++) for_out(k, [&](size_t q) { writer[q] = (u32)k; });
    for (u32 f = 0; f < nf; f++) {
        int rc = GLP_OK;
        for_out(nu_total + f, [&](size_t q) {
            if (rc != GLP_OK) return;
            const u32 wk = writer[q];
            if (wk == NONE) { writer[q] = (u32)(nu_total + f); return; }
            if (wk >= nu_total) rc = set_error(GLP_ERR_ARG, "%s: units[%u]: output cell %zu is also written by units[%u]", fn, f, q, (u32)(wk - nu_total));
            else rc = set_error(GLP_ERR_ARG, "%s: units[%u]: output cell %zu (column %zu, row %zu) is also written by unit %u of gate %u of that row", fn, f, q, q / n, q % n,
                                (u32)(wk - row_first[unit_row[wk]]), row_gate[unit_row[wk]]);
        });
        if (rc != GLP_OK) return rc;
    }
    GLP_TRY(witness_sigma_decode(c, cc, fn));

    // the copy classes: the cycles of the decoded permutation, named by their smallest position; a non-routed cell is its own class
    std::vector<u32> cls(cells);
    {
        std::vector<u32> pos((size_t)nr * n);
        GLP_TRY(d2h(c, pos.data(), cc->dev_sigma_pos, pos.size() * sizeof(u32)));
        for (size_t p = 0; p < cells; p++) cls[p] = NONE;
        for (size_t p = 0; p < pos.size(); p++) {                 // ascending: the first cell of a cycle met is its smallest
            if (cls[p] != NONE) continue;
            for (size_t q = p; cls[q] == NONE; q = pos[q]) {
                cls[q] = (u32)p;
                GLP_REQUIRE(pos[q] < pos.size(), "%s: the decoded permutation leaves the routed columns", fn);
            }
        }
        for (size_t p = pos.size(); p < cells; p++) cls[p] = (u32)p;
    }
    // class_wave by class name: 0 for a class with an input, -1 = not (yet) known; two inputs in one class are refused
    std::vector<int32_t> class_wave(cells, -1);
    {
        std::vector<u32> class_input(num_inputs ? cells : 0, NONE);
        for (u32 i = 0; i < num_inputs; i++) {
            u32 &first = class_input[cls[(size_t)input_cells[i]]];
            GLP_REQUIRE(first == NONE, "%s: input_cells[%u] = %llu and input_cells[%u] = %llu lie in one copy class: one value per class", fn, first,
                        (unsigned long long)input_cells[first], i, (unsigned long long)input_cells[i]);
            first = i;
            class_wave[cls[(size_t)input_cells[i]]] = 0;
        }
    }
    // per class the units that wait for it (one entry per cell read in a class not known from the inputs)
    std::vector<u32> pending(nk, 0);
    std::vector<size_t> reader_off(cells + 1, 0);
    for (size_t k = 0; k < nk; k++)
        for_in(k, [&](size_t q) { const u32 cl = cls[q]; if (class_wave[cl] < 0) { reader_off[cl + 1]++; pending[k]++; } });
    for (size_t p = 0; p < cells; p++) reader_off[p + 1] += reader_off[p];
    std::vector<u32> readers(reader_off[cells]);
    {
        std::vector<size_t> fill(reader_off.begin(), reader_off.end() - 1);
        for (size_t k = 0; k < nk; k++)
            for_in(k, [&](size_t q) { const u32 cl = cls[q]; if (class_wave[cl] < 0) readers[fill[cl]++] = (u32)k; });
    }
    // the waves: a unit is ready once every class it reads is known; its wave is one more than the wave that made the last one known
    std::vector<int32_t> unit_wave(nk, -1);
    std::vector<u32> ready, next;
    for (size_t k = 0; k < nk; k++) if (pending[k] == 0) ready.push_back((u32)k);
    u32 num_waves = 0;
    uint64_t widest = 0, widest_free = 0;
    while (!ready.empty()) {
        num_waves++;
        uint64_t wave_free = 0;
        for (u32 k : ready) wave_free += k >= nu_total;
        widest = std::max<uint64_t>(widest, ready.size() - wave_free);
        widest_free = std::max<uint64_t>(widest_free, wave_free);
        next.clear();
        for (u32 k : ready) unit_wave[k] = (int32_t)num_waves;
        for (u32 k : ready)
            for_out(k, [&](size_t q) {
                const u32 cl = cls[q];
                if (class_wave[cl] >= 0) return;
                class_wave[cl] = (int32_t)num_waves;
                for (size_t i = reader_off[cl]; i < reader_off[cl + 1]; i++) if (--pending[readers[i]] == 0) next.push_back(readers[i]);
            });
        ready.swap(next);
    }
    std::unique_ptr<glp_witness_plan> p(new glp_witness_plan);
    p->ctx = c; p->cc = cc; p->num_inputs = num_inputs;
    if (const char *e = getenv("GLP_WITNESS_NARROW_MAX")) p->narrow_max = (u32)std::min<unsigned long long>(strtoull(e, nullptr, 10), 0xFFFFFFFFull);
    struct glp_witness_plan_info &info = p->info;
    memset(&info, 0, sizeof(info));
    info.num_waves = num_waves; info.num_units = nu_total; info.widest_wave_units = widest;
    struct glp_witness_plan_free_info &finfo = p->free_info;
    memset(&finfo, 0, sizeof(finfo));
    finfo.num_free_units = nf; finfo.widest_wave_free_units = widest_free;
    // the lists: units by wave in (row, unit) order, the source of every known class, the copies by wave in order of the destination
    p->unit_off.assign(num_waves + 2, 0);
    p->copy_off.assign(num_waves + 2, 0);
    for (size_t k = 0; k < nu_total; k++) {
        if (unit_wave[k] > 0) { p->unit_off[unit_wave[k] + 1]++; continue; }
        if (!info.num_stuck_units++) { info.stuck_row = unit_row[k]; info.stuck_gate = row_gate[unit_row[k]]; info.stuck_unit = (u32)(k - row_first[unit_row[k]]); }
    }
    for (u32 w = 0; w <= num_waves; w++) p->unit_off[w + 1] += p->unit_off[w];
    std::vector<WUnit> units(p->unit_off[num_waves + 1]);
    {
        std::vector<u32> fill(p->unit_off.begin(), p->unit_off.end() - 1);
        for (size_t k = 0; k < nu_total; k++)
            if (unit_wave[k] > 0) units[fill[unit_wave[k]]++] = WUnit{unit_row[k], row_gate[unit_row[k]] << 16 | (u32)(k - row_first[unit_row[k]])};
    }
    // the free units by wave, in the caller's order; program units are listed apart, below
    auto is_prog = [&](u32 f) { return with_programs && funits[f].kind == GLP_WGEN_PROGRAM; };
    u32 nf_prog = 0;
    for (u32 f = 0; f < nf; f++) nf_prog += is_prog(f);
    std::vector<WFree> free_list;
    if (nf) {
        if (nf > nf_prog) p->free_off.assign(num_waves + 2, 0);
        for (u32 f = 0; f < nf; f++) {
            const int32_t uw = unit_wave[nu_total + f];
            if (uw > 0) { if (!is_prog(f)) p->free_off[uw + 1]++; continue; }
            if (!finfo.num_stuck_free_units++) finfo.first_stuck_free_unit = f;
        }
    }
    if (nf > nf_prog) {
        for (u32 w = 0; w <= num_waves; w++) p->free_off[w + 1] += p->free_off[w];
        free_list.resize(p->free_off[num_waves + 1]);
        std::vector<u32> fill(p->free_off.begin(), p->free_off.end() - 1);
        for (u32 f = 0; f < nf; f++) if (!is_prog(f) && unit_wave[nu_total + f] > 0) free_list[fill[unit_wave[nu_total + f]]++] = funits[f];
    }
    // the program units by wave, sorted by program (then in the caller's order), cut into chunks of at most 64 units of one program; the
    // image: per program its code, zero-padded to a multiple of 4 words (opcode 0 does nothing), then its pool
    std::vector<WFree> prog_units;
    std::vector<WProgChunk> prog_chunks;
    std::vector<WProgEntry> prog_tab;
    std::vector<u64> prog_image;
    if (nf_prog) {
        std::vector<u32> order;
        for (u32 f = 0; f < nf; f++) if (is_prog(f) && unit_wave[nu_total + f] > 0) order.push_back(f);
        std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) {
            const int32_t wx = unit_wave[nu_total + x], wy = unit_wave[nu_total + y];
            return wx != wy ? wx < wy : funits[x].modulus < funits[y].modulus;
        });
        p->prog_chunk_off.assign(num_waves + 2, 0);
        for (size_t i = 0; i < order.size();) {
            const u32 f = order[i], w = (u32)unit_wave[nu_total + f], pr = funits[f].modulus;
            size_t j = i;
            while (j < order.size() && j - i < 64 && (u32)unit_wave[nu_total + order[j]] == w && funits[order[j]].modulus == pr) j++;
            prog_chunks.push_back(WProgChunk{pr, (u32)i, (u32)(j - i)});
            p->prog_chunk_off[w + 1]++;
            i = j;
        }
        for (u32 w = 0; w <= num_waves; w++) p->prog_chunk_off[w + 1] += p->prog_chunk_off[w];
        for (u32 f : order) prog_units.push_back(funits[f]);
        for (u32 i = 0; i < num_programs; i++) {
            const glp_witness_program_desc &pd = programs[i];
            const u32 words = (pd.num_instructions + 3) & ~3u;
            WProgEntry e;
            e.code_off = (u32)prog_image.size(); e.code_words = words; e.pool_off = e.code_off + words; e.num_inputs = pd.num_inputs;
            GLP_REQUIRE(prog_image.size() + words + pd.num_pool < NONE, "%s: the programs exceed the 2^32 - 1 words a plan addresses", fn);
            prog_image.insert(prog_image.end(), pd.code, pd.code + pd.num_instructions);
            prog_image.resize((size_t)e.code_off + words, 0);
            if (pd.num_pool) prog_image.insert(prog_image.end(), pd.pool, pd.pool + pd.num_pool);
            prog_tab.push_back(e);
            p->prog_lds = std::max<u32>(p->prog_lds, pd.num_regs * 64 * 8);
        }
    }
    std::vector<u32> source(cells, NONE);        // by class name
    p->cell_waves.assign(cells, -1);
    for (size_t q = 0; q < cells; q++) {
        const u32 cl = cls[q];
        const int32_t cw = class_wave[cl];
        if (cw < 0) continue;
        const bool written = writer[q] != NONE && unit_wave[writer[q]] > 0;
        p->cell_waves[q] = written ? unit_wave[writer[q]] : cw;
        info.num_cells_known++;
        if (source[cl] == NONE && (cw == 0 ? input_at[q] != NONE : (written && unit_wave[writer[q]] == cw))) source[cl] = (u32)q;
    }
    for (size_t q = 0; q < cells; q++) if (class_wave[cls[q]] >= 0 && source[cls[q]] != q) p->copy_off[class_wave[cls[q]] + 1]++;
    for (u32 w = 0; w <= num_waves; w++) {
        GLP_REQUIRE((size_t)p->copy_off[w] + p->copy_off[w + 1] < NONE, "%s: the copies exceed the 2^32 - 1 a plan addresses", fn);
        p->copy_off[w + 1] += p->copy_off[w];
    }
    info.num_copies = p->copy_off[num_waves + 1];
    std::vector<WCopy> copies(info.num_copies);
    {
        std::vector<u32> fill(p->copy_off.begin(), p->copy_off.end() - 1);
        for (size_t q = 0; q < cells; q++) {
            const u32 cl = cls[q];
            if (class_wave[cl] >= 0 && source[cl] != q) copies[fill[class_wave[cl]]++] = WCopy{source[cl], (u32)q};
        }
    }
    std::vector<u32> in32(num_inputs);
    for (u32 i = 0; i < num_inputs; i++) in32[i] = (u32)input_cells[i];
    int rc = GLP_OK;
    auto up = [&](auto **dev, const auto &v) {
        if (rc != GLP_OK) return;
        const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(v[0]);
        rc = c->alloc((void **)dev, bytes);
        if (rc == GLP_OK && !v.empty()) rc = h2d(c, *dev, v.data(), v.size() * sizeof(v[0]));
    };
    up(&p->dev_units, units); up(&p->dev_copies, copies); up(&p->dev_unit_off, p->unit_off); up(&p->dev_copy_off, p->copy_off); up(&p->dev_inputs, in32);
    if (nf) {
        const std::vector<u32> mod32(moduli, moduli + (size_t)num_moduli * 8);
        up(&p->dev_free_units, free_list); up(&p->dev_free_off, p->free_off); up(&p->dev_free_cells, fcells32); up(&p->dev_moduli, mod32);
    }
    if (nf_prog) { up(&p->dev_prog_chunks, prog_chunks); up(&p->dev_prog_units, prog_units); up(&p->dev_prog_tab, prog_tab); up(&p->dev_prog_image, prog_image); }
    if (rc != GLP_OK) { glp_witness_plan_free(p.release()); return rc; }
    *out = p.release();
    return GLP_OK;
}

extern "C" int glp_witness_plan_create_ex(glp_ctx *c, const glp_circuit *cc, const uint64_t *input_cells, uint32_t num_inputs,
                                          const glp_witness_free_unit *units, uint32_t num_units, const uint64_t *cells, size_t num_cells,
                                          const uint32_t *moduli, uint32_t num_moduli, glp_witness_plan **out) {
    static const char *fn = "glp_witness_plan_create_ex";
    try {
        return witness_plan_build(fn, c, cc, input_cells, num_inputs, units, num_units, cells, num_cells, moduli, num_moduli, nullptr, 0, false, out);
    } catch (const std::bad_alloc &) {       // the planner's host tables: about 40 bytes per cell
        return set_error(GLP_ERR_UNSUPPORTED, "%s: out of host memory for the planner's tables (about 40 bytes per cell of num_wires * 2^degree_bits)", fn);
    }
}

extern "C" int glp_witness_plan_create_prog(glp_ctx *c, const glp_circuit *cc, const uint64_t *input_cells, uint32_t num_inputs,
                                            const glp_witness_free_unit *units, uint32_t num_units, const uint64_t *cells, size_t num_cells,
                                            const uint32_t *moduli, uint32_t num_moduli, const glp_witness_program_desc *programs,
                                            uint32_t num_programs, glp_witness_plan **out) {
    static const char *fn = "glp_witness_plan_create_prog";
    try {
        return witness_plan_build(fn, c, cc, input_cells, num_inputs, units, num_units, cells, num_cells, moduli, num_moduli, programs, num_programs, true, out);
    } catch (const std::bad_alloc &) {
        return set_error(GLP_ERR_UNSUPPORTED, "%s: out of host memory for the planner's tables (about 40 bytes per cell of num_wires * 2^degree_bits)", fn);
    }
}

extern "C" int glp_witness_plan_create(glp_ctx *c, const glp_circuit *cc, const uint64_t *input_cells, uint32_t num_inputs, glp_witness_plan **out) {
    static const char *fn = "glp_witness_plan_create";
    try {
        return witness_plan_build(fn, c, cc, input_cells, num_inputs, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, false, out);
    } catch (const std::bad_alloc &) {
        return set_error(GLP_ERR_UNSUPPORTED, "%s: out of host memory for the planner's tables (about 40 bytes per cell of num_wires * 2^degree_bits)", fn);
    }
}

extern "C" int glp_witness_plan_free_info(const glp_witness_plan *p, struct glp_witness_plan_free_info *out) {
    GLP_REQUIRE(p, "glp_witness_plan_free_info: plan is null");
    GLP_REQUIRE(out, "glp_witness_plan_free_info: out is null");
    *out = p->free_info;
    return GLP_OK;
}

extern "C" int glp_witness_plan_info(const glp_witness_plan *p, struct glp_witness_plan_info *out) {
    GLP_REQUIRE(p, "glp_witness_plan_info: plan is null");
    GLP_REQUIRE(out, "glp_witness_plan_info: out is null");
    *out = p->info;
    return GLP_OK;
}

extern "C" int glp_witness_plan_cell_waves(const glp_witness_plan *p, int32_t *waves_out) {
    GLP_REQUIRE(p, "glp_witness_plan_cell_waves: plan is null");
    GLP_REQUIRE(waves_out, "glp_witness_plan_cell_waves: waves_out is null");
    memcpy(waves_out, p->cell_waves.data(), p->cell_waves.size() * sizeof(int32_t));
    return GLP_OK;
}

extern "C" int glp_witness_generate(glp_ctx *c, const glp_witness_plan *p, uint32_t num_proofs, const uint64_t *input_values, uint64_t *dev_wires,
                                    uint32_t flags) {
    static const char *fn = "glp_witness_generate";
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    GLP_REQUIRE(p, "%s: plan is null", fn);
    GLP_REQUIRE(dev_wires, "%s: dev_wires is null", fn);
    GLP_REQUIRE(p->ctx == c, "%s: plan belongs to another ctx", fn);
    GLP_REQUIRE(input_values || p->num_inputs == 0, "%s: input_values is null, the plan has %u inputs", fn, p->num_inputs);
    GLP_REQUIRE((flags & ~GLP_WITNESS_GEN_ZERO_FIRST) == 0, "%s: flags = 0x%x has bits other than GLP_WITNESS_GEN_ZERO_FIRST", fn, flags);
    const u32 K = num_proofs, ni = p->num_inputs;
    GLP_REQUIRE(K >= 1 && K <= WGEN_MAX_PROOFS, "%s: num_proofs = %u outside 1..%u", fn, K, WGEN_MAX_PROOFS);
    const glp_circuit *cc = p->cc;
    const u32 nw = cc->d.num_wires;
    const size_t n = (size_t)1 << cc->d.degree_bits;
    GLP_REQUIRE((size_t)K * nw <= BATCH_MAX_BYTES / (8 * n), "%s: wires too large (num_proofs * num_wires * 2^degree_bits words)", fn);
    for (u32 k = 0; k < K && ni; k++) {
        const size_t bad = first_noncanonical(input_values + (size_t)k * ni, ni);
        GLP_REQUIRE(bad == ni, "%s: input_values: proof %u, input %zu = 0x%016llx is not a canonical field element (>= p)", fn, k, bad,
                    (unsigned long long)input_values[(size_t)k * ni + (bad == ni ? 0 : bad)]);
    }
    GLP_TRY(bind(c));
    const glp_witness_plan *pm = p;                                // the value buffer grows with the largest batch seen
    const size_t nvals = (size_t)K * ni;
    if (nvals > pm->vals_cap) {
        GLP_HIP(hipStreamSynchronize(c->stream));
        c->release(pm->dev_vals);
        pm->dev_vals = nullptr; pm->vals_cap = 0;
        GLP_TRY(c->alloc((void **)&pm->dev_vals, nvals * 8));
        pm->vals_cap = nvals;
    }
    if (nvals) GLP_TRY(h2d(c, pm->dev_vals, input_values, nvals * 8));
    WGen g;
    memset(&g, 0, sizeof(g));
    g.a.wires = dev_wires; g.a.consts = cc->dev_consts; g.a.gates = cc->dev_gates;
    g.a.lg = cc->d.degree_bits; g.a.nsel = cc->d.num_selectors; g.a.num_gates = cc->d.num_gates; g.a.only_advice = 0; g.a.nr = cc->d.num_routed_wires;
    g.units = p->dev_units; g.copies = p->dev_copies; g.unit_off = p->dev_unit_off; g.copy_off = p->dev_copy_off; g.inputs = p->dev_inputs;
    g.vals = p->dev_vals; g.num_inputs = ni; g.nw = nw;
    const bool has_free = !p->free_off.empty();
    if (has_free) { g.free_units = p->dev_free_units; g.free_off = p->dev_free_off; g.free_cells = p->dev_free_cells; g.moduli = p->dev_moduli; }
    StageScope st(c, "witness_generate", 16.0 * K * p->info.num_cells_known);
    if (flags & GLP_WITNESS_GEN_ZERO_FIRST) GLP_HIP(hipMemsetAsync(dev_wires, 0, (size_t)K * nw * n * 8, c->stream));
    // a wave is wide (one launch for its units, one for its copies) while the proofs alone do not fill the chip and it holds more than
    // narrow_max units; runs of the other waves are walked by one workgroup per proof
    const u32 nwaves = p->info.num_waves;
    auto free_count = [&](u32 w) -> size_t { return has_free ? p->free_off[w + 1] - p->free_off[w] : 0; };      // wave 0 holds none
    // a wave with program units is always wide: its chunks get a launch of their own between its units and its copies
    auto prog_count = [&](u32 w) -> u32 { return p->prog_chunk_off.empty() ? 0 : p->prog_chunk_off[w + 1] - p->prog_chunk_off[w]; };
    WProgArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.wires = dev_wires; pa.image = p->dev_prog_image; pa.progs = p->dev_prog_tab; pa.chunks = p->dev_prog_chunks; pa.units = p->dev_prog_units;
    pa.cells = p->dev_free_cells; pa.nw = nw; pa.lg = cc->d.degree_bits;
    auto wide = [&](u32 w) {
        const size_t cnt = (w == 0 ? ni : p->unit_off[w + 1] - p->unit_off[w]) + free_count(w);
        return prog_count(w) || (K < (u32)c->num_cus && cnt > p->narrow_max);
    };
    for (u32 w = 0; w <= nwaves;) {
        if (wide(w)) {
            const size_t cnt = w == 0 ? ni : p->unit_off[w + 1] - p->unit_off[w], ncp = p->copy_off[w + 1] - p->copy_off[w], nfr = free_count(w);
            if (cnt) hipLaunchKernelGGL(k_witness_units, dim3((unsigned)((cnt + 255) / 256), K), dim3(256), 0, c->stream, g, w);
            if (nfr) hipLaunchKernelGGL(k_witness_free, dim3((unsigned)((nfr + 63) / 64), K), dim3(64), 0, c->stream, g, w);
            if (const u32 npc = prog_count(w)) hipLaunchKernelGGL(k_witness_programs, dim3(npc, K), dim3(64), p->prog_lds, c->stream, pa, p->prog_chunk_off[w]);
            if (ncp) hipLaunchKernelGGL(k_witness_copies, dim3((unsigned)((ncp + 255) / 256), K), dim3(256), 0, c->stream, g, w);
            w++;
        } else {
            u32 w1 = w;
            while (w1 < nwaves && !wide(w1 + 1)) w1++;
            if (has_free) hipLaunchKernelGGL(k_witness_waves<true>, dim3(K), dim3(256), 0, c->stream, g, w, w1);
            else hipLaunchKernelGGL(k_witness_waves<false>, dim3(K), dim3(256), 0, c->stream, g, w, w1);
            w = w1 + 1;
        }
        GLP_HIP(hipGetLastError());
    }
    return GLP_OK;
}

extern "C" int glp_witness_read_cells(glp_ctx *c, const glp_circuit *cc, uint32_t num_proofs, const uint64_t *dev_wires, const uint64_t *cells,
                                      uint32_t num_cells, uint64_t *out) {
    static const char *fn = "glp_witness_read_cells";
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    GLP_REQUIRE(cc, "%s: circuit is null", fn);
    GLP_REQUIRE(dev_wires, "%s: dev_wires is null", fn);
    GLP_REQUIRE(cells, "%s: cells is null", fn);
    GLP_REQUIRE(out, "%s: out is null", fn);
    GLP_REQUIRE(cc->ctx == c, "%s: circuit belongs to another ctx", fn);
    GLP_REQUIRE(num_proofs >= 1 && num_proofs <= WGEN_MAX_PROOFS, "%s: num_proofs = %u outside 1..%u", fn, num_proofs, WGEN_MAX_PROOFS);
    GLP_REQUIRE(num_cells >= 1, "%s: num_cells is 0", fn);
    const size_t per_proof = (size_t)cc->d.num_wires << cc->d.degree_bits;
    GLP_REQUIRE(per_proof < ((size_t)1 << 32), "%s: num_wires * 2^degree_bits = %zu positions, cells are named below 2^32", fn, per_proof);
    std::vector<u32> c32(num_cells);
    for (u32 i = 0; i < num_cells; i++) {
        GLP_REQUIRE(cells[i] < per_proof, "%s: cells[%u] = %llu is out of range (num_wires * 2^degree_bits = %zu cells)", fn, i, (unsigned long long)cells[i], per_proof);
        c32[i] = (u32)cells[i];
    }
    GLP_TRY(bind(c));
    Scratch tmp(c);
    u32 *dev_cells;
    u64 *dev_out;
    GLP_TRY(tmp.array(&dev_cells, num_cells));
    GLP_TRY(tmp.words(&dev_out, (size_t)num_proofs * num_cells));
    GLP_TRY(h2d(c, dev_cells, c32.data(), (size_t)num_cells * 4));
    hipLaunchKernelGGL(k_witness_read_cells, dim3((num_cells + 255) / 256, num_proofs), dim3(256), 0, c->stream, dev_wires, dev_cells, dev_out, num_cells, per_proof);
    GLP_HIP(hipGetLastError());
    return d2h(c, out, dev_out, (size_t)num_proofs * num_cells * 8);
}
