// witness.hip -- witness generation on the GPU: the row-local half (glp_witness_fill) and, over the same
// per-unit body, the dataflow half (glp_witness_plan_*, glp_witness_generate: second part of this file; caller-defined generators as
// unit programs: witness_program.inc).  What is here: the generator bodies (witness_unit), the kernels, glp_witness_fill, the role
// queries, the planner's driver (witness_plan_create), glp_witness_generate and glp_witness_read_cells.  The planner itself -- the unit
// table, the records of a plan's lists, every check and index of a plan -- is host-only text in witness_plan.h.
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
// Every value written is a canonical field element; inputs are reduced mod p as they are loaded, which is the canonical u64
// that `to_canonical_u64()` hands to the Rust generators.
#include <stdlib.h>
#include <new>
#include "common.h"
#include "poseidon.h"
#include "prover_types.h"
#include "biguint_dev.h"
#include "witness_plan.h"

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

// One unit of one row: generator `unit` (< witness_gate_units, witness_plan.h) of gate g on the row W points at (wire j -> W[j * n], gate constant
// i -> GC[i * n]).  k_witness_fill runs every unit of a row; the wave kernels below run the units a plan lists.  WHICH = 1 keeps only
// the gates with one unit per op, WHICH = 2 only those with one unit per row (k_witness_fill loops over the first kind alone, so that
// nothing of a PoseidonGate row is hoisted out of a loop it runs once); 0 keeps all.
template <int WHICH = 0, bool RAW = false>
__device__ __forceinline__ void witness_unit(const WArgs &a, const DevGate &g, u64 *W, const u64 *GC, size_t n, u32 unit) {
    const u32 nr = a.only_advice ? a.nr : 0xFFFFFFFFu;         // only_advice: columns < nr (routed) are never written
    constexpr bool ONE = WHICH != 1, PER_OP = WHICH != 2;      // which cases this instance keeps: gates of one unit per row, gates of one per op
    const u32 i = unit;                                        // the op of a gate with one generator per op
#define WR(col, val) do { const u32 _c = (col); if (!a.only_advice || _c >= nr) W[(size_t)_c * n] = (val); } while (0)
#define RD(col) (RAW ? canon(W[(size_t)(col) * n]) : W[(size_t)(col) * n])    // RAW: a caller's device words (glp_witness_fill), reduced mod p as they are loaded
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

// One thread = one trace row (its gate: witness_row_gate, witness_plan.h): every unit of the row.  Rows of one gate type are contiguous in every circuit the builder emits, so a
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
    if (nu) witness_unit<2, true>(a, g, W, GC, n, 0);                          // a gate with one unit per row: nothing for the others
    for (u32 u = 0; u < nu; u++) witness_unit<1, true>(a, g, W, GC, n, u);    // a gate with one unit per op: nothing for the others
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

// Which wire columns glp_witness_fill writes on rows of gate `gate_index` (1) and which it reads as inputs (2); 0 = untouched
// (witness_unit_roles, witness_plan.h).
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
// planner: no value read from a witness is an address (RandomAccessGate's index keeps its idx < vs guard in witness_unit).  The planner
// is host-only text in witness_plan.h (the records of the lists, the unit table and the six stages); witness_plan_create below drives it.
namespace {
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
// The random cells of a plan (include/glp.h, RANDOM CELLS): one lane per block of eight cells, blockIdx.y = proof.  One permutation of
// the seed, the tag and the block's number gives the block's eight values (the rate words; the capacity words go nowhere).  The
// positions were range-checked by the planner; every count here is the 8 of the block, the tail of the last block is masked.
__global__ __launch_bounds__(256) void k_witness_random(u64 *wires, const u32 *cells, u32 num_random, size_t per_proof, u64 seed0, u64 seed1, u64 seed2,
                                                        u64 seed3) {
    const u32 b = blockIdx.x * 256 + threadIdx.x;
    if ((u64)b * 8 >= num_random) return;
    const u32 left = num_random - b * 8;                  // >= 1
    u32 at[8];
#pragma unroll
    for (u32 j = 0; j < 8; j++) at[j] = j < left ? cells[(size_t)b * 8 + j] : NONE;
    u64 s[12] = {seed0, seed1, seed2, add(seed3, (u64)blockIdx.y), (u64)GLP_SALT_TAG_WITNESS, (u64)b, 0 /* b >> 32: a plan lists fewer than 2^32 cells */, 0, 0, 0, 0, 0};
    pos::permute(s);
    u64 *W = wires + (size_t)blockIdx.y * per_proof;
#pragma unroll
    for (u32 j = 0; j < 8; j++) if (at[j] != NONE) W[at[j]] = s[j];
}
}  // namespace

#include "witness_program.inc"

struct glp_witness_plan : WPlanKept {              // the figures, cell_waves and the wave offsets stay on the host (witness_plan.h)
    glp_ctx *ctx = nullptr;
    const glp_circuit *cc = nullptr;
    u32 num_inputs = 0, num_random = 0, narrow_max = WITNESS_NARROW_MAX_DEFAULT;
    u32 *dev_random = nullptr;                     // the random cells in the caller's order; null without any
    WUnit *dev_units = nullptr;
    WCopy *dev_copies = nullptr;
    u32 *dev_unit_off = nullptr, *dev_copy_off = nullptr, *dev_inputs = nullptr;
    WFree *dev_free_units = nullptr;
    u32 *dev_free_off = nullptr, *dev_free_cells = nullptr, *dev_moduli = nullptr;
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
    c->release(p->dev_inputs); c->release(p->dev_random); c->release(p->dev_vals);
    c->release(p->dev_free_units); c->release(p->dev_free_off); c->release(p->dev_free_cells); c->release(p->dev_moduli);
    c->release(p->dev_prog_chunks); c->release(p->dev_prog_units); c->release(p->dev_prog_tab); c->release(p->dev_prog_image);
    delete p;
}

// The driver of the planner (witness_plan.h) behind the four entry points: the stages in their order, between them what needs the device
// (the selectors for the gate of every row, the decoded permutation), at the end the upload; it holds the guard of the host tables' allocation.
static int witness_plan_create(glp_ctx *c, const glp_circuit *cc, const WPlanRequest &rq, glp_witness_plan **out) try {
    const char *fn = rq.fn;
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    GLP_REQUIRE(cc, "%s: circuit is null", fn);
    GLP_REQUIRE(out, "%s: out is null", fn);
    GLP_TRY(wplan_check_pointers(rq));
    GLP_REQUIRE(cc->ctx == c, "%s: circuit belongs to another ctx", fn);
    for (u32 i = 0; i < rq.num_programs; i++) {
        char where[96];
        snprintf(where, sizeof(where), "%s: programs[%u]", fn, i);
        GLP_TRY(witness_program_check(where, rq.programs + i));
    }
    const glp_circuit_desc &d = cc->d;
    WPlanCircuit cv = {d.degree_bits, d.num_wires, d.num_routed_wires, d.num_gates, cc->gates.data(), nullptr, nullptr};
    const size_t n = cv.n();
    WPlanState s;
    GLP_TRY(wplan_check_request(rq, cv, s));
    GLP_TRY(wplan_check_free_units(rq, cv, s));
    GLP_TRY(bind(c));
    std::vector<u32> row_gate(n);
    {
        std::vector<u64> sel((size_t)d.num_selectors * n);
        GLP_TRY(d2h(c, sel.data(), cc->dev_consts, sel.size() * 8));
        for (size_t r = 0; r < n; r++) { const u32 gi = witness_row_gate(sel.data(), d.num_selectors, n, r); row_gate[r] = gi < cv.ng ? gi : NONE; }
    }
    cv.row_gate = row_gate.data();
    GLP_TRY(wplan_units(rq, cv, s));
    GLP_TRY(witness_sigma_decode(c, cc, fn));
    {
        std::vector<u32> pos((size_t)cv.nr * n);
        GLP_TRY(d2h(c, pos.data(), cc->dev_sigma_pos, pos.size() * sizeof(u32)));
        cv.pos = pos.data();
        GLP_TRY(wplan_classes(rq, cv, s));
        cv.pos = nullptr;
    }
    GLP_TRY(wplan_waves(rq, cv, s));
    GLP_TRY(wplan_lists(rq, cv, s));
    const WPlanLists &L = s.lists;
    std::unique_ptr<glp_witness_plan> p(new glp_witness_plan);
    p->ctx = c; p->cc = cc; p->num_inputs = rq.num_inputs; p->num_random = rq.num_random;
    if (const char *e = getenv("GLP_WITNESS_NARROW_MAX")) p->narrow_max = (u32)std::min<unsigned long long>(strtoull(e, nullptr, 10), 0xFFFFFFFFull);
    static_cast<WPlanKept &>(*p) = std::move(static_cast<WPlanKept &>(s.lists));
    int rc = GLP_OK;
    auto up = [&](auto **dev, const auto &v) {
        if (rc != GLP_OK) return;
        const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(v[0]);
        rc = c->alloc((void **)dev, bytes);
        if (rc == GLP_OK && !v.empty()) rc = h2d(c, *dev, v.data(), v.size() * sizeof(v[0]));
    };
    up(&p->dev_units, L.units); up(&p->dev_copies, L.copies); up(&p->dev_unit_off, p->unit_off); up(&p->dev_copy_off, p->copy_off); up(&p->dev_inputs, L.inputs);
    if (rq.num_random) up(&p->dev_random, L.random);
    if (rq.num_units) {
        const std::vector<u32> mod32(rq.moduli, rq.moduli + (size_t)rq.num_moduli * 8);
        up(&p->dev_free_units, L.free_units); up(&p->dev_free_off, p->free_off); up(&p->dev_free_cells, L.free_cells); up(&p->dev_moduli, mod32);
    }
    if (!p->prog_chunk_off.empty()) { up(&p->dev_prog_chunks, L.prog_chunks); up(&p->dev_prog_units, L.prog_units); up(&p->dev_prog_tab, L.prog_tab); up(&p->dev_prog_image, L.prog_image); }
    if (rc != GLP_OK) { glp_witness_plan_free(p.release()); return rc; }
    *out = p.release();
    return GLP_OK;
} catch (const std::bad_alloc &) {       // the planner's host tables: about 40 bytes per cell
    return set_error(GLP_ERR_UNSUPPORTED, "%s: out of host memory for the planner's tables (about 40 bytes per cell of num_wires * 2^degree_bits)", rq.fn);
}

extern "C" int glp_witness_plan_create_ex(glp_ctx *c, const glp_circuit *cc, const uint64_t *input_cells, uint32_t num_inputs,
                                          const glp_witness_free_unit *units, uint32_t num_units, const uint64_t *cells, size_t num_cells,
                                          const uint32_t *moduli, uint32_t num_moduli, glp_witness_plan **out) {
    // without programs kind GLP_WGEN_PROGRAM stays an unknown kind
    return witness_plan_create(c, cc, {"glp_witness_plan_create_ex", input_cells, num_inputs, nullptr, 0, units, num_units, cells, num_cells, moduli, num_moduli, nullptr, 0, false}, out);
}

extern "C" int glp_witness_plan_create_prog(glp_ctx *c, const glp_circuit *cc, const uint64_t *input_cells, uint32_t num_inputs,
                                            const glp_witness_free_unit *units, uint32_t num_units, const uint64_t *cells, size_t num_cells,
                                            const uint32_t *moduli, uint32_t num_moduli, const glp_witness_program_desc *programs,
                                            uint32_t num_programs, glp_witness_plan **out) {
    return witness_plan_create(c, cc, {"glp_witness_plan_create_prog", input_cells, num_inputs, nullptr, 0, units, num_units, cells, num_cells, moduli, num_moduli, programs, num_programs, true}, out);
}

extern "C" int glp_witness_plan_create_rand(glp_ctx *c, const glp_circuit *cc, const uint64_t *input_cells, uint32_t num_inputs,
                                            const uint64_t *random_cells, uint32_t num_random, const glp_witness_free_unit *units, uint32_t num_units,
                                            const uint64_t *cells, size_t num_cells, const uint32_t *moduli, uint32_t num_moduli,
                                            const glp_witness_program_desc *programs, uint32_t num_programs, glp_witness_plan **out) {
    return witness_plan_create(c, cc, {"glp_witness_plan_create_rand", input_cells, num_inputs, random_cells, num_random, units, num_units, cells, num_cells, moduli, num_moduli, programs, num_programs, true}, out);
}

extern "C" uint32_t glp_witness_plan_num_random(const glp_witness_plan *p) { return p ? p->num_random : 0; }

extern "C" int glp_witness_plan_create(glp_ctx *c, const glp_circuit *cc, const uint64_t *input_cells, uint32_t num_inputs, glp_witness_plan **out) {
    return witness_plan_create(c, cc, {"glp_witness_plan_create", input_cells, num_inputs, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, false}, out);
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
    u64 seed[4] = {0, 0, 0, 0};                                    // random cells: one seed per call, proof k draws with seed3 + k
    if (p->num_random) GLP_TRY(salt_seed_draw(c, seed));
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
    // the random cells belong to wave 0, beside the scatter of the inputs and before its copies, whichever form wave 0 takes
    if (p->num_random) {
        hipLaunchKernelGGL(k_witness_random, dim3((unsigned)(((size_t)p->num_random + 8 * 256 - 1) / (8 * 256)), K), dim3(256), 0, c->stream, dev_wires, p->dev_random, p->num_random,
                           (size_t)nw * n, seed[0], seed[1], seed[2], seed[3]);
        GLP_HIP(hipGetLastError());
    }
    const u32 nwaves = p->info.num_waves;
    auto free_count = [&](u32 w) -> size_t { return has_free ? p->free_off[w + 1] - p->free_off[w] : 0; };      // wave 0 holds none
    // a wave with program units is always wide: its chunks get a launch of their own between its units and its copies
    auto prog_count = [&](u32 w) -> u32 { return p->prog_chunk_off.empty() ? 0 : p->prog_chunk_off[w + 1] - p->prog_chunk_off[w]; };
    WProgArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.wires = dev_wires; pa.image = p->dev_prog_image; pa.progs = p->dev_prog_tab; pa.chunks = p->dev_prog_chunks; pa.units = p->dev_prog_units;
    pa.cells = p->dev_free_cells; pa.nw = nw; pa.lg = cc->d.degree_bits;
    auto wide = [&](u32 w) {
        const size_t cnt = (w == 0 ? (size_t)ni + p->num_random : p->unit_off[w + 1] - p->unit_off[w]) + free_count(w);      // wave 0: inputs and random cells
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
