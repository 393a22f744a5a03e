// witness_plan.h -- the planner of the dataflow half of witness generation (include/glp.h) as host-only stages.  No HIP in here: given
// include/glp.h and biguint_dev.h it compiles with a plain g++, and examples/witness_plan_host.cpp runs it under the host sanitizers
// (tests/test_witness_plan_host.py).  Every index the wave kernels of witness.hip and witness_program.inc use unchecked is built and
// range-checked here: the records of the lists (kernel argument types, in the unnamed namespace), the unit table, the gate of a row, and
// the stages 1 wplan_check_pointers + wplan_check_request, 2 wplan_check_free_units, 3 wplan_units, 4 wplan_classes, 5 wplan_waves,
// 6 wplan_lists, run in that order by witness_plan_create (witness.hip), which reads the selectors and the decoded permutation back from
// the device between them.  The refusals keep that order and go through glp::set_error (the library's is common.h's; a host program
// supplies one).  Host memory: about 40 bytes per cell of num_wires * n while the stages run -- add no table with one entry per cell.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/glp.h"
#include "biguint_dev.h"

typedef uint64_t u64;
typedef uint32_t u32;
#if defined(__HIPCC__) || defined(__CUDACC__)
#define WPLAN_HD __host__ __device__ __forceinline__
#else
#define WPLAN_HD inline
#endif
namespace glp { int set_error(int code, const char *fmt, ...); }
#define WPLAN_REQUIRE(cond, ...) do { if (!(cond)) return glp::set_error(GLP_ERR_ARG, __VA_ARGS__); } while (0)
#define WPLAN_TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)

namespace {
constexpr u32 NONE = 0xFFFFFFFFu;
struct WUnit { u32 row, gu; };          // gu = gate << 16 | unit
struct WCopy { u32 src, dst; };         // flat positions col * n + row
typedef glp_witness_free_unit WFree;    // a free unit as the caller gave it; cell_begin points into the plan's 32-bit copy of cells[]
static_assert(sizeof(WFree) == 24, "glp_witness_free_unit: three u32 and six u16");
struct WProgChunk { u32 prog, first, count; };      // units[first .. first + count) of the plan's program-unit list, count <= 64
struct WProgEntry { u32 code_off, code_words, pool_off, num_inputs; };      // offsets into the image; code zero-padded to a multiple of 4 words

// How many independent generators (units) a row of a gate has; the table of include/glp.h ("witness generation, the dataflow half").
WPLAN_HD u32 witness_gate_units(u32 type, u32 p0, u32 p1) {
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

// the row's gate: the selector polynomial of its group holds the gate index, every other selector UNUSED.  One text for k_witness_fill,
// the witness checker's kernels (witness_check.inc, circuit_program.inc) and the planner's driver
WPLAN_HD u32 witness_row_gate(const u64 *consts, u32 nsel, size_t n, size_t row) {
    u32 gi = 0xFFFFFFFFu;
    for (u32 s = 0; s < nsel; s++) {
        const u64 v = consts[(size_t)s * n + row];
        if (nsel == 1 || v != 0xFFFFFFFFull) gi = (u32)v;
    }
    return gi;
}

constexpr u32 ALL_UNITS = 0xFFFFFFFFu;
// Which wire columns unit `unit` of a row of gate g writes (1) and which it reads as inputs (2); 0 = untouched.  ALL_UNITS: the whole
// row, what glp_witness_fill does -- the union of the units, by construction.
inline void witness_unit_roles(const glp_gate &g, u32 nw, u32 unit, uint8_t *role_out) {
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

// The shape of a free unit's kind: which of len[0..5] are operands, which of them are single cells, which is a divisor.  0 = unknown kind.
struct WFreeShape { u32 operands; u32 single; int divisor; };     // bit i of single: len[i] must be 1
inline WFreeShape witness_free_shape(u32 kind) {
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

// What the caller of glp_witness_plan_create* handed in; fn, the entry point, opens every message.  with_programs: GLP_WGEN_PROGRAM is a
// known kind (glp_witness_plan_create_prog).
struct WPlanRequest {
    const char *fn;
    const uint64_t *input_cells; u32 num_inputs;
    const uint64_t *random_cells; u32 num_random;      // wave-0 sources as the inputs are; their values come from the PRF (glp_witness_plan_create_rand)
    const glp_witness_free_unit *units; u32 num_units;
    const uint64_t *cells; size_t num_cells;
    const u32 *moduli; u32 num_moduli;               // [num_moduli][8]
    const glp_witness_program_desc *programs; u32 num_programs;
    bool with_programs;
    bool is_prog(u32 f) const { return with_programs && units[f].kind == GLP_WGEN_PROGRAM; }
};
// The circuit as the planner sees it, plain host arrays: gates[ng] (type, p0, p1 are read), from stage 3 on row_gate[n] (NONE: a row of
// no gate), in stage 4 the decoded permutation pos[nr * n] (flat positions); nr <= nw.
struct WPlanCircuit {
    u32 lg, nw, nr, ng;
    const glp_gate *gates;
    const u32 *row_gate, *pos;
    size_t n() const { return (size_t)1 << lg; }
    size_t cells() const { return (size_t)nw << lg; }
};
// What a plan keeps on the host, and with it what it uploads.  Wave w of a list: items[off[w] .. off[w + 1]), off is [num_waves + 2].
struct WPlanKept {
    struct glp_witness_plan_info info = {};
    struct glp_witness_plan_free_info free_info = {};
    std::vector<int32_t> cell_waves;                  // [num_wires][n]
    std::vector<u32> unit_off, copy_off;
    std::vector<u32> free_off, prog_chunk_off;        // empty without free units that are no program units / without program units
    u32 prog_lds = 0;                                 // bytes of LDS a chunk's workgroup asks for: the widest register file of the programs
};
struct WPlanLists : WPlanKept {
    std::vector<WUnit> units;                         // by wave, in (row, unit) order; wave 0 holds none
    std::vector<WCopy> copies;                        // by wave, in order of the destination
    std::vector<u32> inputs, free_cells;              // input_cells and cells[], 32 bits each (NONE: GLP_WGEN_NO_CELL)
    std::vector<u32> random;                          // random_cells, 32 bits each, in the caller's order
    std::vector<WFree> free_units, prog_units;        // by wave, in the caller's order | sorted by (wave, program), then in the caller's order
    std::vector<WProgChunk> prog_chunks;              // by wave: at most 64 units of one program each
    std::vector<WProgEntry> prog_tab;
    std::vector<u64> prog_image;                      // per program its code, zero-padded to a multiple of 4 words (opcode 0 does nothing), then its pool
};
// The planner's tables: each stage reads what the stages before it left and adds its own (the number in front).
struct WPlanState {
    std::vector<u32> input_at;                        // 1: [cells] which input names a cell, num_inputs + i for random cell i (NONE: none)
    std::vector<u32> f_n[2], fcells32;                // 2: per free unit its input [0] and output [1] cells; cells[] in 32 bits
    std::vector<std::vector<std::vector<u32>>> g[2];  // 3: per gate and unit the columns read [0] and written [1]
    std::vector<size_t> row_first;                    //    [n + 1]: unit k of the plan = unit k - row_first[row] of its row
    std::vector<u32> unit_row, writer;                //    [nu_total] (the free units follow: unit nu_total + f); [cells] the unit that writes a cell
    size_t nu_total = 0, nk = 0;
    std::vector<u32> cls;                             // 4: [cells] the copy class of a cell, named by its smallest position
    std::vector<int32_t> class_wave, unit_wave;       // 4, 5: by class name, 0 for a class with an input, -1 = not (yet) known | 5: [nk], -1 = stuck
    WPlanLists lists;                                 // 5: the number of waves and the widest; 6: the rest
};

// the cells unit k reads (out = 0) or writes (out = 1); an output that is not placed is skipped
template <class V> inline void wplan_cells(const WPlanRequest &rq, const WPlanCircuit &cv, const WPlanState &s, size_t k, int out, V &&visit) {
    if (k < s.nu_total) { const size_t r = s.unit_row[k]; for (u32 col : s.g[out][cv.row_gate[r]][k - s.row_first[r]]) visit((size_t)col * cv.n() + r); return; }
    const u32 f = (u32)(k - s.nu_total), *run = s.fcells32.data() + rq.units[f].cell_begin + (out ? s.f_n[0][f] : 0);
    for (u32 i = 0; i < s.f_n[out][f]; i++) if (run[i] != NONE) visit((size_t)run[i]);
}

// Bucket items by wave: the one place that counts, prefix-sums and fills.  each(put) calls put(wave, item) for every item, and is run
// twice; then items[off[w] .. off[w + 1]) are the items of wave w in the order each() put them.
template <class T, class Each>
inline int wplan_bucket(const char *fn, const char *what, u32 num_waves, Each &&each, std::vector<u32> &off, std::vector<T> &items) {
    off.assign((size_t)num_waves + 2, 0);
    each([&](u32 w, const T &) { off[w + 1]++; });
    for (u32 w = 0; w <= num_waves; w++) {
        WPLAN_REQUIRE((size_t)off[w] + off[w + 1] < NONE, "%s: the %s exceed the 2^32 - 1 a plan addresses", fn, what);
        off[w + 1] += off[w];
    }
    items.resize(off[num_waves + 1]);
    std::vector<u32> fill(off.begin(), off.end() - 1);
    each([&](u32 w, const T &item) { items[fill[w]++] = item; });
    return GLP_OK;
}

// ---- 1. the request: null pointers (the driver checks the programs between the two) | the bounds, the input cells, the moduli
inline int wplan_check_pointers(const WPlanRequest &rq) {
    WPLAN_REQUIRE(rq.input_cells || rq.num_inputs == 0, "%s: input_cells is null, num_inputs = %u", rq.fn, rq.num_inputs);
    WPLAN_REQUIRE(rq.random_cells || rq.num_random == 0, "%s: random_cells is null, num_random = %u", rq.fn, rq.num_random);
    WPLAN_REQUIRE(rq.units || rq.num_units == 0, "%s: units is null, num_units = %u", rq.fn, rq.num_units);
    WPLAN_REQUIRE(rq.cells || rq.num_cells == 0, "%s: cells is null, num_cells = %zu", rq.fn, rq.num_cells);
    WPLAN_REQUIRE(rq.moduli || rq.num_moduli == 0, "%s: moduli is null, num_moduli = %u", rq.fn, rq.num_moduli);
    WPLAN_REQUIRE(rq.programs || rq.num_programs == 0, "%s: programs is null, num_programs = %u", rq.fn, rq.num_programs);
    return GLP_OK;
}
inline int wplan_check_request(const WPlanRequest &rq, const WPlanCircuit &cv, WPlanState &s) {
    const char *fn = rq.fn;
    const size_t cells = cv.cells();
    // one short of the decoded sigma's 2^32: position 2^32 - 1 is the planner's "none"
    WPLAN_REQUIRE(cells < ((size_t)1 << 32), "%s: num_wires * 2^degree_bits = %zu positions, a plan addresses fewer than 2^32 (the bound of the decoded sigma)", fn, cells);
    WPLAN_REQUIRE(cv.ng <= 0xFFFF, "%s: num_gates = %u, a plan names at most 65535 gates", fn, cv.ng);
    for (u32 i = 0; i < rq.num_inputs; i++)
        WPLAN_REQUIRE(rq.input_cells[i] < cells, "%s: input_cells[%u] = %llu is out of range (num_wires * 2^degree_bits = %zu cells)", fn, i,
                      (unsigned long long)rq.input_cells[i], cells);
    s.input_at.assign(cells, NONE);                   // a cell listed twice is refused
    for (u32 i = 0; i < rq.num_inputs; i++) {
        u32 &at = s.input_at[(size_t)rq.input_cells[i]];
        WPLAN_REQUIRE(at == NONE, "%s: input_cells[%u] = %llu is listed twice (also input_cells[%u])", fn, i, (unsigned long long)rq.input_cells[i], at);
        at = i;
    }
    // the random cells: wave-0 sources like the inputs, so a cell is one or the other, once
    WPLAN_REQUIRE((size_t)rq.num_inputs + rq.num_random < NONE, "%s: num_inputs + num_random = %zu, a plan addresses fewer than 2^32 - 1", fn,
                  (size_t)rq.num_inputs + rq.num_random);
    for (u32 i = 0; i < rq.num_random; i++)
        WPLAN_REQUIRE(rq.random_cells[i] < cells, "%s: random_cells[%u] = %llu is out of range (num_wires * 2^degree_bits = %zu cells)", fn, i,
                      (unsigned long long)rq.random_cells[i], cells);
    for (u32 i = 0; i < rq.num_random; i++) {
        const unsigned long long cell = rq.random_cells[i];
        u32 &at = s.input_at[(size_t)cell];
        WPLAN_REQUIRE(at == NONE || at < rq.num_inputs, "%s: random_cells[%u] = %llu is listed twice (also random_cells[%u])", fn, i, cell, at - rq.num_inputs);
        WPLAN_REQUIRE(at == NONE, "%s: random_cells[%u] = %llu is also input_cells[%u]", fn, i, cell, at);
        at = rq.num_inputs + i;
    }
    WPLAN_REQUIRE(rq.num_cells < NONE, "%s: num_cells = %zu, a plan addresses fewer than 2^32 - 1", fn, rq.num_cells);
    for (u32 i = 0; i < rq.num_moduli; i++) {
        const uint32_t *m = rq.moduli + (size_t)i * 8;
        WPLAN_REQUIRE(m[0] & 1, "%s: moduli[%u] is even", fn, i);
        WPLAN_REQUIRE(big::used_limbs(m, 8) > 1 || m[0] >= 3, "%s: moduli[%u] = %u is below 3", fn, i, m[0]);
    }
    return GLP_OK;
}

// ---- 2. the free units and program units: shapes, runs and cells
inline int wplan_check_free_units(const WPlanRequest &rq, const WPlanCircuit &cv, WPlanState &s) {
    const char *fn = rq.fn;
    const size_t cells = cv.cells(), num_fcells = rq.num_cells;
    s.fcells32.resize(num_fcells); s.f_n[0].resize(rq.num_units); s.f_n[1].resize(rq.num_units);
    for (size_t i = 0; i < num_fcells; i++) s.fcells32[i] = rq.cells[i] < cells ? (u32)rq.cells[i] : NONE;      // outputs may be GLP_WGEN_NO_CELL; checked per run below
    for (u32 f = 0; f < rq.num_units; f++) {
        const glp_witness_free_unit &u = rq.units[f];
        u32 &ni = s.f_n[0][f], &no = s.f_n[1][f];
        if (rq.is_prog(f)) {
            WPLAN_REQUIRE(u.modulus < rq.num_programs, "%s: units[%u].modulus = %u, a program unit names its program there and num_programs = %u", fn, f, u.modulus, rq.num_programs);
            const glp_witness_program_desc &pd = rq.programs[u.modulus];
            WPLAN_REQUIRE(u.len[0] == pd.num_inputs, "%s: units[%u].len[0] = %u, programs[%u] has num_inputs = %u", fn, f, u.len[0], u.modulus, pd.num_inputs);
            WPLAN_REQUIRE(u.len[1] == pd.num_outputs, "%s: units[%u].len[1] = %u, programs[%u] has num_outputs = %u", fn, f, u.len[1], u.modulus, pd.num_outputs);
            for (u32 i = 2; i < 6; i++) WPLAN_REQUIRE(u.len[i] == 0, "%s: units[%u].len[%u] = %u, a program unit has two operands: unused entries are 0", fn, f, i, u.len[i]);
            ni = u.len[0]; no = u.len[1];
        } else {
            const WFreeShape sh = witness_free_shape(u.kind);
            WPLAN_REQUIRE(sh.operands, "%s: units[%u].kind = %u is not a GLP_WGEN_* kind", fn, f, u.kind);
            const bool has_modulus = u.kind >= GLP_WGEN_NONNATIVE_ADD && u.kind <= GLP_WGEN_NONNATIVE_INV;
            if (has_modulus) WPLAN_REQUIRE(u.modulus < rq.num_moduli, "%s: units[%u].modulus = %u, num_moduli = %u", fn, f, u.modulus, rq.num_moduli);
            else WPLAN_REQUIRE(u.modulus == 0, "%s: units[%u].modulus = %u, kind %u has no modulus: 0", fn, f, u.modulus, u.kind);
            for (u32 i = 0; i < 6; i++) {
                const u32 l = u.len[i];
                if (i >= sh.operands) { WPLAN_REQUIRE(l == 0, "%s: units[%u].len[%u] = %u, kind %u has %u operands: unused entries are 0", fn, f, i, l, u.kind, sh.operands); continue; }
                if (sh.single >> i & 1) { WPLAN_REQUIRE(l == 1, "%s: units[%u].len[%u] = %u, that operand of kind %u is 1 cell", fn, f, i, l, u.kind); continue; }
                if (u.kind == GLP_WGEN_NONNATIVE_MULTI_ADD && i == 0) continue;                                   // the number of summands
                if ((int)i == sh.divisor) WPLAN_REQUIRE(l <= 8, "%s: units[%u].len[%u] = %u, a divisor has at most 8 limbs", fn, f, i, l);
                WPLAN_REQUIRE(l <= GLP_WGEN_MAX_LIMBS, "%s: units[%u].len[%u] = %u, an operand has at most GLP_WGEN_MAX_LIMBS = %u limbs", fn, f, i, l, GLP_WGEN_MAX_LIMBS);
                if (u.kind == GLP_WGEN_GLV_SECP256K1) WPLAN_REQUIRE(l == (i ? 4u : 8u), "%s: units[%u].len[%u] = %u, GLV_SECP256K1 has k of 8 and k1, k2 of 4 limbs", fn, f, i, l);
            }
            ni = big::num_in(u.kind, u.len); no = big::num_out(u.kind, u.len);
        }
        WPLAN_REQUIRE((size_t)u.cell_begin + ni + no <= num_fcells, "%s: units[%u].cell_begin = %u: its run of %u cells leaves cells[] (num_cells = %zu)", fn, f,
                      u.cell_begin, ni + no, num_fcells);
        for (u32 i = 0; i < ni + no; i++) {
            const uint64_t cell = rq.cells[(size_t)u.cell_begin + i];
            WPLAN_REQUIRE(cell < cells || (i >= ni && cell == GLP_WGEN_NO_CELL), "%s: units[%u]: cells[%zu] = %llu is out of range (num_wires * 2^degree_bits = %zu cells)", fn, f,
                          (size_t)u.cell_begin + i, (unsigned long long)cell, cells);
        }
    }
    return GLP_OK;
}

// ---- 3. the units in (row, unit) order and the writer of every cell; a free unit may not write what another unit writes
inline int wplan_units(const WPlanRequest &rq, const WPlanCircuit &cv, WPlanState &s) {
    const char *fn = rq.fn;
    const size_t n = cv.n();
    std::vector<uint8_t> role(cv.nw);
    s.g[0].resize(cv.ng); s.g[1].resize(cv.ng);
    for (u32 gi = 0; gi < cv.ng; gi++) {
        const glp_gate &g = cv.gates[gi];
        const u32 nu = witness_gate_units(g.type, g.p0, g.p1);
        WPLAN_REQUIRE(nu <= 0xFFFF, "%s: gate %u has %u units per row, a plan names at most 65535", fn, gi, nu);
        s.g[0][gi].resize(nu); s.g[1][gi].resize(nu);
        for (u32 u = 0; u < nu; u++) {
            witness_unit_roles(g, cv.nw, u, role.data());
            for (u32 col = 0; col < cv.nw; col++) if (role[col]) s.g[role[col] == 1][gi][u].push_back(col);
        }
    }
    s.row_first.assign(n + 1, 0);
    for (size_t r = 0; r < n; r++) s.row_first[r + 1] = s.row_first[r] + (cv.row_gate[r] == NONE ? 0 : s.g[0][cv.row_gate[r]].size());
    const size_t nu_total = s.nu_total = s.row_first[n];
    s.nk = nu_total + rq.num_units;
    WPLAN_REQUIRE(s.nk < NONE, "%s: %zu units exceed the 2^32 - 1 a plan addresses", fn, s.nk);
    s.unit_row.resize(nu_total);
    for (size_t r = 0; r < n; r++) for (size_t k = s.row_first[r]; k < s.row_first[r + 1]; k++) s.unit_row[k] = (u32)r;
    std::vector<u32> &writer = s.writer;
    writer.assign(cv.cells(), NONE);
    for (size_t k = 0; k < nu_total; k++) wplan_cells(rq, cv, s, k, 1, [&](size_t q) { writer[q] = (u32)k; });
    for (u32 f = 0; f < rq.num_units; f++) {
        int rc = GLP_OK;
        wplan_cells(rq, cv, s, nu_total + f, 1, [&](size_t q) {
            if (rc != GLP_OK) return;
            const u32 wk = writer[q];
            if (wk == NONE) { writer[q] = (u32)(nu_total + f); return; }
            if (wk >= nu_total) rc = glp::set_error(GLP_ERR_ARG, "%s: units[%u]: output cell %zu is also written by units[%u]", fn, f, q, (u32)(wk - nu_total));
            else rc = glp::set_error(GLP_ERR_ARG, "%s: units[%u]: output cell %zu (column %zu, row %zu) is also written by unit %u of gate %u of that row", fn, f, q, q / n, q % n,
                                     (u32)(wk - s.row_first[s.unit_row[wk]]), cv.row_gate[s.unit_row[wk]]);
        });
        if (rc != GLP_OK) return rc;
    }
    return GLP_OK;
}

// ---- 4. the copy classes: the cycles of the decoded permutation, named by their smallest position; a non-routed cell is its own class
inline int wplan_classes(const WPlanRequest &rq, const WPlanCircuit &cv, WPlanState &s) {
    const size_t cells = cv.cells(), routed = (size_t)cv.nr << cv.lg;
    std::vector<u32> &cls = s.cls;
    cls.assign(cells, NONE);
    for (size_t p = 0; p < routed; p++) {                 // ascending: the first cell of a cycle met is its smallest
        if (cls[p] != NONE) continue;
        for (size_t q = p; cls[q] == NONE; q = cv.pos[q]) {
            cls[q] = (u32)p;
            WPLAN_REQUIRE(cv.pos[q] < routed, "%s: the decoded permutation leaves the routed columns", rq.fn);
        }
    }
    for (size_t p = routed; p < cells; p++) cls[p] = (u32)p;
    s.class_wave.assign(cells, -1);                       // two inputs in one class are refused; so are two random cells, and one of each
    std::vector<u32> class_input(rq.num_inputs + rq.num_random ? cells : 0, NONE);
    for (u32 i = 0; i < rq.num_inputs; i++) {
        u32 &first = class_input[cls[(size_t)rq.input_cells[i]]];
        WPLAN_REQUIRE(first == NONE, "%s: input_cells[%u] = %llu and input_cells[%u] = %llu lie in one copy class: one value per class", rq.fn, first,
                      (unsigned long long)rq.input_cells[first], i, (unsigned long long)rq.input_cells[i]);
        first = i;
        s.class_wave[cls[(size_t)rq.input_cells[i]]] = 0;
    }
    for (u32 i = 0; i < rq.num_random; i++) {
        const unsigned long long cell = rq.random_cells[i];
        u32 &first = class_input[cls[(size_t)cell]];
        if (first != NONE && first >= rq.num_inputs)
            return glp::set_error(GLP_ERR_ARG, "%s: random_cells[%u] = %llu and random_cells[%u] = %llu lie in one copy class: one value per class", rq.fn,
                                  first - rq.num_inputs, (unsigned long long)rq.random_cells[first - rq.num_inputs], i, cell);
        WPLAN_REQUIRE(first == NONE, "%s: random_cells[%u] = %llu and input_cells[%u] = %llu lie in one copy class: one value per class", rq.fn, i, cell, first,
                      (unsigned long long)rq.input_cells[first]);
        first = rq.num_inputs + i;
        s.class_wave[cls[(size_t)cell]] = 0;
    }
    return GLP_OK;
}

// ---- 5. the waves: a unit is ready once every class it reads is known; its wave is one more than the wave that made the last one known
inline int wplan_waves(const WPlanRequest &rq, const WPlanCircuit &cv, WPlanState &s) {
    const size_t cells = cv.cells(), nk = s.nk;
    const std::vector<u32> &cls = s.cls;
    std::vector<int32_t> &class_wave = s.class_wave;
    // per class the units that wait for it (one entry per cell read in a class not known from the inputs)
    std::vector<u32> pending(nk, 0);
    std::vector<size_t> reader_off(cells + 1, 0);
    for (size_t k = 0; k < nk; k++)
        wplan_cells(rq, cv, s, k, 0, [&](size_t q) { const u32 cl = cls[q]; if (class_wave[cl] < 0) { reader_off[cl + 1]++; pending[k]++; } });
    for (size_t p = 0; p < cells; p++) reader_off[p + 1] += reader_off[p];
    std::vector<u32> readers(reader_off[cells]);
    {
        std::vector<size_t> fill(reader_off.begin(), reader_off.end() - 1);
        for (size_t k = 0; k < nk; k++)
            wplan_cells(rq, cv, s, k, 0, [&](size_t q) { const u32 cl = cls[q]; if (class_wave[cl] < 0) readers[fill[cl]++] = (u32)k; });
    }
    s.unit_wave.assign(nk, -1);
    std::vector<u32> ready, next;
    for (size_t k = 0; k < nk; k++) if (pending[k] == 0) ready.push_back((u32)k);
    u32 &num_waves = s.lists.info.num_waves;
    uint64_t &widest = s.lists.info.widest_wave_units, &widest_free = s.lists.free_info.widest_wave_free_units;
    while (!ready.empty()) {
        num_waves++;
        uint64_t wave_free = 0;
        for (u32 k : ready) wave_free += k >= s.nu_total;
        widest = std::max<uint64_t>(widest, ready.size() - wave_free);
        widest_free = std::max<uint64_t>(widest_free, wave_free);
        next.clear();
        for (u32 k : ready) s.unit_wave[k] = (int32_t)num_waves;
        for (u32 k : ready)
            wplan_cells(rq, cv, s, k, 1, [&](size_t q) {
                const u32 cl = cls[q];
                if (class_wave[cl] >= 0) return;
                class_wave[cl] = (int32_t)num_waves;
                for (size_t i = reader_off[cl]; i < reader_off[cl + 1]; i++) if (--pending[readers[i]] == 0) next.push_back(readers[i]);
            });
        ready.swap(next);
    }
    return GLP_OK;
}

// ---- 6. the lists: what the plan keeps and uploads
inline int wplan_lists(const WPlanRequest &rq, const WPlanCircuit &cv, WPlanState &s) {
    const char *fn = rq.fn;
    const size_t cells = cv.cells(), nu_total = s.nu_total;
    const std::vector<int32_t> &unit_wave = s.unit_wave;
    WPlanLists &L = s.lists;
    struct glp_witness_plan_info &info = L.info;
    struct glp_witness_plan_free_info &finfo = L.free_info;
    const u32 nf = rq.num_units, num_waves = info.num_waves;
    info.num_units = nu_total; finfo.num_free_units = nf;
    auto gu = [&](size_t k) { return WUnit{s.unit_row[k], cv.row_gate[s.unit_row[k]] << 16 | (u32)(k - s.row_first[s.unit_row[k]])}; };
    // the stuck units, the first of each kind named; the units by wave in (row, unit) order
    for (size_t k = 0; k < nu_total; k++)
        if (unit_wave[k] <= 0 && !info.num_stuck_units++) { info.stuck_row = gu(k).row; info.stuck_gate = gu(k).gu >> 16; info.stuck_unit = gu(k).gu & 0xFFFF; }
    u32 nf_prog = 0;
    for (u32 f = 0; f < nf; f++) {
        nf_prog += rq.is_prog(f);
        if (unit_wave[nu_total + f] <= 0 && !finfo.num_stuck_free_units++) finfo.first_stuck_free_unit = f;
    }
    WPLAN_TRY(wplan_bucket(fn, "units", num_waves, [&](auto &&put) {
        for (size_t k = 0; k < nu_total; k++) if (unit_wave[k] > 0) put((u32)unit_wave[k], gu(k));
    }, L.unit_off, L.units));
    // the free units by wave, in the caller's order; program units are listed apart, below
    if (nf > nf_prog)
        WPLAN_TRY(wplan_bucket(fn, "free units", num_waves, [&](auto &&put) {
            for (u32 f = 0; f < nf; f++) if (!rq.is_prog(f) && unit_wave[nu_total + f] > 0) put((u32)unit_wave[nu_total + f], rq.units[f]);
        }, L.free_off, L.free_units));
    // the program units by wave, sorted by program (then in the caller's order), cut into chunks of at most 64 units of one program
    if (nf_prog) {
        std::vector<u32> order;
        for (u32 f = 0; f < nf; f++) if (rq.is_prog(f) && unit_wave[nu_total + f] > 0) order.push_back(f);
        std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) {
            const int32_t wx = unit_wave[nu_total + x], wy = unit_wave[nu_total + y];
            return wx != wy ? wx < wy : rq.units[x].modulus < rq.units[y].modulus;
        });
        WPLAN_TRY(wplan_bucket(fn, "program chunks", num_waves, [&](auto &&put) {
            for (size_t i = 0, j = 0; i < order.size(); i = j) {
                const u32 w = (u32)unit_wave[nu_total + order[i]], pr = rq.units[order[i]].modulus;
                while (j < order.size() && j - i < 64 && (u32)unit_wave[nu_total + order[j]] == w && rq.units[order[j]].modulus == pr) j++;
                put(w, WProgChunk{pr, (u32)i, (u32)(j - i)});
            }
        }, L.prog_chunk_off, L.prog_chunks));
        for (u32 f : order) L.prog_units.push_back(rq.units[f]);
        for (u32 i = 0; i < rq.num_programs; i++) {
            const glp_witness_program_desc &pd = rq.programs[i];
            const u32 words = (pd.num_instructions + 3) & ~3u;
            WProgEntry e;
            e.code_off = (u32)L.prog_image.size(); e.code_words = words; e.pool_off = e.code_off + words; e.num_inputs = pd.num_inputs;
            WPLAN_REQUIRE(L.prog_image.size() + words + pd.num_pool < NONE, "%s: the programs exceed the 2^32 - 1 words a plan addresses", fn);
            L.prog_image.insert(L.prog_image.end(), pd.code, pd.code + pd.num_instructions);
            L.prog_image.resize((size_t)e.code_off + words, 0);
            if (pd.num_pool) L.prog_image.insert(L.prog_image.end(), pd.pool, pd.pool + pd.num_pool);
            L.prog_tab.push_back(e);
            L.prog_lds = std::max<u32>(L.prog_lds, pd.num_regs * 64 * 8);
        }
    }
    // the wave of every known cell, the source of every known class, the copies by wave in order of the destination
    std::vector<u32> source(cells, NONE);        // by class name
    L.cell_waves.assign(cells, -1);
    for (size_t q = 0; q < cells; q++) {
        const u32 cl = s.cls[q];
        const int32_t cw = s.class_wave[cl];
        if (cw < 0) continue;
        const bool written = s.writer[q] != NONE && unit_wave[s.writer[q]] > 0;
        L.cell_waves[q] = written ? unit_wave[s.writer[q]] : cw;
        info.num_cells_known++;
        if (source[cl] == NONE && (cw == 0 ? s.input_at[q] != NONE : (written && unit_wave[s.writer[q]] == cw))) source[cl] = (u32)q;
    }
    WPLAN_TRY(wplan_bucket(fn, "copies", num_waves, [&](auto &&put) {
        for (size_t q = 0; q < cells; q++) if (s.class_wave[s.cls[q]] >= 0 && source[s.cls[q]] != q) put((u32)s.class_wave[s.cls[q]], WCopy{source[s.cls[q]], (u32)q});
    }, L.copy_off, L.copies));
    info.num_copies = L.copy_off[num_waves + 1];
    L.inputs.assign(rq.input_cells, rq.input_cells + rq.num_inputs);      // every one is below 2^32
    L.random.assign(rq.random_cells, rq.random_cells + rq.num_random);
    L.free_cells.swap(s.fcells32);
    return GLP_OK;
}
}  // namespace
