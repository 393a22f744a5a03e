// witness_plan_host.cpp -- csrc/witness_plan.h as a plain host program: the planner of witness generation (include/glp.h, "witness
// generation, the dataflow half") without a GPU, so that tests/test_witness_plan_host.py can compare every list of a plan with
// tests/witness_plan_restate.py and build it with the host sanitizers.  What the library's driver reads back from the device -- the
// gate of every row and the decoded permutation -- is part of the request here.
//
// stdin, numbers in decimal separated by white space:
//     lg  num_wires  num_routed  num_gates
//     type p0 p1                                  per gate
//     row_gate[2^lg]                              -1: a row of no gate
//     pos[num_routed * 2^lg]                      the decoded permutation, flat positions col * 2^lg + row
//     null_mask                                   bit 0..4: hand input_cells, units, cells, moduli, programs over as null pointers; bit 5: random_cells
//     num_inputs  input_cells[num_inputs]
//     num_units   then per unit: kind modulus cell_begin len[0..5]
//     num_cells  given  cells[given]              given = num_cells, but for the refusal of a num_cells no machine holds
//     num_moduli  then per modulus 8 limbs
//     with_programs  num_programs  then per program: num_inputs num_outputs num_regs num_instructions num_pool
//     num_random  random_cells[num_random]        optional: input that ends after the programs has no random cells
// (a program's code and pool are not part of the request: word i of program p's code is p << 32 | i, of its pool 1 << 63 | p << 32 | i.)
// The stages run in the library's order.  stdout: one line per figure or list, its name first -- info (num_waves num_units
// num_stuck_units num_copies num_cells_known widest_wave_units stuck_row stuck_gate stuck_unit), free_info (num_free_units
// num_stuck_free_units first_stuck_free_unit widest_wave_free_units), prog_lds, cell_waves, unit_off, units (row gu ...), copy_off, copies
// (src dst ...), inputs, random, free_off, free_units (kind modulus cell_begin len[0..5] ...), free_cells, prog_chunk_off, prog_chunks (prog
// first count ...), prog_units, prog_tab (code_off code_words pool_off num_inputs ...), prog_image.  A refusal prints
// "refused <code> <message>" instead and exits with status 3; unusable input exits with status 2.
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined witness_plan_host.cpp -o witness_plan_host
#include <stdarg.h>
#include <stdio.h>
#include <vector>

#include "../witness_plan.h"

static char g_error[1024];
int glp::set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

static bool rd(long long *v) { return scanf("%lld", v) == 1; }
static bool rdu(unsigned long long *v) { return scanf("%llu", v) == 1; }
#define NEED(cond) do { if (!(cond)) { fprintf(stderr, "bad input: %s (line %d)\n", #cond, __LINE__); return 2; } } while (0)

template <class T, class F> static void line(const char *name, const std::vector<T> &v, F &&each) {
    printf("%s", name);
    for (const T &x : v) each(x);
    printf("\n");
}
static void words(const char *name, const std::vector<u32> &v) { line(name, v, [](u32 x) { printf(" %u", x); }); }
static void free_units(const char *name, const std::vector<WFree> &v) {
    line(name, v, [](const WFree &u) { printf(" %u %u %u", u.kind, u.modulus, u.cell_begin); for (int i = 0; i < 6; i++) printf(" %u", u.len[i]); });
}

int main() {
    long long a, b, c, e, f;
    NEED(rd(&a) && rd(&b) && rd(&c) && rd(&e));
    NEED(a >= 0 && a <= 24 && b >= 1 && b <= (1 << 24) && c >= 0 && c <= b && e >= 0 && e <= (1 << 20));
    const u32 lg = (u32)a, nw = (u32)b, nr = (u32)c, ng = (u32)e;
    const size_t n = (size_t)1 << lg;
    std::vector<glp_gate> gates(ng);
    for (glp_gate &g : gates) {
        NEED(rd(&a) && rd(&b) && rd(&c));
        memset(&g, 0, sizeof(g));
        g.type = (u32)a; g.p0 = (u32)b; g.p1 = (u32)c;
    }
    std::vector<u32> row_gate(n), pos((size_t)nr * n);
    for (u32 &g : row_gate) { NEED(rd(&a)); g = a >= 0 && a < (long long)ng ? (u32)a : NONE; }      // as the library's driver: a gate of the table or none
    for (u32 &p : pos) { NEED(rd(&a) && a >= 0 && a <= 0xFFFFFFFFll); p = (u32)a; }
    long long null_mask;
    NEED(rd(&null_mask));
    NEED(rd(&a) && a >= 0 && a <= (1 << 28));
    std::vector<uint64_t> input_cells((size_t)a);
    for (uint64_t &v : input_cells) { unsigned long long x; NEED(rdu(&x)); v = x; }
    NEED(rd(&a) && a >= 0 && a <= (1 << 28));
    std::vector<glp_witness_free_unit> units((size_t)a);
    for (glp_witness_free_unit &u : units) {
        NEED(rd(&a) && rd(&b) && rd(&c) && a >= 0 && b >= 0 && c >= 0);
        u.kind = (u32)a; u.modulus = (u32)b; u.cell_begin = (u32)c;
        for (int i = 0; i < 6; i++) { NEED(rd(&a) && a >= 0 && a <= 0xFFFF); u.len[i] = (uint16_t)a; }
    }
    unsigned long long num_cells;
    NEED(rdu(&num_cells) && rd(&a) && a >= 0 && a <= (1 << 28));
    std::vector<uint64_t> cells((size_t)a);
    for (uint64_t &v : cells) { unsigned long long x; NEED(rdu(&x)); v = x; }
    NEED(num_cells == cells.size() || num_cells >= NONE);       // a count beyond the cells given only where the planner refuses it unread
    NEED(rd(&a) && a >= 0 && a <= (1 << 20));
    std::vector<u32> moduli((size_t)a * 8);
    for (u32 &v : moduli) { NEED(rd(&a) && a >= 0 && a <= 0xFFFFFFFFll); v = (u32)a; }
    long long with_programs;
    NEED(rd(&with_programs) && rd(&a) && a >= 0 && a <= (1 << 16));
    std::vector<glp_witness_program_desc> programs((size_t)a);
    std::vector<std::vector<uint64_t>> code(programs.size()), pool(programs.size());
    for (size_t p = 0; p < programs.size(); p++) {
        NEED(rd(&a) && rd(&b) && rd(&c) && rd(&e) && rd(&f));
        NEED(a >= 0 && b >= 0 && c >= 0 && e >= 0 && e <= (1 << 20) && f >= 0 && f <= (1 << 24));
        for (long long i = 0; i < e; i++) code[p].push_back((uint64_t)p << 32 | (uint64_t)i);
        for (long long i = 0; i < f; i++) pool[p].push_back(1ull << 63 | (uint64_t)p << 32 | (uint64_t)i);
        glp_witness_program_desc &d = programs[p];
        d.code = code[p].data(); d.num_instructions = (u32)e; d.pool = pool[p].data(); d.num_pool = (u32)f;
        d.num_regs = (u32)c; d.num_inputs = (u32)a; d.num_outputs = (u32)b;
    }
    std::vector<uint64_t> random_cells;
    if (rd(&a)) {                                                // the optional last line
        NEED(a >= 0 && a <= (1 << 28));
        random_cells.resize((size_t)a);
        for (uint64_t &v : random_cells) { unsigned long long x; NEED(rdu(&x)); v = x; }
    }
    auto ptr = [&](int bit, auto &v) { return null_mask >> bit & 1 ? nullptr : v.data(); };
    const WPlanRequest rq = {"witness_plan_host", ptr(0, input_cells), (u32)input_cells.size(), ptr(5, random_cells), (u32)random_cells.size(),
                             ptr(1, units), (u32)units.size(), ptr(2, cells),
                             (size_t)num_cells, ptr(3, moduli), (u32)(moduli.size() / 8), ptr(4, programs), (u32)programs.size(), with_programs != 0};
    const WPlanCircuit cv = {lg, nw, nr, ng, gates.data(), row_gate.data(), pos.data()};
    WPlanState s;
    int rc = wplan_check_pointers(rq);
    if (rc == GLP_OK) rc = wplan_check_request(rq, cv, s);
    if (rc == GLP_OK) rc = wplan_check_free_units(rq, cv, s);
    if (rc == GLP_OK) rc = wplan_units(rq, cv, s);
    if (rc == GLP_OK) rc = wplan_classes(rq, cv, s);
    if (rc == GLP_OK) rc = wplan_waves(rq, cv, s);
    if (rc == GLP_OK) rc = wplan_lists(rq, cv, s);
    if (rc != GLP_OK) { printf("refused %d %s\n", rc, g_error); return 3; }
    const WPlanLists &L = s.lists;
    const struct glp_witness_plan_info &in = L.info;
    printf("info %u %llu %llu %llu %llu %llu %llu %u %u\n", in.num_waves, (unsigned long long)in.num_units, (unsigned long long)in.num_stuck_units,
           (unsigned long long)in.num_copies, (unsigned long long)in.num_cells_known, (unsigned long long)in.widest_wave_units,
           (unsigned long long)in.stuck_row, in.stuck_gate, in.stuck_unit);
    const struct glp_witness_plan_free_info &fi = L.free_info;
    printf("free_info %llu %llu %llu %llu\n", (unsigned long long)fi.num_free_units, (unsigned long long)fi.num_stuck_free_units,
           (unsigned long long)fi.first_stuck_free_unit, (unsigned long long)fi.widest_wave_free_units);
    printf("prog_lds %u\n", L.prog_lds);
    line("cell_waves", L.cell_waves, [](int32_t x) { printf(" %d", x); });
    words("unit_off", L.unit_off);
    line("units", L.units, [](const WUnit &u) { printf(" %u %u", u.row, u.gu); });
    words("copy_off", L.copy_off);
    line("copies", L.copies, [](const WCopy &x) { printf(" %u %u", x.src, x.dst); });
    words("inputs", L.inputs);
    words("random", L.random);
    words("free_off", L.free_off);
    free_units("free_units", L.free_units);
    words("free_cells", L.free_cells);
    words("prog_chunk_off", L.prog_chunk_off);
    line("prog_chunks", L.prog_chunks, [](const WProgChunk &x) { printf(" %u %u %u", x.prog, x.first, x.count); });
    free_units("prog_units", L.prog_units);
    line("prog_tab", L.prog_tab, [](const WProgEntry &x) { printf(" %u %u %u %u", x.code_off, x.code_words, x.pool_off, x.num_inputs); });
    line("prog_image", L.prog_image, [](u64 x) { printf(" %llu", (unsigned long long)x); });
    return 0;
}
