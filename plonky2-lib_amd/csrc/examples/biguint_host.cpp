// biguint_host.cpp -- csrc/biguint_dev.h as a plain host program: the limb arithmetic of the free units of witness generation
// (include/glp.h, GLP_WGEN_*) without a GPU, so that tests/test_biguint_host.py can compare every kind with Python integers and build
// it with the host sanitizers.
//
// stdin, one unit per line, every number hexadecimal:
//     kind  nm  m[0] .. m[nm-1]  len[0] .. len[5]  in[0] .. in[num_in-1]
// (nm = 0 for the kinds without a modulus; inputs in the order of the unit's cell run, as 64-bit cell values: only the low 32 bits are
// read, as on the device).  stdout: the unit's output cells on one line; the last line is "stats <digit corrections> <add-backs>", how
// often the division took its two correction branches over the whole run.
//
// With --per-unit every output line starts with four fields: the instance that ran (`all8`: every count a compile-time 8, or `any`), and
// for this unit alone its digit corrections, its digits corrected twice and its add-backs; the last line then ends with the digits
// corrected twice over the whole run.  tests/test_biguint_device_vectors.py shows with them that the vectors the GPU gets reach the rare
// branches in both instances.
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I.. biguint_host.cpp -o biguint_host
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../biguint_dev.h"

int main(int argc, char **argv) {
    const bool per_unit = argc == 2 && !strcmp(argv[1], "--per-unit");
    if (argc > 1 && !per_unit) { fprintf(stderr, "usage: %s [--per-unit] < units\n", argv[0]); return 2; }
    big::Stats st = {0, 0, 0};
    unsigned kind, nm;
    while (scanf("%x %x", &kind, &nm) == 2) {
        if (nm > (unsigned)big::MAX_MOD) { fprintf(stderr, "modulus of %u limbs\n", nm); return 2; }
        uint32_t m[big::MAX_MOD] = {0};
        uint16_t len[6];
        for (unsigned i = 0; i < nm; i++) if (scanf("%x", &m[i]) != 1) return 2;
        for (int i = 0; i < 6; i++) { unsigned v; if (scanf("%x", &v) != 1) return 2; len[i] = (uint16_t)v; }
        const uint32_t ni = big::num_in(kind, len), no = big::num_out(kind, len);
        std::vector<unsigned long long> in(ni);
        std::vector<uint32_t> out(no, 0xDEADBEEFu);
        for (uint32_t i = 0; i < ni; i++) if (scanf("%llx", &in[i]) != 1) return 2;
        auto rd = [&](int i) { return (uint32_t)in.at((size_t)i); };
        auto wr = [&](int i, uint32_t v) { out.at((size_t)i) = v; };
        const big::Stats was = st;
        const bool all8 = big::all8(kind, len, (int)nm);
        if (all8) big::run_unit<true>(kind, len, m, 8, rd, wr, &st);          // the instance the device runs for the secp256k1 gadgets
        else big::run_unit<false>(kind, len, m, (int)nm, rd, wr, &st);
        if (per_unit)
            printf("%s %llu %llu %llu%s", all8 ? "all8" : "any", (unsigned long long)(st.qhat_corrections - was.qhat_corrections),
                   (unsigned long long)(st.twice - was.twice), (unsigned long long)(st.add_backs - was.add_backs), no ? " " : "");
        for (uint32_t i = 0; i < no; i++) printf("%x%c", out[i], i + 1 < no ? ' ' : '\n');
        if (!no) printf("\n");
    }
    printf("stats %llu %llu", (unsigned long long)st.qhat_corrections, (unsigned long long)st.add_backs);
    if (per_unit) printf(" %llu", (unsigned long long)st.twice);
    printf("\n");
    return 0;
}
