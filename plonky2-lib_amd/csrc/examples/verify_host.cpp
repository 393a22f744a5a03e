// verify_host.cpp -- the host half of the verifier as a stand-alone program: csrc/circuit_common.h (the rules a circuit description is
// held to, the verifier's view of a circuit), csrc/verify_host.h (glp_verify's body) and csrc/proof_bytes.h without a GPU, so that
// tests/test_verify_host.py can hold them to the CPU oracle and build them with the host sanitizers.  It makes no HIP runtime call; it
// is compiled by hipcc only because glf.h, poseidon.h and keccak.h carry the device attributes:
//
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wall -Wno-unused-function -Xarch_host -fsanitize=address,undefined \
//           -Xarch_host -fno-sanitize-recover=all -I.. verify_host.cpp -o verify_host
//
// stdin, numbers in decimal separated by white space:
//     degree_bits num_wires num_routed_wires num_constants num_selectors num_challenges quotient_degree_factor num_partial_products
//     num_gate_constraints rate_bits cap_height proof_of_work_bits num_query_rounds num_reductions
//     reduction_arity_bits[num_reductions]
//     num_public_inputs  hasher  flags  null_mask          null_mask bit 0..3: hand gates, k_is, constants, sigmas over as null pointers
//     num_gates  then per gate: type selector_index group_start group_end row num_constraints p0 p1
//     num_k_is  k_is[num_k_is]                             num_k_is = num_routed_wires, but for a description that is refused before they are read
//     circuit_digest[4]                                    all zero: the library's recipe over the cap
//     num_programs  then per program: num_regs num_params num_oracles oracle_cols[num_oracles] num_instructions code[] num_pool pool[]
//     cap_words  cap[cap_words]                            the constants/sigmas cap, 4 << cap_height words
//     num_bases  then per base proof: num_words words[]
//     num_members  then per member: base num_words num_edits (word value)[num_edits]
//                                                          the base proof with those words replaced, handed over as num_words words
//     num_byte_ops  then per operation: 0 base | 1 num_bytes hex        (hex: 2 num_bytes digits, "-" for none)
// The description takes no constants and no sigmas: a holder of the view never sees them, and their canonical-form scan is a step of its
// own (circuit_fields_check).  stdout: "digest d0 d1 d2 d3", "words n", "bytes n", then one line per member, "member i <status> <message>"
// (verify_impl_n; members run on a few threads, the lines come in order), then per byte operation "to_bytes <status> <hex>" or
// "from_bytes <status> <message> | words...".  A refused description prints "refused <code> <message>" instead and exits with
// status 3; unusable input exits with status 2.
#include <stdarg.h>
#include <stdio.h>
#include <atomic>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../verify_host.h"
#include "../proof_bytes.h"

static thread_local char g_error[1024];
int glp::set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

static bool rdu(unsigned long long *v) { return scanf("%llu", v) == 1; }
#define NEED(cond) do { if (!(cond)) { fprintf(stderr, "bad input: %s (line %d)\n", #cond, __LINE__); return 2; } } while (0)
#define U32(dst, bound) do { unsigned long long _v; NEED(rdu(&_v) && _v <= (bound)); (dst) = (u32)_v; } while (0)
static bool words(std::vector<uint64_t> &v, unsigned long long bound) {
    unsigned long long n, x;
    if (!rdu(&n) || n > bound) return false;
    v.resize((size_t)n);
    for (uint64_t &w : v) { if (!rdu(&x)) return false; w = x; }
    return true;
}

struct Member { u32 base; size_t num_words; std::vector<std::pair<size_t, uint64_t>> edits; int status = 0; std::string message; };

int main() {
    glp_circuit_desc d;
    memset(&d, 0, sizeof(d));
    u32 *scalars[14] = {&d.degree_bits, &d.num_wires, &d.num_routed_wires, &d.num_constants, &d.num_selectors, &d.num_challenges,
                        &d.quotient_degree_factor, &d.num_partial_products, &d.num_gate_constraints, &d.rate_bits, &d.cap_height,
                        &d.proof_of_work_bits, &d.num_query_rounds, &d.num_reductions};
    for (u32 *s : scalars) U32(*s, 0xFFFFFFFFull);
    NEED(d.num_reductions <= 64);
    for (u32 i = 0, ab; i < d.num_reductions; i++) { U32(ab, 0xFFFFFFFFull); if (i < 16) d.reduction_arity_bits[i] = ab; }     // more than 16 is refused; the array holds 16
    u32 flags, null_mask;
    U32(d.num_public_inputs, 1u << 20); U32(d.hasher, 0xFFFFFFFFull); U32(flags, 0xFFFFFFFFull); U32(null_mask, 15);
    U32(d.num_gates, 1u << 16);
    std::vector<glp_gate> gates(d.num_gates);
    for (glp_gate &g : gates) {
        u32 *f[8] = {&g.type, &g.selector_index, &g.group_start, &g.group_end, &g.row, &g.num_constraints, &g.p0, &g.p1};
        for (u32 *x : f) U32(*x, 0xFFFFFFFFull);
    }
    std::vector<uint64_t> k_is, cap;
    NEED(words(k_is, 1u << 24));
    for (uint64_t &w : d.circuit_digest) { unsigned long long x; NEED(rdu(&x)); w = x; }
    u32 num_programs;
    U32(num_programs, 1u << 12);
    std::vector<glp_gate_program_desc> programs(num_programs);
    std::vector<std::vector<uint64_t>> code(num_programs), pool(num_programs);
    std::vector<std::vector<u32>> ocols(num_programs);
    for (u32 p = 0; p < num_programs; p++) {
        glp_gate_program_desc &pd = programs[p];
        U32(pd.num_regs, 0xFFFFFFFFull); U32(pd.num_params, 0xFFFFFFFFull); U32(pd.num_oracles, 64);
        ocols[p].resize(pd.num_oracles);
        for (u32 &c : ocols[p]) U32(c, 0xFFFFFFFFull);
        NEED(words(code[p], 1u << 24) && words(pool[p], 1u << 24));
        pd.code = code[p].data(); pd.num_instructions = (u32)code[p].size();
        pd.pool = pool[p].empty() ? nullptr : pool[p].data(); pd.num_pool = (u32)pool[p].size();
        pd.oracle_cols = ocols[p].data();
    }
    NEED(words(cap, 1u << 24));
    static const uint64_t unread = 0;          // constants and sigmas: present, and never read here
    d.gates = null_mask & 1 ? nullptr : gates.data();
    d.k_is = null_mask & 2 ? nullptr : k_is.data();
    d.constants = null_mask & 4 ? nullptr : &unread;
    d.sigmas = null_mask & 8 ? nullptr : &unread;

    // the order of glp_circuit_create_prog: its own refusal of unknown flags, the rules, the canonical form of the field arrays
    int rc = (flags & ~GLP_CIRCUIT_ZERO_KNOWLEDGE) == 0 ? GLP_OK : glp::set_error(GLP_ERR_ARG, "unknown circuit flags 0x%x", flags);
    if (rc == GLP_OK) rc = circuit_desc_check(d, programs.empty() ? nullptr : programs.data(), num_programs);
    if (rc == GLP_OK) {
        NEED(k_is.size() == d.num_routed_wires && cap.size() == (size_t)4 << d.cap_height);
        rc = circuit_fields_check(d, false);
    }
    if (rc != GLP_OK) { printf("refused %d %s\n", rc, g_error); return 3; }
    CircuitCommon cc;
    circuit_common_describe(cc, d, flags, programs.data(), num_programs);
    circuit_common_commit(cc, cap);
    const size_t total = cc.L.total, nbytes = proof_bytes_len(cc);
    printf("digest %llu %llu %llu %llu\nwords %zu\nbytes %zu\n", (unsigned long long)cc.digest[0], (unsigned long long)cc.digest[1],
           (unsigned long long)cc.digest[2], (unsigned long long)cc.digest[3], total, nbytes);

    u32 num_bases, num_members, num_byte_ops;
    U32(num_bases, 64);
    std::vector<std::vector<uint64_t>> bases(num_bases);
    for (auto &b : bases) NEED(words(b, 1u << 26));
    U32(num_members, 1u << 20);
    std::vector<Member> members(num_members);
    for (Member &m : members) {
        unsigned long long n, e, at, value;
        U32(m.base, num_bases - 1);
        NEED(rdu(&n) && n <= (1u << 26) && rdu(&e) && e <= 64);
        m.num_words = (size_t)n;
        for (unsigned long long i = 0; i < e; i++) { NEED(rdu(&at) && at < n && rdu(&value)); m.edits.push_back({(size_t)at, value}); }
    }
    std::atomic<size_t> next(0);
    auto work = [&] {
        for (size_t i; (i = next++) < members.size();) {
            Member &m = members[i];
            const std::vector<uint64_t> &b = bases[m.base];
            std::unique_ptr<uint64_t[]> proof(new uint64_t[m.num_words]);     // exactly the words handed over: one word past them is the sanitizer's
            for (size_t j = 0; j < m.num_words; j++) proof[j] = j < b.size() ? b[j] : 0;
            for (const auto &ed : m.edits) proof[ed.first] = ed.second;
            g_error[0] = 0;
            m.status = verify_impl_n(cc, proof.get(), m.num_words);
            m.message = m.status == GLP_OK ? "" : g_error;
        }
    };
    std::vector<std::thread> pool_threads;
    for (unsigned t = 1; t < std::min(8u, std::max(1u, std::thread::hardware_concurrency())); t++) pool_threads.emplace_back(work);
    work();
    for (std::thread &t : pool_threads) t.join();
    for (size_t i = 0; i < members.size(); i++) printf("member %zu %d %s\n", i, members[i].status, members[i].message.c_str());

    U32(num_byte_ops, 1u << 16);
    for (u32 op = 0; op < num_byte_ops; op++) {
        u32 kind;
        U32(kind, 1);
        if (kind == 0) {
            u32 base;
            U32(base, num_bases - 1);
            NEED(bases[base].size() == total);
            std::vector<uint8_t> out(nbytes);
            rc = proof_to_bytes(cc, bases[base].data(), out.data(), out.size());
            printf("to_bytes %d ", rc);
            for (uint8_t b : out) printf("%02x", b);
            printf("\n");
        } else {
            unsigned long long n;
            NEED(rdu(&n) && n <= (1u << 28));
            std::unique_ptr<uint8_t[]> in(new uint8_t[(size_t)n]);      // exactly the bytes handed over
            std::vector<char> hex(2 * (size_t)n + 2);
            NEED(scanf(" %c", &hex[0]) == 1);
            if (n) {
                NEED(fread(&hex[1], 1, 2 * (size_t)n - 1, stdin) == 2 * (size_t)n - 1);
                for (size_t i = 0; i < n; i++) { unsigned v; NEED(sscanf(&hex[2 * i], "%2x", &v) == 1); in[i] = (uint8_t)v; }
            } else NEED(hex[0] == '-');
            std::vector<uint64_t> w(total, 0);
            g_error[0] = 0;
            rc = proof_from_bytes(cc, in.get(), (size_t)n, w.data());
            printf("from_bytes %d %s |", rc, rc == GLP_OK ? "" : g_error);
            if (rc == GLP_OK) for (uint64_t x : w) printf(" %llu", (unsigned long long)x);
            printf("\n");
        }
    }
    return 0;
}
