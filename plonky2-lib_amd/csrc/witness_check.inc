// witness_check.inc -- glp_witness_check: every gate constraint on the rows of H and every copy constraint of K witnesses of one circuit,
// with the first failure of each kind named (include/glp.h, "witness checker").  Included by prover.hip behind quotient_kernels.inc:
// the constraints are gate_terms' own bodies, consumed by a second sink.
//
//   k_witness_check_sigma   once per circuit (the first check; kept in glp_circuit::dev_sigma_pos), one lane per routed position:
//                           sigma(j, i) = k_j' w^i' decoded into the flat position j' n + i'
//   k_witness_check_gate    per gate of the table, one lane per row (rows of other gates leave at once), blockIdx.y = proof: gate_terms
//                           into WcSink; counts by wave and workgroup reduction, then one atomic per workgroup and counter; the first
//                           failure by a 64-bit atomicMin on row << 32 | constraint (the device of running_columns.inc).  Launched a
//                           second time with fetch = 1 and one wave per proof: lane 0 re-evaluates the row of the smallest key and
//                           stores that constraint's value
//   k_witness_check_copies  one lane per routed position and proof: the wire against the wire at the decoded position, key
//                           row << 32 | column; k_witness_check_copy_fetch names the other end and both values
// The values are read on H: N = n, slot = row, wires [num_wires][n], gate constants dev_consts + num_selectors n.
//
// Per proof k, res + k res_stride: the counters below, then rows_failed_by_gate[num_gates].
enum { WC_CONSTRAINTS, WC_ROWS, WC_KEY, WC_VALUE, WC_GATE, WC_COPIES, WC_COPY_KEY, WC_TO_POS, WC_COPY_VALUE, WC_TO_VALUE, WC_BY_GATE };
struct WcArgs {
    const u64 *wires;               // [K][num_wires][n]
    const u64 *consts;              // dev_consts [num_constants][n], selectors first
    const DevGate *gates;
    const u64 *pih;                 // [K][4] Poseidon hash of each proof's public inputs
    const u32 *pos;                 // [nr][n] decoded sigma: j' n + i'
    unsigned long long *res;
    u32 lg, nsel, num_gates, nw, nr, res_stride, fetch;
};
// The second sink of gate_terms (quotient_kernels.inc): constraint k's value, reduced (the bodies emit non-canonical words in places;
// a word equal to p is zero), is counted if it is not zero and the smallest such k kept; `want` is the constraint whose value the
// fetch launch is after (none: ~0).
struct WcSink {
    u32 nfail = 0, kmin = 0xFFFFFFFFu, want = 0xFFFFFFFFu;
    u64 val = 0;
    __device__ __forceinline__ void emit(u32 k, u64 v) {
        v = canon(v);
        if (v != 0) { nfail++; kmin = min(kmin, k); }
        if (k == want) val = v;
    }
};
// the gate of a row, as k_witness_fill and the planner read it (witness_plan.h)
__device__ __forceinline__ u32 wc_row_gate(const WcArgs &w, size_t n, size_t row) { return witness_row_gate(w.consts, w.nsel, n, row); }
// sums of cnt and rows and the minimum of key over the workgroup (blockDim.x = 256 = four waves); valid in thread 0
__device__ __forceinline__ void wc_block_reduce(u64 &cnt, u32 &rows, unsigned long long &key) {
    __shared__ u64 sh_cnt[4];
    __shared__ u32 sh_rows[4];
    __shared__ unsigned long long sh_key[4];
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_down((unsigned long long)cnt, o);
        rows += __shfl_down(rows, o);
        const unsigned long long other = __shfl_down(key, o);
        key = other < key ? other : key;
    }
    const u32 wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh_cnt[wave] = cnt; sh_rows[wave] = rows; sh_key[wave] = key; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (u32 v = 1; v < 4; v++) { cnt += sh_cnt[v]; rows += sh_rows[v]; key = sh_key[v] < key ? sh_key[v] : key; }
}
template <int TYPE>
__global__ __launch_bounds__(256) void k_witness_check_gate(WcArgs w, u32 gi) {
    const size_t n = (size_t)1 << w.lg, k = blockIdx.y;
    unsigned long long *res = w.res + k * w.res_stride;
    size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    WcSink sink;
    bool mine = row < n;
    if (w.fetch) {                                       // one wave per proof; lane 0 owns the row of the first failure
        const unsigned long long key = res[WC_KEY];
        mine = threadIdx.x == 0 && key != ~0ull;
        row = mine ? (size_t)(key >> 32) : 0;
        sink.want = (u32)key;
    }
    mine = mine && wc_row_gate(w, n, row) == gi;
    if (mine) {
        QArgs a = {};
        QProof p = {};
        a.cs = w.consts; a.gates = w.gates; a.nsel = w.nsel; a.num_gates = w.num_gates; a.lg = w.lg;
        p.wl = w.wires + k * (size_t)w.nw * n;
        _Pragma("unroll") for (int i = 0; i < 4; i++) p.pih[i] = w.pih[k * 4 + i];
        const DevGate g = w.gates[gi];
        gate_terms<1, TYPE, false>(a, p, g, n, row, 0, sink);
    }
    if (w.fetch) {
        if (mine) { res[WC_VALUE] = sink.val; res[WC_GATE] = gi; }
        return;
    }
    u64 cnt = sink.nfail;
    u32 rows = sink.nfail ? 1 : 0;
    unsigned long long key = sink.nfail ? ((unsigned long long)row << 32 | sink.kmin) : ~0ull;
    wc_block_reduce(cnt, rows, key);
    if (threadIdx.x == 0 && rows) {
        atomicAdd(res + WC_CONSTRAINTS, (unsigned long long)cnt);
        atomicAdd(res + WC_ROWS, (unsigned long long)rows);
        atomicAdd(res + WC_BY_GATE + gi, (unsigned long long)rows);
        atomicMin(res + WC_KEY, key);
    }
}

// Sigma decoding.  x = sigmas[j][i] lies on exactly one coset k_j' H (distinct cosets have distinct k_j'^n): t = x^n by lg squarings
// names j' in the host-made table kn[] = k_j^n; y = x k_j'^-1 is in H, and i' = log_w y comes bit by bit from the low end
// (Pohlig-Hellman over the 2-group): bit b of i' is set iff y^(2^(lg-1-b)) = -1, and then y <- y w^(-2^b).  About lg^2 / 2 squarings per
// position.  A value on no coset puts its flat index j n + i into *bad by atomicMin.
// tab: kn[nr], kinv[nr], winv[lg] (w_n^(-2^b))
__global__ __launch_bounds__(256) void k_witness_check_sigma(const u64 *sigmas, const u64 *tab, u32 *pos, unsigned long long *bad, u32 lg, u32 nr) {
    const size_t n = (size_t)1 << lg, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const u32 j = blockIdx.y;
    if (i >= n) return;
    const u64 x = sigmas[(size_t)j * n + i];
    u64 t = x;
    for (u32 s = 0; s < lg; s++) t = sqr(t);
    u32 jp = 0xFFFFFFFFu;
    for (u32 c = 0; c < nr; c++) if (tab[c] == t) jp = c;
    if (jp == 0xFFFFFFFFu) {
        atomicMin(bad, (unsigned long long)((size_t)j * n + i));
        pos[(size_t)j * n + i] = (u32)((size_t)j * n + i);
        return;
    }
    u64 y = mul(x, tab[nr + jp]);
    u32 ip = 0;
    for (u32 b = 0; b < lg; b++) {
        u64 z = y;
        for (u32 s = b + 1; s < lg; s++) z = sqr(z);
        if (z != 1) { ip |= 1u << b; y = mul(y, tab[2 * nr + b]); }
    }
    pos[(size_t)j * n + i] = (u32)((size_t)jp * n + ip);
}
__global__ __launch_bounds__(256) void k_witness_check_copies(WcArgs w) {
    const size_t n = (size_t)1 << w.lg, k = blockIdx.z, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const u32 j = blockIdx.y;
    unsigned long long *res = w.res + k * w.res_stride;
    const u64 *W = w.wires + k * (size_t)w.nw * n;
    bool fail = false;
    if (i < n) fail = canon(W[(size_t)j * n + i]) != canon(W[w.pos[(size_t)j * n + i]]);
    u64 cnt = fail ? 1 : 0;
    u32 rows = 0;
    unsigned long long key = fail ? ((unsigned long long)i << 32 | j) : ~0ull;
    wc_block_reduce(cnt, rows, key);
    if (threadIdx.x == 0 && cnt) {
        atomicAdd(res + WC_COPIES, (unsigned long long)cnt);
        atomicMin(res + WC_COPY_KEY, key);
    }
}
// one lane per proof: the other end of the first failing copy and both values
__global__ __launch_bounds__(64) void k_witness_check_copy_fetch(WcArgs w, u32 K) {
    const size_t n = (size_t)1 << w.lg, k = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    unsigned long long *res = w.res + k * w.res_stride;
    const unsigned long long key = res[WC_COPY_KEY];
    if (key == ~0ull) return;
    const u64 *W = w.wires + k * (size_t)w.nw * n;
    const size_t at = (size_t)(u32)key * n + (size_t)(key >> 32);
    const u32 to = w.pos[at];
    res[WC_TO_POS] = to;
    res[WC_COPY_VALUE] = canon(W[at]);
    res[WC_TO_VALUE] = canon(W[to]);
}

// a device witness is read where it lies if every word is canonical (the gate bodies take canonical wires), else from a reduced copy
__global__ __launch_bounds__(256) void k_witness_check_scan(const u64 *v, size_t count, u32 *flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) bad = bad || v[i] >= P;
    if (bad) *flag = 1;
}
__global__ __launch_bounds__(256) void k_witness_check_reduce(const u64 *v, u64 *out, size_t count) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) out[i] = canon(v[i]);
}

namespace {
template <int TYPE>
void wc_launch_type(glp_ctx *c, const WcArgs &w, u32 gi, u32 K) {
    const size_t n = (size_t)1 << w.lg;
    if (w.fetch) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_witness_check_gate<TYPE>), dim3(1, K), dim3(64), 0, c->stream, w, gi);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_witness_check_gate<TYPE>), dim3(nblk(n), K), dim3(256), 0, c->stream, w, gi);
}
// one gate body per launch, as the per-gate quotient kernels: the switch over the type is the host's
int wc_launch_gate(glp_ctx *c, const WcArgs &w, u32 type, u32 gi, u32 K) {
    switch (type) {
#define WC_CASE(T) case T: wc_launch_type<T>(c, w, gi, K); break;
    WC_CASE(GLP_GATE_CONSTANT) WC_CASE(GLP_GATE_PUBLIC_INPUT) WC_CASE(GLP_GATE_ARITHMETIC) WC_CASE(GLP_GATE_POSEIDON)
    WC_CASE(GLP_GATE_U32_INTERLEAVE) WC_CASE(GLP_GATE_UNINTERLEAVE_U32) WC_CASE(GLP_GATE_UNINTERLEAVE_B32) WC_CASE(GLP_GATE_U32_ARITHMETIC)
    WC_CASE(GLP_GATE_U32_ADD_MANY) WC_CASE(GLP_GATE_U32_SUBTRACTION) WC_CASE(GLP_GATE_U32_RANGE_CHECK) WC_CASE(GLP_GATE_COMPARISON)
    WC_CASE(GLP_GATE_BASE_SUM) WC_CASE(GLP_GATE_RANDOM_ACCESS) WC_CASE(GLP_GATE_ARITHMETIC_EXTENSION) WC_CASE(GLP_GATE_MUL_EXTENSION)
    WC_CASE(GLP_GATE_REDUCING) WC_CASE(GLP_GATE_REDUCING_EXTENSION) WC_CASE(GLP_GATE_EXPONENTIATION) WC_CASE(GLP_GATE_COSET_INTERPOLATION)
    WC_CASE(GLP_GATE_POSEIDON_MDS)
#undef WC_CASE
    default: return GLP_OK;         // NoopGate has no constraints
    }
    GLP_HIP(hipGetLastError());
    return GLP_OK;
}
// a gate of type GLP_GATE_PROGRAM: k_witness_check_program (circuit_program.inc)
int wc_launch_program(glp_ctx *c, const glp_circuit *cc, const WcArgs &w, u32 gi, u32 K);
}  // namespace

// The permutation decoded into flat positions, made by the first caller that needs it (glp_witness_check, glp_witness_plan_create:
// `fn` names it in a refusal) and kept with the circuit (DESIGN.md section 7: 8.6 of a check's 9.7 ms at 2^20 rows).  The ctx is bound.
int witness_sigma_decode(glp_ctx *c, const glp_circuit *cc, const char *fn) {
    if (cc->dev_sigma_pos) return GLP_OK;
    const u32 lg = cc->d.degree_bits, nr = cc->d.num_routed_wires;
    const size_t n = (size_t)1 << lg;
    Scratch tmp(c);
    std::vector<u64> tab(2 * (size_t)nr + lg);
    for (u32 j = 0; j < nr; j++) { tab[j] = pow(cc->k_is[j], (u64)n); tab[nr + j] = inv(cc->k_is[j]); }
    u64 wi = inv(root_of_unity((int)lg));
    for (u32 b = 0; b < lg; b++) { tab[2 * (size_t)nr + b] = wi; wi = mul(wi, wi); }
    u64 *dev_tab;
    u32 *pos = nullptr;
    unsigned long long *bad;
    GLP_TRY(tmp.words(&dev_tab, tab.size()));
    GLP_TRY(h2d(c, dev_tab, tab.data(), tab.size() * 8));
    GLP_TRY(tmp.array(&bad, 1));
    GLP_HIP(hipMemsetAsync(bad, 0xFF, 8, c->stream));
    GLP_TRY(c->alloc((void **)&pos, (size_t)nr * n * sizeof(u32)));
    unsigned long long first_bad = 0;
    int rc = GLP_OK;
    {
        StageScope st(c, "witness_check.sigma", 12.0 * nr * n);
        hipLaunchKernelGGL(k_witness_check_sigma, dim3(nblk(n), nr), dim3(256), 0, c->stream, cc->dev_sigmas, dev_tab, pos, bad, lg, nr);
        if (hipGetLastError() != hipSuccess) rc = set_error(GLP_ERR_HIP, "%s: the sigma decode could not be launched", fn);
    }
    if (rc == GLP_OK) rc = d2h(c, &first_bad, bad, 8);
    if (rc == GLP_OK && first_bad != ~0ull)
        rc = set_error(GLP_ERR_ARG, "%s: sigmas[%zu][%zu] is k_is[j'] * w_n^i' for no (j', i'): the circuit's permutation is malformed", fn,
                       (size_t)first_bad / n, (size_t)first_bad % n);
    if (rc != GLP_OK) {
        (void)hipStreamSynchronize(c->stream);
        c->release(pos);
        return rc;
    }
    cc->dev_sigma_pos = pos;
    return GLP_OK;
}

extern "C" {

int glp_witness_check(glp_ctx *c, const glp_circuit *cc, uint32_t num_proofs, const uint64_t *wires, int wires_on_device, const uint64_t *public_inputs,
                      glp_witness_report *reports_out, uint64_t *rows_failed_by_gate_out) {
    static const char *fn = "glp_witness_check";
    GLP_REQUIRE(c, "%s: ctx is null", fn);
    GLP_REQUIRE(cc, "%s: circuit is null", fn);
    GLP_REQUIRE(cc->ctx == c, "%s: circuit belongs to another ctx", fn);
    GLP_REQUIRE(wires, "%s: wires is null", fn);
    GLP_REQUIRE(reports_out, "%s: reports_out is null", fn);
    const glp_circuit_desc &d = cc->d;
    const u32 K = num_proofs, lg = d.degree_bits, nw = d.num_wires, nr = d.num_routed_wires, ng = d.num_gates, npi = d.num_public_inputs;
    GLP_TRY(seam_num_proofs_check(fn, K));
    GLP_REQUIRE(public_inputs || npi == 0, "%s: public_inputs is null, the circuit has num_public_inputs = %u", fn, npi);
    const size_t n = (size_t)1 << lg, per_proof = (size_t)nw * n;
    GLP_REQUIRE((size_t)nw * n <= ((size_t)1 << 32), "%s: num_wires * 2^degree_bits = %zu positions exceed the 2^32 a decoded sigma addresses", fn, per_proof);
    GLP_REQUIRE((size_t)K * nw <= BATCH_MAX_BYTES / (8 * n), "%s: wires too large (num_proofs * num_wires * 2^degree_bits words)", fn);
    if (!wires_on_device)
        for (u32 k = 0; k < K; k++) {
            const size_t bad = first_noncanonical(wires + k * per_proof, per_proof);
            GLP_REQUIRE(bad == per_proof, "%s: wires: proof %u, word %zu = 0x%016llx is not a canonical field element (>= p)", fn, k, bad,
                        (unsigned long long)wires[k * per_proof + (bad == per_proof ? 0 : bad)]);
        }
    for (u32 k = 0; k < K && npi; k++) {
        const size_t bad = first_noncanonical(public_inputs + (size_t)k * npi, npi);
        GLP_REQUIRE(bad == npi, "%s: public_inputs: proof %u, word %zu = 0x%016llx is not a canonical field element (>= p)", fn, k, bad,
                    (unsigned long long)public_inputs[(size_t)k * npi + (bad == npi ? 0 : bad)]);
    }
    GLP_TRY(bind(c));
    Scratch tmp(c);
    WcArgs w;
    memset(&w, 0, sizeof(w));
    w.consts = cc->dev_consts; w.gates = cc->dev_gates;
    w.lg = lg; w.nsel = d.num_selectors; w.num_gates = ng; w.nw = nw; w.nr = nr; w.res_stride = WC_BY_GATE + ng;

    GLP_TRY(witness_sigma_decode(c, cc, fn));
    w.pos = cc->dev_sigma_pos;

    GLP_TRY(tmp.input(wires, wires_on_device, (size_t)K * per_proof, &w.wires));
    if (wires_on_device) {
        u32 *flag, any = 0;
        GLP_TRY(tmp.array(&flag, 2));
        GLP_HIP(hipMemsetAsync(flag, 0, 4, c->stream));
        const unsigned blocks = (unsigned)std::min<size_t>(nblk((size_t)K * per_proof), (size_t)c->num_cus * 16);
        hipLaunchKernelGGL(k_witness_check_scan, dim3(blocks), dim3(256), 0, c->stream, wires, (size_t)K * per_proof, flag);
        GLP_HIP(hipGetLastError());
        GLP_TRY(d2h(c, &any, flag, 4));
        if (any) {
            u64 *red;
            GLP_TRY(tmp.words(&red, (size_t)K * per_proof));
            hipLaunchKernelGGL(k_witness_check_reduce, dim3(blocks), dim3(256), 0, c->stream, wires, red, (size_t)K * per_proof);
            GLP_HIP(hipGetLastError());
            w.wires = red;
        }
    }
    {
        std::vector<u64> pih((size_t)K * 4);
        for (u32 k = 0; k < K; k++) host_hash_no_pad(public_inputs + (size_t)k * npi, npi, pih.data() + 4 * (size_t)k);
        u64 *dev_pih;
        GLP_TRY(tmp.words(&dev_pih, pih.size()));
        GLP_TRY(h2d(c, dev_pih, pih.data(), pih.size() * 8));
        w.pih = dev_pih;
    }
    std::vector<unsigned long long> res((size_t)K * w.res_stride, 0);
    for (u32 k = 0; k < K; k++) res[(size_t)k * w.res_stride + WC_KEY] = res[(size_t)k * w.res_stride + WC_COPY_KEY] = ~0ull;
    GLP_TRY(tmp.array(&w.res, res.size()));
    GLP_TRY(h2d(c, w.res, res.data(), res.size() * 8));
    {
        StageScope st(c, "witness_check.gates", 8.0 * K * n * (nw + d.num_constants));
        for (u32 fetch = 0; fetch < 2; fetch++) {
            w.fetch = fetch;
            for (u32 gi = 0; gi < ng; gi++) {
                if (cc->gates[gi].type == GLP_GATE_PROGRAM) GLP_TRY(wc_launch_program(c, cc, w, gi, K));
                else GLP_TRY(wc_launch_gate(c, w, cc->gates[gi].type, gi, K));
            }
        }
    }
    {
        StageScope st(c, "witness_check.copies", K * n * nr * 20.0);
        hipLaunchKernelGGL(k_witness_check_copies, dim3(nblk(n), nr, K), dim3(256), 0, c->stream, w);      // K <= 4096 rides in grid.z
        hipLaunchKernelGGL(k_witness_check_copy_fetch, dim3((K + 63) / 64), dim3(64), 0, c->stream, w, K);
        GLP_HIP(hipGetLastError());
    }
    GLP_TRY(d2h(c, res.data(), w.res, res.size() * 8));
    for (u32 k = 0; k < K; k++) {
        const unsigned long long *r = res.data() + (size_t)k * w.res_stride;
        glp_witness_report &o = reports_out[k];
        memset(&o, 0, sizeof(o));
        o.failed_constraints = r[WC_CONSTRAINTS]; o.failed_rows = r[WC_ROWS]; o.failed_copies = r[WC_COPIES];
        if (o.failed_constraints) { o.row = r[WC_KEY] >> 32; o.constraint = (u32)r[WC_KEY]; o.gate = (u32)r[WC_GATE]; o.value = r[WC_VALUE]; }
        if (o.failed_copies) {
            o.copy_row = r[WC_COPY_KEY] >> 32; o.copy_col = (u32)r[WC_COPY_KEY];
            o.to_col = (u32)(r[WC_TO_POS] / n); o.to_row = r[WC_TO_POS] % n;
            o.copy_value = r[WC_COPY_VALUE]; o.to_value = r[WC_TO_VALUE];
        }
        if (rows_failed_by_gate_out) for (u32 gi = 0; gi < ng; gi++) rows_failed_by_gate_out[(size_t)k * ng + gi] = r[WC_BY_GATE + gi];
    }
    return GLP_OK;
}

}  // extern "C"
