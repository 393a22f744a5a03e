// circuit_create.inc -- the circuit handle: validation of a description against gate_shapes.h, the quotient launch plan, the uploads
// and the constants/sigmas commitment.  Included by prover.hip after the session.

// Quotient launch plan: the base-4 limb gates (at most LIMB_SLOTS of them) share k_quotient_limbs, the HBM-bound light
// gates share k_quotient_light, every other gate type keeps its own launch.  Builds the column program of
// k_quotient_limbs (format: see the kernel).
static int build_quotient_plan(glp_ctx *c, glp_circuit *cc) {
    const glp_circuit_desc &d = cc->d;
    std::vector<u64> desc((size_t)LIMB_GROUPS * d.num_wires * LIMB_SLOTS, 0);
    for (int g = 0; g < LIMB_GROUPS; g++) { cc->limb_jlo[g] = d.num_wires; cc->limb_jhi[g] = 0; }
    auto put = [&](u32 s, u32 col, u32 pos, u32 kl, bool flush, u32 kf, u32 ref) {       // s = slot over all groups
        const u32 grp = s / LIMB_SLOTS, slot = s % LIMB_SLOTS;
        desc[((size_t)grp * d.num_wires + col) * LIMB_SLOTS + slot] = 1ull | ((u64)pos << 1) | (flush ? 32ull : 0ull) | ((u64)kl << 6) | ((u64)kf << 16) | ((u64)ref << 26);
        cc->limb_jlo[grp] = std::min(cc->limb_jlo[grp], col); cc->limb_jhi[grp] = std::max(cc->limb_jhi[grp], col);
    };
    std::vector<GateShape> shape(d.num_gates);     // glp_circuit_create_ex has accepted every gate: gate_shape succeeds
    for (u32 gi = 0; gi < d.num_gates; gi++) gate_shape(cc->gates[gi], shape[gi]);
    std::vector<u32> limb_list;
    auto fill = [&](u32 s, u32 gi) {               // column program of gate gi in slot s (= 4 group + slot)
        const LimbBlock &b = shape[gi].limb;
        cc->limb_gi[s] = gi;
        for (u32 i = 0; i < b.ops; i++)
            for (u32 j = 0; j < b.limbs; j++)
                put(s, b.first + b.limbs * i + j, j & 15, b.kstride * i + b.klimb + (b.descending ? b.limbs - 1 - j : j), (j & 15) == 15 || j + 1 == b.limbs,
                    b.kstride * i + b.ksum + (j >> 4), b.ref_stride * i + b.ref0 + (j >> 4));
    };
    auto limb_start = [&](u32 gi) -> u32 { return shape[gi].limb.first; };
    auto limb_weight = [&](u32 gi) -> u32 { return shape[gi].limb.limbs * shape[gi].limb.ops; };      // limb columns of the gate = its share of the per-point work
    for (u32 gi = 0; gi < d.num_gates; gi++) {
        const glp_gate &g = cc->gates[gi];
        if (g.type == GLP_GATE_PROGRAM) { cc->program_gates.push_back(gi); continue; }      // k_quotient_gate_program, for every challenge count
        const bool limb_gate = shape[gi].launch == GATE_LAUNCH_LIMB, light = shape[gi].launch == GATE_LAUNCH_LIGHT;
        // alpha indices and wire columns must fit the descriptor fields (10 and 8 bits); glp_circuit_create has already
        // bounded num_constraints by ACC3_MAX_TERMS = 512
        if (limb_gate && limb_list.size() < (size_t)(LIMB_SLOTS * LIMB_GROUPS) && d.num_wires <= 256) {
            limb_list.push_back(gi);                       // slots are assigned below, once all limb gates are known
        } else if (g.type == GLP_GATE_ARITHMETIC && cc->arith_ops == 0 && 4 * g.p0 <= d.num_routed_wires && d.quotient_degree_factor % 4 == 0 &&
                   d.num_selectors + 2 <= d.num_constants) {
            cc->arith_gi = gi; cc->arith_ops = g.p0;      // evaluated inside the permutation loop of k_quotient
        } else if (light && cc->light_count < 8) {
            cc->light_gi[cc->light_count++] = gi;
        } else if (g.type != GLP_GATE_NOOP) {
            cc->single_gates.push_back(gi);
        }
    }
    if (limb_list.size() == 1) {               // nothing to share: the gate's own kernel is the better launch
        cc->single_gates.push_back(limb_list[0]);
        limb_list.clear();
    }
    if (!limb_list.empty()) {
        // Up to LIMB_SLOTS gates share a set of accumulators (one group); more gates go through the same launch group after group.  Every
        // group computes the range products of its own column range, so gates are grouped by where their limb columns START: the
        // union ranges of the groups then overlap least (secp256k1 circuit: [8,136) + [40,136) = 224 columns instead of 2 x 128).
        const u32 cnt = (u32)limb_list.size();
        const u32 G = (cnt + LIMB_SLOTS - 1) / LIMB_SLOTS;
        u32 used[LIMB_GROUPS] = {0, 0, 0, 0};
        std::stable_sort(limb_list.begin(), limb_list.end(), [&](u32 x, u32 y) {
            return limb_start(x) != limb_start(y) ? limb_start(x) < limb_start(y) : limb_weight(x) > limb_weight(y); });
        for (u32 t = 0; t < cnt; t++) {
            const u32 grp = t / LIMB_SLOTS;
            fill(grp * LIMB_SLOTS + used[grp], limb_list[t]);
            used[grp]++;
        }
        cc->limb_count = cnt; cc->limb_groups = G;
        for (u32 g = 0; g < G; g++) cc->limb_gcount[g] = used[g];
    }
    if (cc->limb_count) {                      // ComparisonGate (HBM-bound) rides with the VALU-bound limb launch
        std::vector<u32> keep;
        for (u32 gi : cc->single_gates) {
            if (cc->gates[gi].type == GLP_GATE_COMPARISON && cc->limb_extra_count < 4) cc->limb_extra_gi[cc->limb_extra_count++] = gi;
            else keep.push_back(gi);
        }
        cc->single_gates.swap(keep);
    }
    if (cc->limb_count) {
        GLP_TRY(c->alloc((void **)&cc->dev_limb_desc, desc.size() * 8));
        GLP_TRY(h2d(c, cc->dev_limb_desc, desc.data(), desc.size() * 8));
    }
    return GLP_OK;
}

// the in-circuit rules of a gate program (circuit_program.inc)
namespace { int circuit_program_check(const char *fn, const glp_gate_program_desc *d, CPInfo &info); }

extern "C" {

void glp_circuit_free(glp_circuit *cc) {
    if (!cc) return;
    glp_ctx *c = cc->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    batch_destroy(cc->cs);
    c->release(cc->dev_sigmas);
    c->release(cc->dev_k_is);
    c->release(cc->dev_gates);
    c->release(cc->dev_limb_desc);
    c->release(cc->dev_consts);
    c->release(cc->dev_sigma_pos);
    c->release(cc->dev_programs);
    delete cc;
}

int glp_circuit_create(glp_ctx *c, const glp_circuit_desc *desc, glp_circuit **out) { return glp_circuit_create_ex(c, desc, 0, out); }

int glp_circuit_create_ex(glp_ctx *c, const glp_circuit_desc *desc, uint32_t flags, glp_circuit **out) {
    return glp_circuit_create_prog(c, desc, flags, nullptr, 0, out);
}

// num_programs = 0 is glp_circuit_create_ex: no gate can name a program, and type 23 is a type this call does not know
int glp_circuit_create_prog(glp_ctx *c, const glp_circuit_desc *desc, uint32_t flags, const glp_gate_program_desc *programs, uint32_t num_programs,
                            glp_circuit **out) {
    GLP_REQUIRE(c && desc && out, "null argument");
    *out = nullptr;
    GLP_REQUIRE(programs || num_programs == 0, "glp_circuit_create_prog: programs is null with num_programs = %u", num_programs);
    GLP_REQUIRE((flags & ~GLP_CIRCUIT_ZERO_KNOWLEDGE) == 0, "unknown circuit flags 0x%x", flags);
    GLP_TRY(bind(c));
    const glp_circuit_desc &d = *desc;
    GLP_REQUIRE(d.gates && d.k_is && d.constants && d.sigmas, "null array in circuit description");
    GLP_REQUIRE(d.num_challenges >= 1 && d.num_challenges <= (u32)MAXCH, "num_challenges=%u outside 1..%d", d.num_challenges, MAXCH);
    if (d.hasher != GLP_HASH_POSEIDON && d.hasher != GLP_HASH_KECCAK25) return set_error(GLP_ERR_UNSUPPORTED, "hasher %u is not one of GLP_HASH_*", d.hasher);
    GLP_REQUIRE(d.rate_bits >= 1 && d.rate_bits <= 4, "rate_bits=%u outside 1..4", d.rate_bits);
    GLP_REQUIRE(d.num_routed_wires <= d.num_wires && d.num_routed_wires > 0, "bad wire counts");
    if ((int)d.degree_bits > NTT_MAX_LG) return set_error(GLP_ERR_UNSUPPORTED, "degree_bits=%u > %d", d.degree_bits, NTT_MAX_LG);
    const u32 qdf = d.quotient_degree_factor;
    if (qdf == 0 || (qdf & (qdf - 1)) || qdf > (1u << d.rate_bits))
        return set_error(GLP_ERR_UNSUPPORTED, "quotient_degree_factor=%u must be a power of two <= 2^rate_bits", qdf);
    GLP_REQUIRE(d.num_partial_products == (d.num_routed_wires + qdf - 1) / qdf - 1, "num_partial_products inconsistent");
    GLP_REQUIRE(d.num_reductions <= 16 && d.cap_height <= d.degree_bits + d.rate_bits, "bad FRI parameters");
    GLP_REQUIRE(d.proof_of_work_bits <= POW_MAX_BITS, "proof_of_work_bits=%u: this build searches at most 2^40 candidates and accepts up to %u bits",
                d.proof_of_work_bits, POW_MAX_BITS);
    u32 sum_ab = 0;
    for (u32 i = 0; i < d.num_reductions; i++) {
        GLP_REQUIRE(d.reduction_arity_bits[i] >= 1 && d.reduction_arity_bits[i] <= 5, "arity_bits outside 1..5");
        sum_ab += d.reduction_arity_bits[i];
        GLP_REQUIRE(sum_ab <= d.degree_bits && d.degree_bits + d.rate_bits - sum_ab >= d.cap_height, "FRI reduction deeper than the domain");
    }
    // Shapes the quotient kernel assumes (gate_shapes.h), checked here so that a malformed description is an error and never an
    // out-of-bounds read on the device: wires / constants / constraints each gate type touches.
    std::vector<CPInfo> pinfo(num_programs);
    for (u32 i = 0; i < num_programs; i++) {
        char who[64];
        snprintf(who, sizeof(who), "glp_circuit_create_prog: programs[%u]", i);
        GLP_TRY(circuit_program_check(who, programs + i, pinfo[i]));
    }
    u32 maxc = 0;
    for (u32 i = 0; i < d.num_gates; i++) {
        const glp_gate &g = d.gates[i];
        GateShape s;
        if (g.type == GLP_GATE_PROGRAM && num_programs) {
            // the shape of a program gate is what its program reads and emits; held to the degree rule of the recursion gates below
            GLP_REQUIRE(g.p0 < num_programs, "gate %u (type %u), field p0: program %u, the circuit has num_programs = %u", i, g.type, g.p0, num_programs);
            GLP_REQUIRE(g.p1 == 0, "gate %u (type %u), field p1: %u, must be 0", i, g.type, g.p1);
            const CPInfo &pi = pinfo[g.p0];
            s = GateShape();
            s.wires = pi.wires; s.constraints = pi.emits; s.degree = pi.degree;
            GLP_REQUIRE(s.constraints == g.num_constraints, "gate %u (type %u), field num_constraints: %u, program %u has %u EMITs", i, g.type,
                        g.num_constraints, g.p0, s.constraints);
            GLP_REQUIRE(s.wires <= d.num_wires, "gate %u (type %u), field p0: program %u reads wire %u, the circuit has num_wires = %u", i, g.type, g.p0,
                        s.wires - 1, d.num_wires);
            GLP_REQUIRE(pi.consts <= d.num_constants, "gate %u (type %u), field p0: program %u reads constant polynomial %u, the circuit has num_constants = %u",
                        i, g.type, g.p0, pi.consts - 1, d.num_constants);
        } else if (!gate_type_known(g.type) || !gate_shape(g, s))
            return set_error(gate_type_known(g.type) ? GLP_ERR_ARG : GLP_ERR_UNSUPPORTED,
                             "gate %u: type %u with parameters (%u, %u) is not supported", i, g.type, g.p0, g.p1);
        GLP_REQUIRE(s.wires <= d.num_wires, "gate %u (type %u) needs %u wires, circuit has %u", i, g.type, s.wires, d.num_wires);
        GLP_REQUIRE(d.num_selectors + s.consts <= d.num_constants, "gate %u (type %u) needs %u constants", i, g.type, s.consts);
        GLP_REQUIRE(s.constraints == g.num_constraints, "gate %u (type %u): num_constraints %u, expected %u", i, g.type, g.num_constraints, s.constraints);
        GLP_REQUIRE(s.routed <= d.num_routed_wires, "gate %u (type %u): %u routed inputs, circuit has %u routed wires", i, g.type, s.routed,
                    d.num_routed_wires);
        if (s.degree || g.type == GLP_GATE_PROGRAM) {
            // The quotient is evaluated on quotient_degree_factor cosets, so filter x constraint may have degree quotient_degree_factor + 1
            // at most (what plonky2's selector grouping guarantees for every gate it places): the filter has one factor per other gate of
            // the group, and the UNUSED factor when there are several selectors.
            const u32 filt = g.group_end - g.group_start - 1 + (d.num_selectors > 1 ? 1 : 0);
            GLP_REQUIRE(g.group_start < g.group_end && s.degree + filt <= qdf + 1, "gate %u (type %u): degree %u with a selector filter of degree %u exceeds "
                        "quotient_degree_factor %u + 1", i, g.type, s.degree, g.group_start < g.group_end ? filt : 0, qdf);
        }
        GLP_REQUIRE(g.selector_index < d.num_selectors && g.group_start <= g.row && g.row < g.group_end, "bad selector data for gate %u", i);
        GLP_REQUIRE(g.type == GLP_GATE_PROGRAM || g.num_constraints <= ACC3_MAX_TERMS, "gate %u: %u constraints exceed the %u the quotient accumulators hold", i,
                    g.num_constraints, ACC3_MAX_TERMS);      // a program gate: GLP_GATE_PROGRAM_MAX_CONSTRAINTS, held by circuit_program_check
        maxc = std::max(maxc, g.num_constraints);
    }
    GLP_REQUIRE(maxc <= d.num_gate_constraints, "num_gate_constraints smaller than a gate's constraint count");
    {   // field arrays from outside: canonical or rejected by name (one host pass, small against the uploads and the commitment below)
        const size_t nrows = (size_t)1 << d.degree_bits;
        const u64 *sec[3] = {d.k_is, d.constants, d.sigmas};
        const size_t cnt[3] = {d.num_routed_wires, (size_t)d.num_constants * nrows, (size_t)d.num_routed_wires * nrows};
        const char *names[3] = {"k_is", "constants", "sigmas"};
        for (int i = 0; i < 3; i++) {
            const size_t bad = first_noncanonical(sec[i], cnt[i]);
            GLP_REQUIRE(bad == cnt[i], "%s[%zu] = 0x%016llx is not a canonical field element (>= p)", names[i], bad, (unsigned long long)sec[i][bad]);
        }
    }

    std::unique_ptr<glp_circuit, void (*)(glp_circuit *)> cc(new glp_circuit(), glp_circuit_free);
    cc->ctx = c;
    cc->d = d;
    cc->gates.assign(d.gates, d.gates + d.num_gates);
    cc->k_is.assign(d.k_is, d.k_is + d.num_routed_wires);
    cc->k_ratio = coset_shift_ratio(cc->k_is.data(), cc->k_is.size());
    cc->d.gates = cc->gates.data(); cc->d.k_is = cc->k_is.data(); cc->d.constants = nullptr; cc->d.sigmas = nullptr;
    cc->zk = (flags & GLP_CIRCUIT_ZERO_KNOWLEDGE) != 0;
    make_layout(cc->d, cc->L, cc->zk);
    const size_t n = (size_t)1 << d.degree_bits;
    const u32 nc = d.num_constants, nr = d.num_routed_wires;
    GLP_TRY(c->alloc((void **)&cc->dev_gates, sizeof(DevGate) * d.num_gates + 8 * COSET_TABLE_WORDS));      // gate table ++ coset_table
    GLP_TRY(c->alloc((void **)&cc->dev_k_is, (size_t)nr * 8));
    GLP_TRY(c->alloc((void **)&cc->dev_sigmas, (size_t)nr * n * 8));
    static_assert(sizeof(DevGate) == sizeof(glp_gate), "gate layout");
    GLP_TRY(h2d(c, cc->dev_gates, cc->gates.data(), sizeof(DevGate) * d.num_gates));
    {
        u64 tab[COSET_TABLE_WORDS];
        coset_table_fill(tab);
        GLP_TRY(h2d(c, cc->dev_gates + d.num_gates, tab, sizeof(tab)));
    }
    GLP_TRY(h2d(c, cc->dev_k_is, cc->k_is.data(), (size_t)nr * 8));
    GLP_TRY(h2d(c, cc->dev_sigmas, d.sigmas, (size_t)nr * n * 8));
    GLP_TRY(c->alloc((void **)&cc->dev_consts, (size_t)nc * n * 8));
    GLP_TRY(h2d(c, cc->dev_consts, d.constants, (size_t)nc * n * 8));
    GLP_TRY(build_quotient_plan(c, cc.get()));
    if (!cc->program_gates.empty()) {              // the programs: host copies for the verifier, one device image for the kernels
        std::vector<u64> img;
        for (u32 i = 0; i < num_programs; i++) {
            const glp_gate_program_desc &pd = programs[i];
            glp_circuit::Program pr;
            pr.code.assign(pd.code, pd.code + pd.num_instructions);
            pr.pool.assign(pd.pool, pd.pool + pd.num_pool);
            pr.nregs = pd.num_regs; pr.dev_at = img.size();
            img.insert(img.end(), pr.code.begin(), pr.code.end());
            img.resize((img.size() + 3) & ~(size_t)3, 0);
            img.insert(img.end(), pr.pool.begin(), pr.pool.end());
            img.resize((img.size() + 3) & ~(size_t)3, 0);
            cc->programs.push_back(std::move(pr));
        }
        GLP_TRY(c->alloc((void **)&cc->dev_programs, img.size() * 8));
        GLP_TRY(h2d(c, cc->dev_programs, img.data(), img.size() * 8));
    }
    {
        Scratch sc(c);
        u64 *csv;
        GLP_TRY(sc.words(&csv, (size_t)(nc + nr) * n));
        GLP_HIP(hipMemcpyAsync(csv, cc->dev_consts, (size_t)nc * n * 8, hipMemcpyDeviceToDevice, c->stream));
        GLP_HIP(hipMemcpyAsync(csv + (size_t)nc * n, cc->dev_sigmas, (size_t)nr * n * 8, hipMemcpyDeviceToDevice, c->stream));
        GLP_TRY(batch_build(c, csv, BATCH_VALUES, nc + nr, (int)d.degree_bits, (int)d.rate_bits, (int)d.cap_height, &cc->cs, nullptr, 1, (int)d.hasher));
    }
    GLP_TRY(batch_cap_host(c, cc->cs, cc->cs_cap));
    bool zero = true;
    for (int i = 0; i < 4; i++) zero = zero && d.circuit_digest[i] == 0;
    if (zero && d.hasher == GLP_HASH_KECCAK25) {
        // the same recipe with C::Hasher = KeccakHash<25>: every hash enters as its four 7-byte chunks (BytesHash::to_vec)
        u64 pad[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, ds[4], e[4];
        kec::host_hash_no_pad(pad, 12, ds);
        std::vector<u64> parts;
        for (size_t i = 0; i < cc->cs_cap.size(); i += 4) { kec::digest_to_elements(&cc->cs_cap[i], e); parts.insert(parts.end(), e, e + 4); }
        kec::digest_to_elements(ds, e);
        parts.insert(parts.end(), e, e + 4);
        parts.push_back(d.degree_bits);
        kec::host_hash_no_pad(parts.data(), parts.size(), cc->digest);
    } else if (zero) {
        // hash_pad([]) = hash_no_pad([1, 0 x 10, 1]); digest = hash_no_pad(cap ++ that ++ [degree_bits])
        u64 pad[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, ds[4];
        host_hash_no_pad(pad, 12, ds);
        std::vector<u64> parts(cc->cs_cap);
        parts.insert(parts.end(), ds, ds + 4);
        parts.push_back(d.degree_bits);
        host_hash_no_pad(parts.data(), parts.size(), cc->digest);
    } else {
        memcpy(cc->digest, d.circuit_digest, 32);
    }
    memcpy(cc->d.circuit_digest, cc->digest, 32);
    *out = cc.release();
    return GLP_OK;
}

int glp_circuit_digest(const glp_circuit *cc, uint64_t out[4]) {
    GLP_REQUIRE(cc && out, "null argument");
    memcpy(out, cc->digest, 32);
    return GLP_OK;
}
int glp_circuit_constants_sigmas_cap(const glp_circuit *cc, uint64_t *cap_out) {
    GLP_REQUIRE(cc && cap_out, "null argument");
    memcpy(cap_out, cc->cs_cap.data(), cc->cs_cap.size() * 8);
    return GLP_OK;
}
size_t glp_proof_words(const glp_circuit *cc) { return cc ? cc->L.total : 0; }
int glp_circuit_zero_knowledge(const glp_circuit *cc) { return cc && cc->zk ? 1 : 0; }
}  // extern "C"
