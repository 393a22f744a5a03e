// circuit_create.inc -- the circuit handle: the quotient launch plan, the uploads and the constants/sigmas commitment around the host
// half of circuit_common.h (the rules a description is held to, the verifier's view, the digest), and the entry points that only read
// the view.  Included by prover.hip after the session.

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

static_assert(CIRCUIT_MAX_DEGREE_BITS == NTT_MAX_LG, "circuit_desc_check refuses what the transforms do not take");

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
    GLP_TRY(circuit_desc_check(d, programs, num_programs));
    GLP_TRY(circuit_fields_check(d, true));

    std::unique_ptr<glp_circuit, void (*)(glp_circuit *)> cc(new glp_circuit(), glp_circuit_free);
    cc->ctx = c;
    circuit_common_describe(*cc, d, flags, programs, num_programs);
    cc->k_ratio = coset_shift_ratio(cc->k_is.data(), cc->k_is.size());
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
    if (!cc->program_gates.empty()) {              // the programs: one device image for the kernels
        std::vector<u64> img;
        for (const glp_circuit::Program &pr : cc->programs) {
            cc->dev_at.push_back(img.size());
            img.insert(img.end(), pr.code.begin(), pr.code.end());
            img.resize((img.size() + 3) & ~(size_t)3, 0);
            img.insert(img.end(), pr.pool.begin(), pr.pool.end());
            img.resize((img.size() + 3) & ~(size_t)3, 0);
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
    std::vector<u64> cap;
    GLP_TRY(batch_cap_host(c, cc->cs, cap));
    circuit_common_commit(*cc, cap);
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

// the proof as bytes (proof_bytes.h)
size_t glp_proof_bytes_len(const glp_circuit *cc) { return cc ? proof_bytes_len(*cc) : 0; }
int glp_proof_to_bytes(const glp_circuit *cc, const uint64_t *words, uint8_t *out, size_t len) {
    GLP_REQUIRE(cc && words && out, "null argument");
    return proof_to_bytes(*cc, words, out, len);
}
int glp_proof_from_bytes(const glp_circuit *cc, const uint8_t *in, size_t len, uint64_t *words) {
    GLP_REQUIRE(cc && words && in, "null argument");
    return proof_from_bytes(*cc, in, len, words);
}
}  // extern "C"
