"""The launch paths of the prover and a deterministic matrix of circuits that reaches each of them (a helper module, not
collected by pytest: test_launch_plan.py checks the matrix on the CPU, test_gpu_launch_paths.py proves it on the GPU).

The prover chooses its kernels at run time from the circuit's shape.  `launch_plan` restates those choices in Python and
names each one; `CASES` lists circuits, each with the paths it exists for.  A rule change in the C++ that this module
does not follow makes test_launch_plan.py fail (a path no case reaches any more, or a case that lost its path)."""
import collections
import os

import numpy as np

import plonky2_lib_amd.synth as synth

LIMB_SLOTS, LIMB_GROUPS = 5, 4            # quotient_kernels.inc: constexpr int LIMB_SLOTS = 5, LIMB_GROUPS = 4
LIGHT_MAX, EXTRA_MAX = 8, 4               # quotient_kernels.inc: LightArgs::gi[8], LimbArgs::extra_gi[4]
PP_SMALL_LDS = 64 * 1024                  # prover_stages.inc stage_partial_products(): small_lds <= 64 KiB
MERKLE_COOP_MAX, MERKLE_QUAD_MAX = 4096, 32768   # common.h: glp_ctx::merkle_coop_max / merkle_quad_max (GLP_MERKLE_COOP_MAX / _QUAD_MAX)
ACC_MAX_TERMS = 1024                      # acc.h: terms a carry-free AccLimb holds before it must be reduced

# context thresholds that force one FRI leaf-hash form (the values test_gpu_commit.py::test_leaf_hash_forms uses)
MERKLE_FORMS = {"lane": (0, 0), "quad": (0, 1 << 40), "coop": (1 << 40, 1 << 40)}

_LIMB = (synth.GATE_U32_ARITHMETIC, synth.GATE_U32_ADD_MANY, synth.GATE_U32_SUBTRACTION, synth.GATE_U32_RANGE_CHECK)
_LIGHT = (synth.GATE_CONSTANT, synth.GATE_PUBLIC_INPUT, synth.GATE_ARITHMETIC, synth.GATE_BASE_SUM, synth.GATE_RANDOM_ACCESS)
_INTERLEAVE = (synth.GATE_U32_INTERLEAVE, synth.GATE_UNINTERLEAVE_U32, synth.GATE_UNINTERLEAVE_B32)
GATE_NAMES = {synth.GATE_CONSTANT: "constant", synth.GATE_PUBLIC_INPUT: "public_input", synth.GATE_ARITHMETIC: "arithmetic",
              synth.GATE_POSEIDON: "poseidon", synth.GATE_U32_INTERLEAVE: "u32_interleave", synth.GATE_UNINTERLEAVE_U32: "uninterleave_u32",
              synth.GATE_UNINTERLEAVE_B32: "uninterleave_b32", synth.GATE_U32_ARITHMETIC: "u32_arithmetic",
              synth.GATE_U32_ADD_MANY: "u32_add_many", synth.GATE_U32_SUBTRACTION: "u32_subtraction",
              synth.GATE_U32_RANGE_CHECK: "u32_range_check", synth.GATE_COMPARISON: "comparison", synth.GATE_BASE_SUM: "base_sum",
              synth.GATE_RANDOM_ACCESS: "random_access"}


def quotient_plan(desc):
    """circuit_create.inc build_quotient_plan(): which launch of the two-challenge quotient evaluates each gate (by index into desc.gates)."""
    limb, light, single, extra = [], [], [], []
    arith = None
    for gi, g in enumerate(desc.gates):
        t = g["type"]
        if t in _LIMB and len(limb) < LIMB_SLOTS * LIMB_GROUPS and desc.num_wires <= 256:
            limb.append(gi)
        elif (t == synth.GATE_ARITHMETIC and arith is None and 4 * g["p0"] <= desc.num_routed_wires
              and desc.quotient_degree_factor % 4 == 0 and desc.num_selectors + 2 <= desc.num_constants):
            arith = gi                                   # fused into the permutation loop of k_quotient<2, 2>
        elif t in _LIGHT and len(light) < LIGHT_MAX:
            light.append(gi)
        elif t != synth.GATE_NOOP:
            single.append(gi)
    demoted = None
    if len(limb) == 1:                                   # "nothing to share: the gate's own kernel is the better launch"
        demoted = limb[0]
        single.append(limb.pop())
    if limb:                                             # ComparisonGate rides with the limb launch, at most four of them
        keep = []
        for gi in single:
            if desc.gates[gi]["type"] == synth.GATE_COMPARISON and len(extra) < EXTRA_MAX:
                extra.append(gi)
            else:
                keep.append(gi)
        single = keep
    return dict(limb=limb, groups=-(-len(limb) // LIMB_SLOTS), light=light, arith=arith, single=single, extra=extra, demoted=demoted)


def opened_columns(desc):
    """polynomials of the four oracles the FRI batch polynomial sums: constants ++ sigmas, wires, Zs ++ partial products, quotient chunks"""
    nch = desc.num_challenges
    return [desc.num_constants + desc.num_routed_wires, desc.num_wires, nch * (1 + desc.num_partial_products),
            nch * desc.quotient_degree_factor]


def final_values_terms(desc):
    """terms the busiest lane of the final-values kernel adds up.  4..128 rows (k_final_values_small): 256 / n lanes share a point,
    lane t takes the columns t, t + lpp, .. of each oracle, so lane 0 carries sum_k ceil(ncols[k] / lpp).  Otherwise
    (k_final_values) one lane walks every column."""
    lg = desc.degree_bits
    lpp = 256 >> lg if 2 <= lg <= 7 else 1
    return sum(-(-c // lpp) for c in opened_columns(desc))


def launch_plan(desc, K=1, coop_max=MERKLE_COOP_MAX, quad_max=MERKLE_QUAD_MAX):
    """The set of launch-path names one glp_prove (K = 1) or one glp_prove_batch of K proofs takes (prover_stages.inc)."""
    nch, lg, rb, qdf = desc.num_challenges, desc.degree_bits, desc.rate_bits, desc.quotient_degree_factor
    if K > 1 and nch != 2:
        raise ValueError("glp_prove_batch takes two challenges only (prover_stages.inc batch_check())")
    out = set()
    # quotient: Rq = qdf cosets evaluated, every 2^rb / qdf-th LDE plane (prover_stages.inc prove_geo())
    out.add("quotient_rq%d_step%d" % (qdf, (1 << rb) // qdf))
    types = {g["type"] for g in desc.gates} - {synth.GATE_NOOP}
    if nch != 2:
        # stage_quotient_eval(): gate_mode 0, k_quotient<NCH, 1>: every gate through gate_contrib<NCH, -1>
        out.add("quotient_monolithic_nch%d" % nch)
        out |= {"monolithic_" + GATE_NAMES[t] for t in types}
    else:
        # stage_quotient_eval(): k_quotient<2, 2> (light gates, fused ArithmeticGate) or <2, 0>;
        # then k_quotient_limbs<2> and one k_quotient_gate<2, T> per gate in single_gates (plan: circuit_create.inc build_quotient_plan())
        qp = quotient_plan(desc)
        gt = lambda gi: desc.gates[gi]["type"]
        out.add("quotient_perm_light" if qp["light"] or qp["arith"] is not None else "quotient_perm_only")
        if qp["arith"] is not None:
            out.add("arith_fused")
            if any(gt(gi) == synth.GATE_ARITHMETIC for gi in qp["light"] + qp["single"]):
                out.add("arith_second_light")
        if qp["light"]:
            out.add("light_gates_8" if len(qp["light"]) == LIGHT_MAX else "light_gates")
        if any(gt(gi) in _LIGHT for gi in qp["single"]):
            out.add("light_overflow_single")
        if qp["limb"]:
            out.add("limb_groups_%d" % qp["groups"])
        if qp["demoted"] is not None:
            out.add("limb_single")
        nlimb = sum(1 for g in desc.gates if g["type"] in _LIMB)
        if nlimb > 1 and any(gt(gi) in _LIMB for gi in qp["single"]):
            out.add("limb_wide_single" if desc.num_wires > 256 else "limb_overflow_single")
        if qp["extra"]:
            out.add("comparison_extra_4" if len(qp["extra"]) == EXTRA_MAX else "comparison_extra")
        if any(gt(gi) == synth.GATE_COMPARISON for gi in qp["single"]):
            out.add("comparison_extra_overflow_single" if qp["limb"] else "comparison_single_no_limbs")
        if any(gt(gi) == synth.GATE_POSEIDON for gi in qp["single"]):
            out.add("single_poseidon")
        if any(gt(gi) in _INTERLEAVE for gi in qp["single"]):
            out.add("single_interleave")
    # partial products: stage_partial_products()
    npp = desc.num_partial_products
    small_lds = 2 * nch * (npp + 2) * (1 << lg) * 8
    if lg <= 7 and small_lds <= PP_SMALL_LDS:
        out.add("pp_small_lg%d" % lg)
    else:
        out.add("pp_large_lds_fallback" if lg <= 7 else "pp_large")
    # final values (FRI combination): stage_fri_values(); 256 / n lanes per point while no lane passes ACC_MAX_TERMS terms
    # (final_values_small_fits(): k_final_values_small never flushes), else k_final_values, which flushes every ACC_MAX_TERMS columns
    if 2 <= lg <= 7 and final_values_terms(desc) <= ACC_MAX_TERMS:
        out.add("fv_small_lg%d_nch%d" % (lg, nch) if lg in (2, 3, 7) else "fv_small_nch%d" % nch)
    elif 2 <= lg <= 7:
        # the fallback runs k_final_values on more than ACC_MAX_TERMS columns by construction, so this name implies its flush
        # too; fv_large_flush is kept for 2^8 rows and more, where the two can be told apart
        out.add("fv_small_wide_fallback")
    else:
        out.add("fv_large_nch%d" % nch)
        if sum(opened_columns(desc)) > ACC_MAX_TERMS:
            out.add("fv_large_flush")
    # FRI leaf hash of each reduction: stage_fri_commit() (nleaves * K)
    lgcur = lg
    for ab in desc.reduction_arity_bits:
        nleaves = 1 << (lgcur + rb - ab)
        if getattr(desc, "hasher", 0) == 1:
            out.add("fri_leaf_keccak")
        elif nleaves * K <= coop_max:
            out.add("fri_leaf_coop")
        elif nleaves * K <= quad_max:
            out.add("fri_leaf_quad")
        else:
            out.add("fri_leaf_lane")
        lgcur -= ab
    if K > 1:
        out.add("batch_k%d" % K)
    return out


ALL_PATHS = sorted(
    ["quotient_rq8_step1", "quotient_rq4_step2", "quotient_rq16_step1"]
    + ["quotient_monolithic_nch%d" % n for n in (1, 3, 4)]
    + ["monolithic_" + name for name in GATE_NAMES.values()]
    + ["quotient_perm_light", "arith_fused", "arith_second_light", "light_gates", "light_gates_8", "light_overflow_single",
       "limb_groups_1", "limb_groups_2", "limb_groups_3", "limb_groups_4", "limb_single", "limb_overflow_single", "limb_wide_single",
       "comparison_extra", "comparison_extra_4", "comparison_extra_overflow_single", "comparison_single_no_limbs",
       "single_poseidon", "single_interleave"]
    + ["pp_small_lg%d" % lg for lg in range(2, 8)] + ["pp_large_lds_fallback", "pp_large"]
    + ["fv_small_lg%d_nch%d" % (lg, n) for lg in (2, 3, 7) for n in (1, 2, 3, 4)]
    + ["fv_small_nch%d" % n for n in (1, 2, 3, 4)] + ["fv_large_nch%d" % n for n in (1, 2, 3, 4)]
    + ["fv_small_wide_fallback", "fv_large_flush"]
    + ["fri_leaf_coop", "fri_leaf_quad", "fri_leaf_lane", "fri_leaf_keccak", "batch_k2", "batch_k9"])

# ------------------------------------------------------------------------------------------------ circuit builders

# distinct limb gates, widest first within a type (each fits 136 wires): 8 + 6 + 3 + 5 = 22
RANGE_CHECKS = [(synth.GATE_U32_RANGE_CHECK, p, 0) for p in range(8, 0, -1)]
SUBTRACTIONS = [(synth.GATE_U32_SUBTRACTION, p, 0) for p in range(6, 0, -1)]
U32_ARITHS = [(synth.GATE_U32_ARITHMETIC, p, 0) for p in range(3, 0, -1)]
ADD_MANYS = [(synth.GATE_U32_ADD_MANY, na, nops) for na, nops in ((16, 3), (8, 4), (3, 5), (2, 1), (1, 6))]
LIMB_GATES = RANGE_CHECKS + SUBTRACTIONS + U32_ARITHS + ADD_MANYS
# ComparisonGate (num_bits, num_chunks): 2, 3, 1, 2, 3, 3 bits per chunk (degree 2^chunk_bits: at most 8)
COMPARISONS = [(synth.GATE_COMPARISON, nb, nc) for nb, nc in ((32, 16), (30, 10), (8, 8), (16, 8), (12, 4), (62, 21))]
BASE_SUMS = [(synth.GATE_BASE_SUM, nl, 4) for nl in range(1, 9)]


def _limbs(count):
    """`count` distinct limb gates, the types interleaved so that every prefix mixes them"""
    order = []
    for i in range(max(len(RANGE_CHECKS), len(SUBTRACTIONS), len(U32_ARITHS), len(ADD_MANYS))):
        for lst in (RANGE_CHECKS, SUBTRACTIONS, ADD_MANYS, U32_ARITHS):
            if i < len(lst):
                order.append(lst[i])
    assert count <= len(order)
    return order[:count]


def _config(nw=136, **kw):
    return synth.Config(nw, 80, **kw)


def gate_rows(kinds, second_arith=0):
    """extra_rows callback for synth.arith_circuit: one row per gate kind (and for a Comparison kind a second row with
    equal inputs), then `second_arith` rows of a 10-op ArithmeticGate."""
    def fill(b, row):
        for t, p0, p1 in kinds:
            row = synth.fill_gate_row(b, row, t, p0, p1)
            if t == synth.GATE_COMPARISON:
                row = synth.fill_gate_row(b, row, t, p0, p1, equal_inputs=True)
        if second_arith:
            synth._fill_arith_rows(b, np.arange(row, row + second_arith), num_ops=10)
            row += second_arith
        return row
    return fill


def mixed(lg, kinds, nw=136, seed=1, second_arith=0, hasher=0, **kw):
    desc = synth.arith_circuit(lg, _config(nw, **kw), seed=seed, extra_rows=gate_rows(kinds, second_arith))
    if hasher:
        desc.hasher, desc.circuit_digest = hasher, None
    return desc


def ecdsa_set(lg, seed=3, hasher=0, **kw):
    """the seven remaining gate types of the secp256k1 circuit (synth.fill_ecdsa_gate_rows), one row each"""
    desc = synth.arith_circuit(lg, _config(136, **kw), seed=seed, ecdsa_gate_rows=1)
    if hasher:
        desc.hasher, desc.circuit_digest = hasher, None
    return desc


def keccak_set(lg, seed=4, **kw):
    """synth.keccak_shape_circuit under another configuration: u32 arithmetic gates + the three interleave gates, 135 wires"""
    rows = lambda b, row: synth._fill_interleave_rows(b, row, 1)
    return synth.arith_circuit(lg, synth.Config(135, 80, **kw), seed=seed, ecdsa_gate_rows=1,
                               ecdsa_gate_subset=(synth.GATE_U32_ARITHMETIC, synth.GATE_U32_ADD_MANY, synth.GATE_U32_SUBTRACTION),
                               extra_rows=rows)


def zkdsa(seed=5, **kw):
    return synth.zkdsa_circuit(3, synth.Config(135, 80, **kw), seed=seed)


def smt(lg, seed=7, **kw):
    return synth.smt_shape_circuit(lg, synth.Config(135, 80, **kw), seed=seed)


def tiny(lg, seed=11, **kw):
    """[PublicInput][Constant][Arithmetic ...][Noop]: the smallest circuit the prover takes, from 4 rows"""
    cfg = synth.Config(135, 80, **kw)
    b = synth.Builder(cfg, lg, seed)
    n = b.n
    b.set_rows(np.array([0]), synth.GATE_PUBLIC_INPUT, 0)
    b.set_rows(np.array([1]), synth.GATE_CONSTANT, cfg.num_constants)
    b.gate_consts[:, 1] = 0
    b.wires[:cfg.num_constants, 1] = 0
    b.wires[:4, 0] = 0                               # no public inputs: the hash cells are zero, tied to the constant zero
    b.connect_cycle([1, 0, 0, 0, 0], [0, 0, 1, 2, 3])
    synth._fill_arith_rows(b, np.arange(2, n - 1))
    return b.build()


Case = collections.namedtuple("Case", "id build paths batch_k")


def _case(cid, build, paths, batch_k=2):
    return Case(cid, build, frozenset(paths), batch_k)


CASES = [
    # the monolithic quotient kernel (num_challenges 1, 3, 4) x gate families
    _case("ecdsa_nch1_lg7", lambda: ecdsa_set(7, num_challenges=1),
          {"quotient_monolithic_nch1", "monolithic_comparison", "monolithic_u32_range_check", "monolithic_random_access", "fv_small_lg7_nch1"}),
    _case("ecdsa_nch3_lg8", lambda: ecdsa_set(8, num_challenges=3), {"quotient_monolithic_nch3", "monolithic_base_sum", "fv_large_nch3", "pp_large"}),
    _case("ecdsa_nch4_lg7", lambda: ecdsa_set(7, num_challenges=4),
          {"quotient_monolithic_nch4", "monolithic_u32_add_many", "pp_large_lds_fallback", "fv_small_lg7_nch4"}),
    _case("keccak_nch1_lg6", lambda: keccak_set(6, num_challenges=1), {"monolithic_u32_interleave", "fv_small_nch1", "pp_small_lg6"}),
    _case("keccak_nch3_lg7", lambda: keccak_set(7, num_challenges=3),
          {"monolithic_uninterleave_u32", "monolithic_uninterleave_b32", "pp_large_lds_fallback", "fv_small_lg7_nch3"}),
    _case("keccak_nch4_lg8", lambda: keccak_set(8, num_challenges=4), {"quotient_monolithic_nch4", "fv_large_nch4"}),
    _case("zkdsa_nch1", lambda: zkdsa(num_challenges=1), {"monolithic_poseidon", "fv_small_lg3_nch1", "pp_small_lg3"}),
    _case("zkdsa_nch3", lambda: zkdsa(num_challenges=3), {"quotient_monolithic_nch3", "fv_small_lg3_nch3"}),
    _case("zkdsa_nch4", lambda: zkdsa(num_challenges=4), {"quotient_monolithic_nch4", "fv_small_lg3_nch4"}),
    _case("smt_nch1_lg8", lambda: smt(8, num_challenges=1), {"monolithic_poseidon", "fv_large_nch1"}),
    _case("smt_nch3_lg5", lambda: smt(5, num_challenges=3), {"monolithic_base_sum", "fv_small_nch3", "pp_small_lg5"}),
    _case("smt_nch4_lg6", lambda: smt(6, num_challenges=4), {"monolithic_constant", "fv_small_nch4", "pp_small_lg6"}),
    # the same families with two challenges (the split quotient launches)
    _case("ecdsa_nch2_lg7", lambda: ecdsa_set(7), {"limb_groups_1", "comparison_extra", "light_gates", "arith_fused", "fv_small_lg7_nch2"}),
    _case("keccak_nch2_lg6", lambda: keccak_set(6), {"single_interleave", "limb_groups_1", "fv_small_nch2"}),
    _case("zkdsa_nch2", lambda: zkdsa(), {"single_poseidon", "fv_small_lg3_nch2", "pp_small_lg3"}),
    _case("smt_nch2_lg8", lambda: smt(8), {"single_poseidon", "light_gates", "fv_large_nch2", "pp_large"}),
    # smallest traces: 4 and 16 rows, every challenge count
    _case("tiny_lg2_nch1", lambda: tiny(2, num_challenges=1), {"monolithic_arithmetic", "monolithic_public_input", "pp_small_lg2", "fv_small_lg2_nch1"}),
    _case("tiny_lg2_nch2", lambda: tiny(2), {"pp_small_lg2", "fv_small_lg2_nch2", "arith_fused"}),
    _case("tiny_lg2_nch3", lambda: tiny(2, num_challenges=3), {"pp_small_lg2", "fv_small_lg2_nch3"}),
    _case("tiny_lg2_nch4", lambda: tiny(2, num_challenges=4), {"pp_small_lg2", "fv_small_lg2_nch4"}),
    _case("tiny_lg4_nch2", lambda: tiny(4), {"pp_small_lg4", "fv_small_nch2"}),
    # limb-gate counts: 0, 1, 2-5, 6-10, 11-15, 16-20, 21+ (one group of LIMB_SLOTS = 5 per launch pass, at most 4 groups)
    _case("limbs0_comparison", lambda: mixed(7, COMPARISONS[:2]), {"comparison_single_no_limbs"}),
    _case("limbs1", lambda: mixed(7, _limbs(1) + COMPARISONS[:1]), {"limb_single", "comparison_single_no_limbs"}),
    _case("limbs3", lambda: mixed(7, _limbs(3)), {"limb_groups_1"}),
    _case("limbs5", lambda: mixed(7, _limbs(5)), {"limb_groups_1"}),
    _case("limbs8", lambda: mixed(7, _limbs(8)), {"limb_groups_2"}),
    _case("limbs13", lambda: mixed(7, _limbs(13)), {"limb_groups_3"}),
    _case("limbs18", lambda: mixed(7, _limbs(18)), {"limb_groups_4"}),
    _case("limbs20", lambda: mixed(7, _limbs(20)), {"limb_groups_4"}),
    _case("limbs22", lambda: mixed(7, _limbs(22)), {"limb_groups_4", "limb_overflow_single"}),
    _case("limbs22_w256", lambda: mixed(7, _limbs(22), nw=256), {"limb_groups_4", "limb_overflow_single"}),
    _case("limbs22_w300", lambda: mixed(7, _limbs(22) + COMPARISONS[:1], nw=300), {"limb_wide_single", "comparison_single_no_limbs"}),
    # light gates (Constant, PublicInput, BaseSum, RandomAccess, a second ArithmeticGate): 8 share k_quotient<2, 2>, the 9th goes alone
    _case("light8", lambda: mixed(7, _limbs(2) + BASE_SUMS[:6]), {"light_gates_8"}),
    _case("light10", lambda: mixed(7, _limbs(2) + BASE_SUMS[:8]), {"light_overflow_single"}),
    _case("arith_two_kinds", lambda: mixed(7, _limbs(2), second_arith=3), {"arith_fused", "arith_second_light"}),
    # ComparisonGate riding on the limb launch: 4 fit, the 5th goes alone
    _case("comparison4", lambda: mixed(7, _limbs(6) + COMPARISONS[:4]), {"comparison_extra_4", "limb_groups_2"}),
    _case("comparison6", lambda: mixed(7, _limbs(6) + COMPARISONS), {"comparison_extra_4", "comparison_extra_overflow_single"}),
    # LDS bound of k_pp_rows_small at 64 and 128 rows, quotient planes away from Rq = 8
    _case("pp_fallback_lg6_nch4_qdf4", lambda: mixed(6, [], num_challenges=4, max_quotient_degree_factor=4),
          {"pp_large_lds_fallback", "quotient_rq4_step2", "fv_small_nch4"}),
    _case("pp_fallback_lg7_nch2_qdf4", lambda: mixed(7, [], max_quotient_degree_factor=4), {"pp_large_lds_fallback", "quotient_rq4_step2"}),
    _case("pp_small_lg7_nch2", lambda: mixed(7, []), {"pp_small_lg7", "quotient_rq8_step1"}),
    _case("ecdsa_qdf16_rb4", lambda: ecdsa_set(7, max_quotient_degree_factor=16, rate_bits=4, num_query_rounds=20),
          {"quotient_rq16_step1", "limb_groups_1"}),
    # KeccakGoldilocksConfig
    _case("ecdsa_keccak_nch1", lambda: ecdsa_set(7, num_challenges=1, hasher=1), {"fri_leaf_keccak", "quotient_monolithic_nch1"}),
    _case("ecdsa_keccak_nch4", lambda: ecdsa_set(8, num_challenges=4, hasher=1), {"fri_leaf_keccak", "quotient_monolithic_nch4"}),
    # a batch whose first FRI layer crosses the cooperative / quad leaf-hash threshold: 512 leaves x 9 proofs > 4096
    _case("arith_lg10_batch9", lambda: mixed(10, _limbs(4)), {"fri_leaf_coop", "limb_groups_1"}, batch_k=9),
]

# what the batch of a case adds (device transcript): checked on the batch plan, so that K = 9 crossing the threshold is pinned
BATCH_PATHS = {"arith_lg10_batch9": {"fri_leaf_quad", "batch_k9"}, "ecdsa_nch2_lg7": {"batch_k2", "fri_leaf_coop"}}

# cases the forced leaf-hash forms are run on (test_gpu_launch_paths.py::test_forced_merkle_forms)
FORM_CASES = ["ecdsa_nch2_lg7", "smt_nch2_lg8", "keccak_nch2_lg6", "limbs13"]

# Circuits wide enough to reach the term bounds of the carry-free accumulators in the final-values kernels (a list of its own:
# test_gpu_wide_shapes.py proves these, test_gpu_launch_paths.py keeps to CASES).  mixed(lg, [], nw=W) opens [83, W, 20, 16] columns.
# 128 rows, two lanes per point, lane 0 carries 60 + ceil(W / 2) terms; 256 rows, one lane walks all 119 + W columns.
WIDE_WIDTHS = [
    (7, 1928, {"fv_small_lg7_nch2"}),                # lane 0 has exactly ACC_MAX_TERMS terms: the last width the small kernel may take
    (7, 1929, {"fv_small_wide_fallback"}),           # 1025 terms: the first width past the bound
    (7, 10000, {"fv_small_wide_fallback"}),          # about 5060 terms per lane: past where natural data wraps an accumulator
    (8, 905, {"fv_large_nch2"}),                     # 1024 columns: k_final_values flushes on its last term
    (8, 906, {"fv_large_flush"}),                    # 1025 columns: one term after the flush
    (8, 2100, {"fv_large_flush"}),                   # two flushes and a remainder
    (8, 6000, {"fv_large_flush"}),                   # 6119 terms: a missing flush is certain to wrap
]
WIDE_TERMS = {(7, 1928): 1024, (7, 1929): 1025, (7, 10000): 5060, (8, 905): 1024, (8, 906): 1025, (8, 2100): 2219, (8, 6000): 6119}


def wide_id(lg, nw):
    return "wide_lg%d_w%d" % (lg, nw)


WIDE_CASES = [_case(wide_id(lg, nw), (lambda lg=lg, nw=nw: mixed(lg, [], nw=nw)), paths) for lg, nw, paths in WIDE_WIDTHS] + [
    # 2000 routed wires: 249 partial products per challenge, 500 columns in the third oracle, 1 MiB of running products
    _case("wide_routed_lg7", lambda: synth.arith_circuit(7, synth.Config(2100, 2000), seed=3), {"fv_small_wide_fallback", "pp_large_lds_fallback"}),
    # arity 32 (glp_circuit_create's largest): one reduction 2^10 -> 2^5, leaves of 64 words
    _case("arity32_lg10", lambda: mixed(10, [], arity_bits=5, final_poly_bits=0, num_query_rounds=3), {"fv_large_nch2", "fri_leaf_coop"}),
]

BY_ID = {c.id: c for c in CASES + WIDE_CASES}


# ------------------------------------------------------------------------------------------------ shared by the GPU parity tests
_REFS = {}                                   # case id -> (desc, oracle circuit, oracle proof): made once per session, left unchanged


def oracle_ref(oracle, cid):
    """the case's description, its oracle circuit and the oracle's proof (which the oracle verifier accepts)"""
    if cid not in _REFS:
        desc = BY_ID[cid].build()
        oc = oracle.OracleCircuit(desc)
        rc, ref = oc.prove()
        assert rc == 0 and oc.verify(ref) == 0
        _REFS[cid] = desc, oc, ref
    return _REFS[cid]


def head_sections(desc):
    """name -> slice of the proof words (layout: include/glp.h)"""
    cap = 4 << desc.cap_height
    nch = desc.num_challenges
    nopen = (desc.num_constants + desc.num_routed_wires + desc.num_wires + 2 * nch + nch * desc.num_partial_products +
             nch * desc.quotient_degree_factor)
    o, out = 0, {}
    for name, ln in (("wires_cap", cap), ("zs_pp_cap", cap), ("quotient_cap", cap), ("openings", 2 * nopen),
                     ("fri_caps", cap * len(desc.reduction_arity_bits))):
        out[name] = slice(o, o + ln)
        o += ln
    out["rest"] = slice(o, None)
    return out


def assert_sections_equal(got, ref, desc, what):
    for name, sl in head_sections(desc).items():
        assert (got[sl] == ref[sl]).all(), "%s: first mismatch in section %s at word %d" % (
            what, name, sl.start + int(np.argmax(got[sl] != ref[sl])))


def prove_batch(gc, desc, K, host_transcript=False):
    """glp_prove_batch of K copies of the case's witness, under the device transcript or the host one"""
    wires = np.stack([desc.wires] * K)
    pis = np.stack([desc.public_inputs] * K) if len(desc.public_inputs) else None
    if not host_transcript:
        return gc.prove_batch(wires, pis)
    os.environ["GLP_BATCH_HOST_TRANSCRIPT"] = "1"
    try:
        return gc.prove_batch(wires, pis)
    finally:
        del os.environ["GLP_BATCH_HOST_TRANSCRIPT"]
