"""CPU checks of the launch-path matrix (launch_matrix.py): every case reaches the paths it exists for, the cases together
reach every path the prover has, and every case's witness satisfies its circuit (the oracle proves and accepts it).  The wide
circuits of launch_matrix.WIDE_CASES are cases like any other here; their term counts are pinned to the accumulator bound."""
import pytest

import launch_matrix as lm

CASES = lm.CASES + lm.WIDE_CASES


@pytest.fixture(scope="module")
def descs():
    return {c.id: c.build() for c in CASES}


def _plans(c, desc):
    """the plans a case is run under on the GPU: one proof, the batch (two challenges) and the forced leaf-hash forms"""
    out = [lm.launch_plan(desc)]
    if desc.num_challenges == 2:
        out.append(lm.launch_plan(desc, K=c.batch_k))
    if c.id in lm.FORM_CASES:
        out += [lm.launch_plan(desc, coop_max=cm, quad_max=qm) for cm, qm in lm.MERKLE_FORMS.values()]
    return out


def test_case_ids_are_unique():
    assert len(lm.BY_ID) == len(CASES)
    assert set(lm.FORM_CASES) <= set(lm.BY_ID) and set(lm.BATCH_PATHS) <= set(lm.BY_ID)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_reaches_its_paths(descs, case):
    desc = descs[case.id]
    plan = lm.launch_plan(desc)
    assert case.paths <= plan, sorted(case.paths - plan)
    if case.id in lm.BATCH_PATHS:
        batch = lm.launch_plan(desc, K=case.batch_k)
        assert lm.BATCH_PATHS[case.id] <= batch, sorted(lm.BATCH_PATHS[case.id] - batch)


def test_cases_cover_every_path(descs):
    reached = set()
    for c in CASES:
        for p in _plans(c, descs[c.id]):
            reached |= p
    assert sorted(reached) == lm.ALL_PATHS, dict(orphaned=sorted(set(lm.ALL_PATHS) - reached), unlisted=sorted(reached - set(lm.ALL_PATHS)))


def test_forced_forms_reach_each_leaf_hash_form(descs):
    for form, (cm, qm) in lm.MERKLE_FORMS.items():
        for cid in lm.FORM_CASES:
            plan = lm.launch_plan(descs[cid], coop_max=cm, quad_max=qm)
            assert "fri_leaf_" + form in plan and not {"fri_leaf_" + f for f in lm.MERKLE_FORMS if f != form} & plan, (cid, form)


def test_plan_follows_the_limb_group_rules(descs):
    """spot checks of the restated rules against counts worked out by hand"""
    q = lm.quotient_plan(descs["limbs22"])
    assert len(q["limb"]) == 20 and q["groups"] == 4 and len(q["single"]) == 2
    q = lm.quotient_plan(descs["limbs22_w300"])
    assert q["limb"] == [] and len(q["single"]) == 23
    q = lm.quotient_plan(descs["limbs1"])
    assert q["limb"] == [] and q["demoted"] is not None and len(q["extra"]) == 0
    q = lm.quotient_plan(descs["comparison6"])
    assert len(q["extra"]) == 4 and len(q["single"]) == 2
    q = lm.quotient_plan(descs["light10"])
    assert len(q["light"]) == 8 and len(q["single"]) == 2 and q["arith"] is not None


def test_wide_cases_sit_on_the_accumulator_bound(descs):
    """the widths were chosen from these counts: a change in synth's column counts must not move a case off its boundary in silence"""
    for lg, nw, paths in lm.WIDE_WIDTHS:
        desc = descs[lm.wide_id(lg, nw)]
        assert lm.opened_columns(desc) == [83, nw, 20, 16] and desc.degree_bits == lg
        assert lm.final_values_terms(desc) == lm.WIDE_TERMS[lg, nw]
    t = lm.WIDE_TERMS
    assert t[7, 1928] == t[8, 905] == lm.ACC_MAX_TERMS and t[7, 1929] == t[8, 906] == lm.ACC_MAX_TERMS + 1
    assert 2 * lm.ACC_MAX_TERMS < t[8, 2100] < 3 * lm.ACC_MAX_TERMS and min(t[7, 10000], t[8, 6000]) > 4400
    # which kernel each takes: the small one up to the bound and not past it; the flush path only past 1024 columns
    plans = {(lg, nw): lm.launch_plan(descs[lm.wide_id(lg, nw)]) for lg, nw, _ in lm.WIDE_WIDTHS}
    assert "fv_small_wide_fallback" not in plans[7, 1928] and "fv_small_lg7_nch2" not in plans[7, 1929]
    assert "fv_large_flush" not in plans[8, 905] and "fv_large_flush" in plans[8, 906]
    # the batch of small proofs the benchmark runs stays on the small kernel
    assert "fv_small_lg3_nch2" in lm.launch_plan(descs["zkdsa_nch2"], K=2)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_oracle_proves_and_accepts_the_witness(oracle, descs, case):
    desc = descs[case.id]
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0 and oc.verify(proof) == 0
