"""tests/limb_gates_restate.py (constraint bodies of gate types 4-12 and 14) pinned before anything relies on it: zero on the builder's
witnesses, the vanishing identity at zeta on oracle proofs under both hashers with every opening category disturbed, and a single-cell
campaign over every column of each gate against the oracle's prove-then-verify verdict.  No GPU."""
import copy

import numpy as np
import pytest

import plonky2_lib_amd.synth as synth
import limb_gates_restate as lg
import witness_check_restate as wr
import zeta_identity as zi
import zeta_identity_recursion as zr

P = zi.P
CATEGORIES = ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q")
FAMILIES = {
    "u32": lambda: synth.u32_circuit(6),
    "ecdsa": lambda: synth.ecdsa_shape_circuit(5),
    "keccak": lambda: synth.keccak_shape_circuit(5),
    "smt": lambda: synth.smt_shape_circuit(4),
    "zkdsa": lambda: synth.zkdsa_circuit(3),
    "poseidon-chain": lambda: synth.poseidon_chain_circuit(2),
}
# [REF src/zkdsa/circuits/mod.rs:85-101]  PoseidonHash::two_to_one(0, 0) = the permutation of the zero state, first four lanes
KAT_TWO_TO_ONE_ZERO = [4330397376401421145, 14124799381142128323, 8742572140681234676, 14345658006221440202]


def gate_width(g):
    """wire columns gate g constrains, from the gates' definitions (include/glp.h GLP_GATE_*)"""
    t, p0, p1 = int(g["type"]), int(g["p0"]), int(g["p1"])
    if t == lg.COMPARISON:
        return lg.comparison_layout(p0, p1)["wires"]
    if t == lg.RANDOM_ACCESS:
        return lg.random_access_layout(p0, p1)["wires"]
    return {0: 0, 1: p0, 2: 4, 3: 4 * p0, lg.POSEIDON: lg.POS_WIRES, lg.U32_INTERLEAVE: 34 * p0, lg.UNINTERLEAVE_U32: 67 * p0,
            lg.UNINTERLEAVE_B32: 67 * p0, lg.U32_ARITHMETIC: 38 * p0, lg.U32_ADD_MANY: (p0 + 3 + 18) * p1, lg.U32_SUBTRACTION: 21 * p0,
            lg.U32_RANGE_CHECK: 17 * p0, 13: 1 + p0}[t]


def test_round_constants_are_the_published_ones():
    rc = lg.round_constants()
    assert len(rc) == 360 and all(0 <= c < P for c in rc) and rc[0] == 0xB585F766F2144405
    assert lg.poseidon_permute([0] * 12)[:4] == KAT_TWO_TO_ONE_ZERO


def test_every_assigned_type_has_a_body():
    assert set(wr.HAS_BODY) == set(range(19)) | {20, 21, 22}
    assert set(lg.LIMB_GATES) == {synth.GATE_POSEIDON, synth.GATE_U32_INTERLEAVE, synth.GATE_UNINTERLEAVE_U32, synth.GATE_UNINTERLEAVE_B32,
                                  synth.GATE_U32_ARITHMETIC, synth.GATE_U32_ADD_MANY, synth.GATE_U32_SUBTRACTION,
                                  synth.GATE_U32_RANGE_CHECK, synth.GATE_COMPARISON, synth.GATE_RANDOM_ACCESS}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_builder_witnesses_satisfy_every_constraint(family):
    desc = FAMILIES[family]()
    rep, by_gate = wr.check(desc)
    assert wr.as_tuple(rep) == (0, 0, 0) + (None,) * 10 and by_gate == [0] * len(desc.gates)
    for gi, g in enumerate(desc.gates):
        for r in zr.gate_rows(desc, gi)[:2]:
            w = [int(x) for x in desc.wires[:, r]]
            gc = [int(x) for x in desc.constants[desc.num_selectors:, r]]
            assert len(zr.gate_constraints(zi._Fp, g, gc, w, [0] * 4)) == synth.gate_num_constraints(int(g["type"]), int(g["p0"]), int(g["p1"]))


def test_families_cover_the_ten_types():
    seen = {int(g["type"]) for f in FAMILIES.values() for g in f().gates}
    assert set(lg.LIMB_GATES) <= seen


@pytest.mark.parametrize("hasher", [0, 1])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_zeta_identity_on_oracle_proofs(oracle, family, hasher):
    """zr.check accepts the oracle's proof and rejects it with one opening word changed, in each of the seven categories: every
    term of every body, and its position in the alpha sum, against the oracle."""
    desc = FAMILIES[family]()
    desc.hasher = hasher
    desc.proof_of_work_bits = 0                      # the grinding judges nothing here
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0 and oc.verify(proof) == 0
    assert zr.check(desc, proof, desc.circuit_digest, hasher)
    lay = zi.proof_layout(desc)
    rng = np.random.default_rng(17 + hasher)
    for name in CATEGORIES:
        o, cnt = lay[name]
        if name == "wires":
            cnt = max(gate_width(g) for g in desc.gates)             # advice columns past the widest gate are in no constraint
        for word in (o, o + 2 * cnt - 1, o + int(rng.integers(0, 2 * cnt))):
            bad = proof.copy()
            bad[word] = (int(bad[word]) + 1) % P
            assert not zr.check(desc, bad, desc.circuit_digest, hasher), (name, word)


# ---------------------------------------------------------------------------------------------------- single-cell campaign
CAMPAIGN = {"ecdsa": lambda: synth.ecdsa_shape_circuit(5), "keccak": lambda: synth.keccak_shape_circuit(5),
            "poseidon-chain": lambda: synth.poseidon_chain_circuit(2)}
CAMPAIGN_SEED = 3


def _cells(desc):
    """per limb gate: one row drawn per column, every column of the gate's width and every advice column past it"""
    rng = np.random.default_rng(CAMPAIGN_SEED)
    out = []
    for gi, g in enumerate(desc.gates):
        if int(g["type"]) not in lg.LIMB_GATES:
            continue
        rows = zr.gate_rows(desc, gi)
        width = gate_width(g)
        assert width <= desc.num_wires
        cols = list(range(width)) + [c for c in range(max(width, desc.num_routed_wires), desc.num_wires)]
        out += [(gi, int(rows[rng.integers(0, len(rows))]), c) for c in cols]
    return out


@pytest.mark.parametrize("name", sorted(CAMPAIGN))
def test_single_cell_campaign_against_the_oracle(oracle, name):
    """One cell of a satisfied witness changed: the restatement accepts iff the oracle's verifier accepts the oracle's proof of it.
    Within a gate's width every cell is constrained; past it (advice columns, in no copy) none is.  PoseidonGate (135 of 135 wires) and
    U32RangeCheckGate with 8 limbs (136 of 136) leave no column unused: only the rejecting verdict is reachable there.  The judge proves
    under the Keccak hasher (the verdict does not depend on the hasher and its proofs are the quicker ones)."""
    desc = CAMPAIGN[name]()
    d = copy.copy(desc)
    d.proof_of_work_bits, d.hasher, d.circuit_digest = 0, 1, None
    oc = oracle.OracleCircuit(d)
    sm = wr.decode_sigmas(desc)
    verdicts = {}
    for gi, r, c in _cells(desc):
        W = desc.wires.copy()
        W[c, r] = (int(W[c, r]) + 1) % P
        rc, proof = oc.prove(wires=W)
        assert rc == 0
        accepted = oc.verify(proof) == 0
        rep, by_gate = wr.check(desc, W, sigma_map=sm)
        clean = wr.as_tuple(rep)[:3] == (0, 0, 0)
        assert clean == accepted, "gate %d row %d column %d: oracle %s, restatement %s" % (gi, r, c, accepted, rep)
        if not clean and c >= desc.num_routed_wires:
            assert (rep["failed_rows"], rep["row"], rep["gate"], rep["failed_copies"]) == (1, r, gi, 0)
        verdicts.setdefault(gi, set()).add(accepted)
    for gi, seen in verdicts.items():
        g = desc.gates[gi]
        want = {True, False} if gate_width(g) < desc.num_wires else {False}
        assert seen == want, (int(g["type"]), seen)


def test_campaign_covers_the_ten_types():
    seen = {int(g["type"]) for f in CAMPAIGN.values() for g in f().gates}
    assert set(lg.LIMB_GATES) <= seen
