"""tests/witness_fill_restate.py (the 20 row-local generators and the column roles) pinned on the CPU: against the oracle's generators
(gate types up to 14) on scrambled witnesses of the five families, against the builder's own witnesses for the extension-field and
recursion gates (types 15-22, which the oracle's generators do not cover), and against the role tables of the GPU tests.  No GPU."""
import numpy as np
import pytest

import plonky2_lib_amd.synth as synth
import witness_fill_restate as wf
import zeta_identity_recursion as zr
from test_oracle_witness import FAMILIES, scramble_derived
from test_recursion_gates import PARAMS

REC = synth.Config.standard_recursion_config
LATE = {
    "ext": lambda: synth.ext_gates_circuit(5, seed=31),
    "ext-ecc": lambda: synth.ext_gates_circuit(4, synth.Config.standard_ecc_config(), seed=32),
    "recursion-default": lambda: synth.recursion_gates_circuit(4, REC(), seed=31, params=PARAMS["default"], mix_ext=True),
    "recursion-odd": lambda: synth.recursion_gates_circuit(4, REC(), seed=31, params=PARAMS["odd"], mix_ext=True),
}


@pytest.mark.parametrize("only_advice", [False, True])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_equals_the_oracle_generators(oracle, family, only_advice):
    desc = FAMILIES[family]()
    oc = oracle.OracleCircuit(desc)
    w, touched = scramble_derived(desc, np.random.default_rng(23), only_advice=only_advice)
    assert touched.any()
    got, ref = wf.fill(desc, w, only_advice), oc.witness_fill(w, only_advice=only_advice)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, "first mismatch at (column, row) %s" % bad[0].tolist()
    assert (got != w).any()
    if only_advice:
        assert (got[:desc.num_routed_wires] == w[:desc.num_routed_wires]).all()


@pytest.mark.parametrize("name", sorted(LATE))
def test_rebuilds_the_builder_witness_of_the_late_types(name):
    desc = LATE[name]()
    erased = desc.wires.copy()
    seen = set()
    for gi, g in enumerate(desc.gates):
        role = np.array(wf.roles(g, desc.num_wires))
        rows = zr.gate_rows(desc, gi)
        if len(rows) and (role == 1).any():
            erased[np.ix_(role == 1, rows)] = 0x1234567
            seen.add(int(g["type"]))
    assert seen >= (set(synth.EXT_GATES) if name.startswith("ext") else set(synth.EXT_GATES) | set(synth.RECURSION_GATES))
    assert (erased != desc.wires).any()
    got = wf.fill(desc, erased)
    bad = np.argwhere(got != desc.wires)
    assert bad.size == 0, "first mismatch at (column, row) %s" % bad[0].tolist()
    # only_advice: the routed outputs stay erased, every advice output is back
    nr = desc.num_routed_wires
    adv = wf.fill(desc, erased, only_advice=True)
    assert (adv[:nr] == erased[:nr]).all() and (adv[nr:] == desc.wires[nr:]).all()


def test_roles_equal_the_existing_tables():
    from test_gpu_ext_gates import _expected_roles as ext_roles
    from test_gpu_recursion_gates import _expected_roles as rec_roles
    seen = set()
    for name in sorted(LATE):
        desc = LATE[name]()
        for g in desc.gates:
            t = int(g["type"])
            if t in synth.EXT_GATES:
                want = ext_roles(t, int(g["p0"]), desc.num_wires)
            elif t in synth.RECURSION_GATES:
                want = rec_roles(t, g, desc.num_wires)
            else:
                continue
            assert wf.roles(g, desc.num_wires) == [int(x) for x in want], (name, t)
            seen.add(t)
    assert seen == set(synth.EXT_GATES) | set(synth.RECURSION_GATES)


def test_roles_of_the_early_types_are_inputs_and_everything_written():
    """types up to 14: role 2 = the generator inputs test_oracle_witness.py lists; role 1 = exactly the cells a fill changes when every
    non-input cell of the row starts scrambled"""
    from test_oracle_witness import generator_inputs
    for family in sorted(FAMILIES):
        desc = FAMILIES[family]()
        w, _ = scramble_derived(desc, np.random.default_rng(29))
        got = wf.fill(desc, w)
        for gi, g in enumerate(desc.gates):
            role = np.array(wf.roles(g, desc.num_wires))
            ins = generator_inputs(g, desc)
            assert sorted(np.nonzero(role == 2)[0].tolist()) == sorted(ins or [])
            rows = zr.gate_rows(desc, gi)
            if len(rows):
                changed = (got != w)[:, rows].any(axis=1)
                assert not (changed & (role != 1)).any(), (family, int(g["type"]))
                assert (got[np.ix_(role == 1, rows)] == desc.wires[np.ix_(role == 1, rows)]).all()
