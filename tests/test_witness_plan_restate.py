"""tests/witness_plan_restate.py pinned on the CPU: the unit tables against witness_fill_restate.roles, the planner's figures on the
project's synthetic circuits (one input cell per copy class that some unit reads and no unit writes), regeneration of the builder's
witness from those inputs alone, and the stuck rule against a closure computed another way."""
import numpy as np
import pytest

from plonky2_lib_amd import synth
import witness_check_restate as wcr
import witness_fill_restate as wfr
import witness_plan_restate as wp

# circuit -> (units, input cells, waves, widest wave in units)
CIRCUITS = {
    "zkdsa3": (lambda: synth.zkdsa_circuit(3), (5, 8, 4, 2)),
    "poseidon-chain2": (lambda: synth.poseidon_chain_circuit(2), (2, 8, 2, 1)),
    "poseidon-chain6": (lambda: synth.poseidon_chain_circuit(6), (62, 248, 62, 1)),
    "arith3": (lambda: synth.arith_circuit(3, num_const_rows=2, num_noop_rows=1), (82, 161, 20, 6)),
    "arith8": (lambda: synth.arith_circuit(8), (4964, 9917, 21, 248)),
    "ext3": (lambda: synth.ext_gates_circuit(3), (28, 226, 23, 5)),
    "recursion3": (lambda: synth.recursion_gates_circuit(3), (16, 101, 4, 13)),
    "u32-6": (lambda: synth.u32_circuit(6), (1042, 2061, 20, 73)),
    "ecdsa5": (lambda: synth.ecdsa_shape_circuit(5), (262, 649, 21, 68)),
    "keccak5": (lambda: synth.keccak_shape_circuit(5), (286, 585, 21, 54)),
    "smt4": (lambda: synth.smt_shape_circuit(4), (108, 223, 20, 9)),
}
_cache = {}


def planned(name):
    """(desc, classes, inputs, plan) of a circuit, made once and left unchanged"""
    if name not in _cache:
        desc = CIRCUITS[name][0]()
        cls = wp.classes(desc)
        ins = wp.default_inputs(desc, cls)
        _cache[name] = (desc, cls, ins, wp.plan(desc, ins, cls))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_unit_tables(name):
    desc = planned(name)[0]
    nw = int(desc.num_wires)
    for g in desc.gates:
        us = wp.units(g, nw)
        union = [0] * nw
        for u in range(len(us)):
            role = wp.unit_roles(g, nw, u)
            for c in range(nw):
                if role[c] == 1:
                    assert union[c] != 1, "column %d written by two units" % c
                    union[c] = 1
                elif role[c] == 2 and union[c] == 0:
                    union[c] = 2
        assert union == wfr.roles(g, nw)


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_table_figures_and_regeneration(name):
    desc, cls, ins, pl = planned(name)
    info = pl.info
    assert (info["num_units"], len(ins), info["num_waves"], info["widest_wave_units"]) == CIRCUITS[name][1]
    assert info["num_stuck_units"] == 0 and pl.stuck == []
    flat = desc.wires.reshape(-1)
    W = wp.generate(pl, [flat[p] for p in ins], np.zeros_like(desc.wires))
    known = pl.cell_waves >= 0
    assert info["num_cells_known"] == known.sum()
    assert (W[known] == desc.wires[known]).all() and not W[~known].any()
    rep, by_gate = wcr.check(desc, W)
    assert wcr.as_tuple(rep)[:3] == (0, 0, 0) and not any(by_gate)
    # poison instead of zeros: the unknown cells keep it
    W2 = wp.generate(pl, [flat[p] for p in ins], np.full_like(desc.wires, 12345))
    assert (W2[known] == desc.wires[known]).all() and (W2[~known] == 12345).all()


def _predicted_stuck(desc, cls, ins):
    """the stuck units by closure from the unknown classes: a unit reading an unknown class is stuck, a class without an input whose
    every writer is stuck is unknown"""
    us = wp.all_units(desc)
    have = {int(cls[p]) for p in ins}
    writers = {}
    for k, u in enumerate(us):
        for p in u[4]:
            writers.setdefault(int(cls[p]), set()).add(k)
    unknown = {int(cls[p]) for u in us for p in u[3]} - have - set(writers)
    stuck = set()
    while True:
        more = {k for k, u in enumerate(us) if k not in stuck and any(int(cls[p]) in unknown for p in u[3])}
        if not more:
            break
        stuck |= more
        unknown |= {c for c, ws in writers.items() if c not in have and ws <= stuck}
    return [(us[k][0], us[k][1], us[k][2]) for k in sorted(stuck)]


@pytest.mark.parametrize("name,drop", [("zkdsa3", 0), ("zkdsa3", 5), ("poseidon-chain6", 3), ("arith3", 40), ("u32-6", 700), ("ext3", 100),
                                       ("smt4", 17)])
def test_dropping_an_input_sticks_the_predicted_units(name, drop):
    desc, cls, ins, _ = planned(name)
    fewer = ins[:drop] + ins[drop + 1:]
    pl = wp.plan(desc, fewer, cls)
    want = _predicted_stuck(desc, cls, fewer)
    assert want and pl.stuck == want
    assert pl.info["num_stuck_units"] == len(want)
    assert (pl.info["stuck_row"], pl.info["stuck_gate"], pl.info["stuck_unit"]) == want[0]
    n = 1 << int(desc.degree_bits)
    stuck = set(want)
    for u in pl.units:                       # what a stuck unit would write is known only through its class, if at all
        if (u[0], u[1], u[2]) in stuck:
            assert all(pl.cell_waves[p // n, p % n] == pl.class_wave.get(int(cls[p]), -1) for p in u[4])
    assert any(pl.cell_waves[p // n, p % n] == -1 for u in pl.units if (u[0], u[1], u[2]) in stuck for p in u[4])


def test_an_input_may_share_a_class_with_an_output():
    """a public-key cell of zkdsa listed as an input as well: the class is known at wave 0 and the unit still runs"""
    desc, cls, ins, base = planned("zkdsa3")
    written = sorted({int(cls[p]) for u in base.units for p in u[4] if (cls == cls[p]).sum() > 1})
    pl = wp.plan(desc, ins + [written[0]], cls)
    assert pl.info["num_stuck_units"] == 0 and pl.class_wave[written[0]] == 0
    flat = desc.wires.reshape(-1)
    W = wp.generate(pl, [flat[p] for p in ins + [written[0]]], np.zeros_like(desc.wires))
    known = pl.cell_waves >= 0
    assert (W[known] == desc.wires[known]).all()
