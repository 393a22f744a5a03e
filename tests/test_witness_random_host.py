"""Random cells in the planner of witness generation (csrc/witness_plan.h; include/glp.h, RANDOM CELLS), device-free: the host program
csrc/examples/witness_plan_host.cpp, built with -fsanitize=address,undefined and run directly as tests/test_witness_plan_host.py does,
with the random list as the optional last line of its input, compared list by list with tests/witness_random_restate.py.

A random cell is a wave-0 source exactly as an input cell is, so every list must be the list of the restated plan over inputs + random
cells, the `inputs` and `random` lists the caller's own, in the caller's order.  refusals() holds the regular expressions of the new
refusals; tests/test_gpu_witness_random.py reuses them through the C ABI, prefixed with the entry point's name."""
import functools
import re
import subprocess

import numpy as np
import pytest

from plonky2_lib_amd import synth
import witness_plan_restate as wp
import witness_random_restate as rr
from test_witness_plan_host import SRC, RECORDS, INFO, FREE_INFO, compare, view_of
from test_witness_plan_restate import planned


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("witness_random") / "witness_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


def plan_host(program, v, inputs, random, null_random=False):
    """Run the stages on a request of gate units only -> the lists as a dict (records as tuples), or the message of a refusal.
    random: None = the input ends where it ended before there were random cells."""
    num = lambda xs: " ".join(str(int(x)) for x in xs)
    text = [num([v.lg, v.nw, v.nr, len(v.gates)])] + [num(g) for g in v.gates] + [num(v.row_gate), num(v.pos), str(32 if null_random else 0)]
    text += [num([len(inputs)] + list(inputs)), "0", "0 0", "0", "0 0"]
    if random is not None:
        text.append(num([len(random)] + list(random)))
    r = subprocess.run([program], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode in (0, 3) and not r.stderr, (r.returncode, r.stderr[-3000:])        # the sanitizers find nothing
    if r.returncode == 3:
        tag, code, message = r.stdout.strip().split(" ", 2)
        assert (tag, code) == ("refused", "-1")                   # GLP_ERR_ARG
        return message
    out = {}
    for ln in r.stdout.splitlines():
        name, *vals = ln.split()
        vals = [int(x) for x in vals]
        k = RECORDS.get(name)
        out[name] = vals if k is None else [tuple(vals[i:i + k]) for i in range(0, len(vals), k)]
    out["info"], out["free_info"], out["prog_lds"] = dict(zip(INFO, out["info"])), dict(zip(FREE_INFO, out["free_info"])), out["prog_lds"][0]
    return out


@functools.lru_cache(maxsize=None)
def noop_circuit():
    """2^6 rows of NoopGate by 80 wires, nothing routed: every cell is a class of its own"""
    cfg = synth.Config(80, 80)
    cfg.proof_of_work_bits = 0
    return synth.Builder(cfg, 6, seed=0, random_from_row=64).build()


def scattered(count, cells=80 * 64, skip=()):
    """`count` distinct cells all over the trace, not sorted: the stride 3063 is coprime to 5120 = 2^10 * 5"""
    out = [(11 + 3 * i * 1021) % cells for i in range(count + len(skip))]
    out = [p for p in out if p not in set(skip)][:count]
    assert len(set(out)) == count == len(out) and (count < 3 or out != sorted(out))
    return out


def moved_zkdsa3():
    """zkdsa3 with two of its eight inputs moved to the random list, out of order -> (view, classes, inputs, random, restated plan)"""
    desc, cls, ins, _ = planned("zkdsa3")
    rnd = [ins[6], ins[1]]
    rest = [p for p in ins if p not in rnd]
    return desc, cls, rest, rnd, rr.plan(desc, rest, rnd, cls=cls)


# ---------------------------------------------------------------------------------------------------- lists
def test_lists_with_inputs_moved_to_the_random_list(program):
    desc, cls, ins, rnd, pl = moved_zkdsa3()
    v = view_of(desc)
    out = plan_host(program, v, ins, rnd)
    compare(out, v, pl, ins)                                     # inputs (the caller's order), copies by destination, cell_waves, info, units
    assert out["random"] == rnd
    base = planned("zkdsa3")[3]
    assert out["info"] == {k: (0 if x is None else x) for k, x in base.info.items()}         # the plan of all eight as inputs: the rule is the same
    assert out["info"]["num_stuck_units"] == 0
    assert all(out["cell_waves"][p] == 0 for p in rnd)
    # the copies of wave 0 carry a random value to the rest of its class
    co = out["copy_off"]
    for p in rnd:
        others = sorted(int(q) for q in np.nonzero(cls == cls[p])[0] if q != p)
        assert others and [(s, d) for s, d in out["copies"][co[0]:co[1]] if s == p] == [(p, q) for q in others]


@pytest.mark.parametrize("count", [1, 7, 8, 9, 8 * 256 + 3])
def test_lists_of_scattered_random_cells(program, count):
    desc = noop_circuit()
    v = view_of(desc)
    ins = [5, 64 * 80 - 1, 1000]
    rnd = scattered(count, skip=ins)
    pl = rr.plan(desc, ins, rnd, cls=np.arange(v.cells, dtype=np.int64))
    out = plan_host(program, v, ins, rnd)
    compare(out, v, pl, ins)
    assert out["random"] == rnd
    assert out["info"]["num_cells_known"] == count + 3 and out["copies"] == [] and out["units"] == []
    waves = np.array(out["cell_waves"])
    assert (waves[rnd] == 0).all() and (waves[ins] == 0).all() and (waves == -1).sum() == v.cells - count - 3


def test_input_without_the_random_line_is_read_as_before(program):
    desc, cls, ins, pl = planned("zkdsa3")
    v = view_of(desc)
    old, empty = plan_host(program, v, ins, None), plan_host(program, v, ins, [])
    compare(old, v, pl, ins)
    assert old["random"] == [] and old == empty


# ---------------------------------------------------------------------------------------------------- source ties
def test_a_random_cell_is_the_source_of_its_class(program):
    """One ArithmeticGate row whose operation 0 (reads wires 0..2, writes wire 3: a unit of wave 1) has its output, position 3 n + 0,
    copy-constrained to (row 1, wire 4), position 4 n + 1, a random cell.  The class has wave 0 and its source is the random cell,
    although the unit's output lies at the smaller position: the copy of wave 0 overwrites nothing the unit needs, and the unit's own
    value lands in its cell in wave 1 (glp_witness_check reports the broken copy if the two disagree)."""
    cfg = synth.Config(80, 80)
    b = synth.Builder(cfg, 3, seed=0, random_from_row=8)
    b.set_rows(np.array([0]), synth.GATE_ARITHMETIC, 20)
    b.connect_pairs(np.array([0]), 3, np.array([1]), 4)
    desc = b.build()
    n = 8
    v = view_of(desc)
    out_cell, rnd_cell = 3 * n + 0, 4 * n + 1
    ins = [0 * n, 1 * n, 2 * n]
    cls = wp.classes(desc)
    assert cls[rnd_cell] == cls[out_cell] == out_cell < rnd_cell
    pl = rr.plan(desc, ins, [rnd_cell], cls=cls)
    out = plan_host(program, v, ins, [rnd_cell])
    compare(out, v, pl, ins)
    co = out["copy_off"]
    assert out["copies"][co[0]:co[1]] == [(rnd_cell, out_cell)] and len(out["copies"]) == 1
    assert out["cell_waves"][rnd_cell] == 0 and out["cell_waves"][out_cell] == 1
    assert any(r == 0 and gu & 0xFFFF == 0 for r, gu in out["units"])              # the unit still runs
    # the same cell as an input: the same lists (ties go to the smallest flat position with inputs and random cells alike)
    as_input = plan_host(program, v, ins + [rnd_cell], [])
    assert as_input["copies"] == out["copies"] and as_input["cell_waves"] == out["cell_waves"] and as_input["info"] == out["info"]


# ---------------------------------------------------------------------------------------------------- refusals
def refusals():
    """[(regular expression, input cells, random cells, random_cells handed over as a null pointer)] on zkdsa3; the entry point's
    name and ": " stand in front of each message"""
    desc, cls, ins, _ = planned("zkdsa3")
    n, nw = 1 << int(desc.degree_bits), int(desc.num_wires)
    sk0, twin = 0 * n + 1, 4 * n + 1                            # (row 1, col 4) carries the private key word of (row 1, col 0)
    assert cls[twin] == cls[sk0] == sk0 and sk0 in ins
    rest = [p for p in ins if p != sk0]
    free = [70 * n + 6, 71 * n + 7, 72 * n + 5]                  # cells of no class but their own
    return [
        (r"random_cells is null, num_random = 2", ins, free[:2], True),
        (r"random_cells\[1\] = %d is out of range \(num_wires \* 2\^degree_bits = %d cells\)" % (nw * n, nw * n), ins, [free[0], nw * n], False),
        (r"random_cells\[2\] = %d is listed twice \(also random_cells\[0\]\)" % free[0], ins, [free[0], free[1], free[0]], False),
        (r"random_cells\[1\] = %d is also input_cells\[%d\]" % (ins[5], 5), ins, [free[0], ins[5]], False),
        (r"random_cells\[1\] = %d and random_cells\[2\] = %d lie in one copy class" % (sk0, twin), rest, [free[0], sk0, twin], False),
        (r"random_cells\[1\] = %d and input_cells\[%d\] = %d lie in one copy class" % (twin, ins.index(sk0), sk0), ins, [free[0], twin], False),
    ]



def test_refusals(program):
    v = view_of(planned("zkdsa3")[0])
    for match, ins, rnd, null in refusals():
        out = plan_host(program, v, ins, rnd, null_random=null)
        assert isinstance(out, str), "not refused: " + match
        assert re.search(match, out), (match, out)
        assert out.startswith("witness_plan_host: ")
    # the input cells are judged first, and a good request with the same cells is taken
    assert re.search(r"input_cells\[0\] = %d is out of range" % v.cells, plan_host(program, v, [v.cells], [v.cells]))
    assert isinstance(plan_host(program, v, refusals()[0][1], refusals()[0][2]), dict)
