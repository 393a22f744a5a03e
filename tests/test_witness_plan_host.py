"""csrc/witness_plan.h -- the planner of witness generation, every index the wave kernels use unchecked -- compiled into a plain host
program (csrc/examples/witness_plan_host.cpp, built with -fsanitize=address,undefined and run directly) and compared, list by list, with
tests/witness_plan_restate.py and tests/witness_free_restate.py, which share no code with csrc/.  The gate of every row comes from
witness_plan_restate.row_gates and the decoded permutation from witness_check_restate.decode_sigmas: no device is involved.

What the GPU tests cannot see is pinned here: the order of every list (units of a wave by (row, unit), copies by destination, free
units in the caller's order, program units by (wave, program) in chunks of at most 64), the wave offsets as running counts, and every
index below its bound.  The refusals of the stages are matched with the regular expressions of the GPU tests (without the entry
point's name: the program's is witness_plan_host)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import witness_check_restate as wcr
import witness_free_restate as fr
import witness_plan_restate as wp
import test_witness_free_restate as tfr
from test_witness_plan_restate import CIRCUITS, planned

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(HERE, "plonky2-lib_amd", "csrc", "examples", "witness_plan_host.cpp")
NONE = 0xFFFFFFFF
NO_CELL = fr.NO_CELL
NOOP, ARITHMETIC, PROGRAM = 0, 3, 9            # GLP_GATE_NOOP, GLP_GATE_ARITHMETIC; GLP_WGEN_PROGRAM
INFO = ("num_waves", "num_units", "num_stuck_units", "num_copies", "num_cells_known", "widest_wave_units", "stuck_row", "stuck_gate", "stuck_unit")
FREE_INFO = ("num_free_units", "num_stuck_free_units", "first_stuck_free_unit", "widest_wave_free_units")
RECORDS = {"units": 2, "copies": 2, "free_units": 9, "prog_units": 9, "prog_chunks": 3, "prog_tab": 4}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("witness_plan") / "witness_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


class View:
    """the circuit as the planner sees it"""

    def __init__(self, lg, nw, nr, gates, row_gate, pos):
        self.lg, self.nw, self.nr, self.gates, self.row_gate, self.pos = lg, nw, nr, [tuple(int(x) for x in g) for g in gates], row_gate, pos
        self.n, self.cells = 1 << lg, nw << lg


def view_of(desc):
    lg, nw, nr = int(desc.degree_bits), int(desc.num_wires), int(desc.num_routed_wires)
    n = 1 << lg
    pos = np.zeros(nr * n, np.int64)
    for (j, i), (j2, i2) in wcr.decode_sigmas(desc).items():
        pos[j * n + i] = j2 * n + i2
    return View(lg, nw, nr, [(g["type"], g["p0"], g["p1"]) for g in desc.gates], wp.row_gates(desc), pos)


@functools.lru_cache(maxsize=None)
def circuit_view(name):
    return view_of(planned(name)[0])


@functools.lru_cache(maxsize=None)
def free_view(name):
    return view_of(tfr.multi_add()[0] if name == "multi_add" else tfr.planned(name)[0])


def noop_view(lg=6, nw=80):
    """2^lg rows of one NoopGate, nothing routed: every cell is a class of its own"""
    return View(lg, nw, 0, [(NOOP, 0, 0)], np.zeros(1 << lg, np.int64), np.zeros(0, np.int64))


def plan_host(program, v, inputs, units=(), cells=(), moduli=(), programs=None, null_mask=0, num_cells=None):
    """Run the stages on one request -> the lists as a dict of int lists (records as tuples), or the message of a refusal as a str.
    programs: None = the entry points without programs, else [(num_inputs, num_outputs, num_regs, num_instructions, num_pool)]."""
    num = lambda xs: " ".join(str(int(x)) for x in xs)
    units = [[int(x) for x in u] for u in np.asarray(units, np.int64).reshape(-1, 9)]
    moduli = np.asarray(moduli, np.int64).reshape(-1, 8)
    text = [num([v.lg, v.nw, v.nr, len(v.gates)])] + [num(g) for g in v.gates] + [num(v.row_gate), num(v.pos), str(null_mask)]
    text += [num([len(inputs)] + list(inputs)), str(len(units))] + [num(u) for u in units]
    text += [num([len(cells) if num_cells is None else num_cells, len(cells)] + list(cells)), num([len(moduli)] + list(moduli.reshape(-1)))]
    text += [num([0 if programs is None else 1, len(programs or ())])] + [num(p) for p in programs or ()]
    r = subprocess.run([program], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode in (0, 3) and not r.stderr, (r.returncode, r.stderr[-3000:])
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


def check_bounds(out, v, num_units, num_cells):
    """every index of every list is below its bound, and the offsets are running counts that end at the list's length"""
    W = out["info"]["num_waves"]
    for off, items in (("unit_off", "units"), ("copy_off", "copies"), ("free_off", "free_units"), ("prog_chunk_off", "prog_chunks")):
        o = out[off]
        if not o:
            assert not out[items]
            continue
        assert len(o) == W + 2 and o[0] == 0 and all(a <= b for a, b in zip(o, o[1:])) and o[-1] == len(out[items]), off
    assert out["unit_off"][1] == 0                                # wave 0 holds no unit
    per_gate = [len(wp.units(dict(type=t, p0=p0, p1=p1), v.nw)) for t, p0, p1 in v.gates]
    for row, gu in out["units"]:
        assert row < v.n and (gu >> 16) == v.row_gate[row] and (gu & 0xFFFF) < per_gate[gu >> 16]
    assert all(src < v.cells and dst < v.cells for src, dst in out["copies"])
    assert all(p < v.cells for p in out["inputs"]) and len(out["cell_waves"]) == v.cells
    assert len(out["free_cells"]) == num_cells and all(p < v.cells or p == NONE for p in out["free_cells"])
    for kind, modulus, cell_begin, *ln in out["free_units"] + out["prog_units"]:
        assert cell_begin + fr.num_in(kind, ln) + fr.num_out(kind, ln) <= num_cells if kind != PROGRAM else cell_begin + ln[0] + ln[1] <= num_cells
    assert all(first + count <= len(out["prog_units"]) and 1 <= count <= 64 and prog < len(out["prog_tab"]) for prog, first, count in out["prog_chunks"])
    assert all(co + cw == po and po <= len(out["prog_image"]) and cw % 4 == 0 for co, cw, po, _ in out["prog_tab"])


def compare(out, v, pl, ins, free_rows=(), free_cells=()):
    """the program's lists against a restated plan (witness_plan_restate.plan, or witness_free_restate.plan with free units)"""
    assert isinstance(out, dict), out
    free_rows = [[int(x) for x in u] for u in np.asarray(free_rows, np.int64).reshape(-1, 9)]
    check_bounds(out, v, len(free_rows), len(free_cells))
    zero = lambda d: {k: 0 if x is None else int(x) for k, x in d.items()}          # the restatement says None where the library leaves 0
    assert out["info"] == zero(pl.info)
    assert out["free_info"] == (zero(pl.free_info) if free_rows else dict.fromkeys(FREE_INFO, 0))
    assert (np.array(out["cell_waves"], np.int64).reshape(v.nw, v.n) == pl.cell_waves).all()
    assert out["inputs"] == [int(p) for p in ins]
    W, ng = pl.num_waves, len(pl.units)
    uo, co = out["unit_off"], out["copy_off"]
    for w in range(W + 1):
        want = [(r, gi << 16 | u) for k, (r, gi, u, _, _) in enumerate(pl.units) if pl.unit_wave[k] == w and w > 0]      # pl.units is in (row, unit) order
        assert out["units"][uo[w]:uo[w + 1]] == want, "units of wave %d" % w
        want = sorted(pl.copies.get(w, ()), key=lambda sd: sd[1])
        assert out["copies"][co[w]:co[w + 1]] == [(int(s), int(d)) for s, d in want], "copies of wave %d" % w
    assert set(pl.copies) <= set(range(W + 1))
    if free_rows:
        fo = out["free_off"]
        for w in range(W + 1):
            want = [tuple(free_rows[f]) for f in range(len(free_rows)) if pl.unit_wave[ng + f] == w and w > 0]           # the caller's order
            assert out["free_units"][fo[w]:fo[w + 1]] == want, "free units of wave %d" % w
        assert out["free_cells"] == [int(c) if int(c) < v.cells else NONE for c in free_cells]
    else:
        assert out["free_off"] == [] and out["free_units"] == []
    assert out["prog_chunk_off"] == [] and out["prog_units"] == [] and out["prog_image"] == [] and out["prog_lds"] == 0


# ---------------------------------------------------------------------------------------------------- gate units and copies
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_every_list_against_the_restatement(program, name):
    desc, cls, ins, pl = planned(name)
    out = plan_host(program, circuit_view(name), ins)
    compare(out, circuit_view(name), pl, ins)
    assert (out["info"]["num_units"], len(ins), out["info"]["num_waves"], out["info"]["widest_wave_units"]) == CIRCUITS[name][1]
    srcs = {}                                                    # every class has one source, and it is the restatement's
    for w, pairs in pl.copies.items():
        for s, d in pairs:
            srcs[int(cls[d])] = s
    assert all(srcs[int(cls[d])] == s and int(cls[s]) == int(cls[d]) for s, d in out["copies"])


def test_the_stuck_rule(program):
    desc, cls, ins, _ = planned("arith3")
    fewer = ins[:40] + ins[41:]
    pl = wp.plan(desc, fewer, cls)
    v = circuit_view("arith3")
    out = plan_host(program, v, fewer)
    compare(out, v, pl, fewer)
    listed = {(r, gu >> 16, gu & 0xFFFF) for r, gu in out["units"]}
    stuck = [(u[0], u[1], u[2]) for u in wp.all_units(desc) if (u[0], u[1], u[2]) not in listed]
    assert pl.stuck and stuck == pl.stuck and out["info"]["num_stuck_units"] == len(stuck)
    assert (out["info"]["stuck_row"], out["info"]["stuck_gate"], out["info"]["stuck_unit"]) == pl.stuck[0]


# ---------------------------------------------------------------------------------------------------- free units
@pytest.mark.parametrize("name", sorted(tfr.OPS) + ["curve_add", "double_then_conditional_add"])
def test_free_units(program, name):
    c, cls, ins, free, pl = tfr.planned(name)
    out = plan_host(program, free_view(name), ins, c.free_units, c.free_cells, c.moduli)
    compare(out, free_view(name), pl, ins, c.free_units, c.free_cells)
    assert out["free_info"]["num_free_units"] == len(free) > 0 and len(out["free_units"]) == len(free)


def test_multi_add_units(program):
    c, ins, free, pl, _ = tfr.multi_add()
    out = plan_host(program, free_view("multi_add"), ins, c.free_units, c.free_cells, c.moduli)
    compare(out, free_view("multi_add"), pl, ins, c.free_units, c.free_cells)
    assert out["free_info"]["widest_wave_free_units"] == 1 + len(tfr.MULTI_ADD_UNITS)


def test_an_output_that_is_not_placed_is_in_no_list(program):
    c, cls, ins, free, _ = tfr.planned("mul")
    v = free_view("mul")
    rows, cells = np.array(c.free_units, np.int64), np.array(c.free_cells, np.uint64)
    f = [int(k) for k in rows[:, 0]].index(fr.MUL)
    at = int(rows[f, 2]) + 16 + 15                               # the last limb of the overflow
    gone = int(cells[at])
    cells[at] = NO_CELL
    pl = fr.plan(c, ins, fr.from_arrays(rows, cells, c.moduli), cls)
    out = plan_host(program, v, ins, rows, cells, c.moduli)
    compare(out, v, pl, ins, rows, cells)
    assert out["free_cells"][at] == NONE and out["free_cells"].count(NONE) == 1
    assert out["cell_waves"][gone] == pl.class_wave.get(int(cls[gone]), -1)          # no unit writes that cell any more: it is known as its class is
    assert all(NONE not in pair and pair[0] != gone for pair in out["copies"]) and NONE not in out["inputs"]


def test_a_withheld_inverse_sticks_free_units(program):
    c, cls, ins, free, _ = tfr.planned("curve_add")
    inv = [i for i, f in enumerate(free) if f.kind == fr.INV]
    rows = np.delete(np.array(c.free_units, np.int64), inv, axis=0)
    pl = fr.plan(c, ins, free, cls, withhold=inv)
    out = plan_host(program, free_view("curve_add"), ins, rows, c.free_cells, c.moduli)
    compare(out, free_view("curve_add"), pl, ins, rows, c.free_cells)
    assert out["free_info"]["num_stuck_free_units"] == len(pl.stuck_free) > 0 and out["free_info"]["first_stuck_free_unit"] == pl.stuck_free[0]
    assert len(out["free_units"]) == len(rows) - len(pl.stuck_free)


# ---------------------------------------------------------------------------------------------------- program units
def test_program_units_in_chunks(program):
    """Two programs; 65 units of each, interleaved, are ready in wave 1, three read their outputs a wave later and one reads a cell
    nothing provides.  Per wave the units are sorted by program, in the caller's order within one, and cut into chunks of 64 at most."""
    v = noop_view()
    progs = [(1, 1, 3, 5, 3), (2, 1, 7, 7, 0)]                   # num_inputs, num_outputs, num_regs, num_instructions, num_pool
    cell = iter(range(0, v.cells, 3))
    rows, cells, inputs, a_out, b_out = [], [], [], [], []

    def unit(prog, cin, cout):
        rows.append([PROGRAM, prog, len(cells), len(cin), len(cout), 0, 0, 0, 0])
        cells.extend(cin + cout)
        return len(rows) - 1
    stuck = None
    for i in range(65):
        a_in, b_in = [next(cell)], [next(cell), next(cell)]
        a_out.append(next(cell))
        b_out.append(NO_CELL if i == 64 else next(cell))          # a target that was placed nowhere
        inputs += a_in + b_in
        unit(0, a_in, [a_out[-1]])
        if i == 3:
            nothing = next(cell)
            stuck = unit(0, [nothing], [next(cell)])
        unit(1, b_in, [b_out[-1]])
    later = [unit(1, [a_out[0], b_out[0]], [next(cell)]), unit(0, [a_out[1]], [next(cell)]), unit(1, [a_out[2], b_out[2]], [next(cell)])]
    out = plan_host(program, v, inputs, rows, cells, programs=progs)
    assert isinstance(out, dict), out
    check_bounds(out, v, len(rows), len(cells))
    assert out["info"] == dict(zip(INFO, (2, 0, 0, 0, len(inputs) + 130 - 1 + 3, 0, 0, 0, 0)))
    assert out["free_info"] == dict(num_free_units=134, num_stuck_free_units=1, first_stuck_free_unit=stuck, widest_wave_free_units=130)
    assert out["free_off"] == [] and out["free_units"] == [] and out["units"] == [] and out["copies"] == []      # program units are listed apart
    first = [f for f in range(len(rows)) if f != stuck and f not in later]
    order = [f for f in first if rows[f][1] == 0] + [f for f in first if rows[f][1] == 1] + [later[1], later[0], later[2]]
    assert out["prog_units"] == [tuple(rows[f]) for f in order] and stuck not in order
    assert out["prog_chunks"] == [(0, 0, 64), (0, 64, 1), (1, 65, 64), (1, 129, 1), (0, 130, 1), (1, 131, 2)]
    assert out["prog_chunk_off"] == [0, 0, 4, 6]
    # the image: per program its code, padded with zero words to a multiple of 4, then its pool
    code = lambda p, k: [p << 32 | i for i in range(k)]
    assert out["prog_tab"] == [(0, 8, 8, 1), (11, 8, 19, 2)]
    assert out["prog_image"] == code(0, 5) + [0] * 3 + [1 << 63 | i for i in range(3)] + code(1, 7) + [0]
    assert out["prog_lds"] == 7 * 64 * 8
    waves = out["cell_waves"]
    assert all(waves[p] == 0 for p in inputs) and all(waves[p] == 1 for p in a_out + b_out[:64])
    assert all(waves[cells[rows[f][2] + rows[f][3]]] == 2 for f in later)
    assert waves[nothing] == -1 and waves[cells[rows[stuck][2] + 1]] == -1 and waves.count(-1) == v.cells - out["info"]["num_cells_known"]
    assert out["free_cells"].count(NONE) == 1


# ---------------------------------------------------------------------------------------------------- refusals
def refused(program, match, *args, **kw):
    out = plan_host(program, *args, **kw)
    assert isinstance(out, str), "not refused: " + match
    assert re.search(match, out), (match, out)
    assert out.startswith("witness_plan_host: ")


def test_refusals_of_the_request(program):
    """stage 1, with the expressions of tests/test_gpu_witness_generate.py::test_refusals and test_size_refusals, and stage 4"""
    desc, cls, ins, _ = planned("zkdsa3")
    v = circuit_view("zkdsa3")
    n, nw = v.n, v.nw
    no = lambda match, inputs, view=v, **kw: refused(program, match, view, inputs, **kw)
    no("input_cells is null", ins, null_mask=1)
    three = [[fr.EQUALITY, 0, 0, 1, 1, 1, 1, 0, 0]] * 3
    no("units is null, num_units = 3", ins, units=three, cells=[0, 1, 2, 3], null_mask=2)
    no("cells is null, num_cells = 4", ins, units=three, cells=[0, 1, 2, 3], null_mask=4)
    no("moduli is null, num_moduli = 1", ins, moduli=[[7, 0, 0, 0, 0, 0, 0, 0]], null_mask=8)
    no("programs is null, num_programs = 1", ins, programs=[(1, 1, 1, 2, 1)], null_mask=16)
    bad = list(ins)
    bad[3] = nw * n
    no(r"input_cells\[3\] = %d is out of range" % (nw * n), bad)
    bad = list(ins)
    bad[5] = bad[2]
    no(r"input_cells\[5\] = %d is listed twice \(also input_cells\[2\]\)" % bad[2], bad)
    assert cls[4 * n + 1] == cls[0 * n + 1] == 0 * n + 1 and (0 * n + 1) in ins      # (row 1, col 4) carries the private key word of (row 1, col 0)
    no(r"input_cells\[%d\] = %d and input_cells\[8\] = %d lie in one copy class" % (ins.index(1), 1, 4 * n + 1), ins + [4 * n + 1])
    # 2^13 rows x (2^19 + 1) wires = 2^32 + 2^13 cells, and x 2^19 wires = 2^32 cells exactly: position 2^32 - 1 is not a cell either
    for wires in ((1 << 19) + 1, 1 << 19):
        no(r"num_wires \* 2\^degree_bits = %d positions, a plan addresses fewer than 2\^32" % (wires << 13), [0], view=noop_view(13, wires))
    small = noop_view(3, 4)
    many = View(3, 4, 0, [(NOOP, 0, 0)] * 65536, small.row_gate, small.pos)
    no(r"num_gates = 65536, a plan names at most 65535 gates", [0], view=many)
    no(r"num_cells = 4294967295, a plan addresses fewer than 2\^32 - 1", [0], view=small, cells=[0, 1], num_cells=NONE)
    no(r"moduli\[1\] is even", [0], view=small, moduli=[[5, 0, 0, 0, 0, 0, 0, 0], [6, 1, 0, 0, 0, 0, 0, 0]])
    no(r"moduli\[0\] = 1 is below 3", [0], view=small, moduli=[[1, 0, 0, 0, 0, 0, 0, 0]])
    # stage 3: the unit table's own bounds
    no(r"gate 0 has 65536 units per row, a plan names at most 65535", [0], view=View(3, 4, 0, [(ARITHMETIC, 65536, 0)], small.row_gate, small.pos))
    wide = View(17, 1, 0, [(ARITHMETIC, 65535, 0)], np.zeros(1 << 17, np.int64), small.pos)
    no(r"%d units exceed the 2\^32 - 1 a plan addresses" % (65535 << 17), [0], view=wide)
    # stage 4: a position of the decoded permutation outside the routed columns
    pos = np.array(v.pos)
    pos[5] = v.nr * n
    no(r"the decoded permutation leaves the routed columns", ins, view=View(v.lg, nw, v.nr, v.gates, v.row_gate, pos))


def test_refusals_of_free_units(program):
    """stages 2 and 3, with the expressions of tests/test_gpu_witness_free.py::test_refusals"""
    c, cls, ins, free, _ = tfr.planned("curve_add")
    v = free_view("curve_add")
    n, ncells = v.n, v.cells

    def no(match, rows=None, cells=None, moduli=None):
        refused(program, match, v, ins, c.free_units if rows is None else rows, c.free_cells if cells is None else cells, c.moduli if moduli is None else moduli)
    base = np.array(c.free_units, np.int64)
    kinds = [int(k) for k in base[:, 0]]
    i_mul, i_sub, i_inv = kinds.index(fr.MUL), kinds.index(fr.SUB), kinds.index(fr.INV)

    def edit(i, col, value):
        rows = base.copy()
        rows[i, col] = value
        return rows
    no(r"units\[%d\]\.kind = 9 is not a GLP_WGEN_\* kind" % i_mul, edit(i_mul, 0, 9))
    no(r"units\[%d\]\.kind = 0 is not a GLP_WGEN_\* kind" % i_mul, edit(i_mul, 0, 0))
    no(r"units\[0\]\.len\[1\] = 2, that operand of kind 1 is 1 cell", [[fr.EQUALITY, 0, 0, 1, 2, 1, 1, 0, 0]])
    no(r"units\[%d\]\.len\[3\] = 2, that operand of kind 4 is 1 cell" % i_sub, edit(i_sub, 3 + 3, 2))
    no(r"units\[%d\]\.len\[3\] = 1, kind 6 has 3 operands: unused entries are 0" % i_inv, edit(i_inv, 3 + 3, 1))
    no(r"units\[0\]\.len\[1\] = 5, GLV_SECP256K1 has k of 8 and k1, k2 of 4 limbs", [[fr.GLV, 0, 0, 8, 5, 4, 1, 1, 0]])
    no(r"units\[%d\]\.len\[0\] = 19, an operand has at most GLP_WGEN_MAX_LIMBS = 18 limbs" % i_mul, edit(i_mul, 3, 19))
    no(r"units\[0\]\.len\[1\] = 9, a divisor has at most 8 limbs", [[fr.DIV_REM, 0, 0, 12, 9, 4, 9, 0, 0]])
    no(r"units\[%d\]\.modulus = 1, num_moduli = 1" % i_mul, edit(i_mul, 1, 1))
    no(r"units\[%d\]\.modulus = 0, num_moduli = 0" % next(i for i, k in enumerate(kinds) if 2 <= k <= 6), moduli=np.zeros((0, 8), np.uint32))
    no(r"units\[0\]\.modulus = 1, kind 7 has no modulus: 0", [[fr.DIV_REM, 1, 0, 1, 1, 1, 1, 0, 0]])
    even = np.array(c.moduli, np.uint32)
    even[0, 0] &= 0xFFFFFFFE
    no(r"moduli\[0\] is even", moduli=even)
    no(r"moduli\[0\] = 1 is below 3", moduli=np.array([[1, 0, 0, 0, 0, 0, 0, 0]], np.uint32))
    cb = int(base[i_mul, 2])
    bad = np.array(c.free_cells, np.uint64)
    bad[cb + 3] = ncells
    no(r"units\[%d\]: cells\[%d\] = %d is out of range" % (i_mul, cb + 3, ncells), cells=bad)
    bad[cb + 3] = NO_CELL                                        # an input cell may not be left out
    no(r"units\[%d\]: cells\[%d\] = %d is out of range" % (i_mul, cb + 3, NO_CELL), cells=bad)
    no(r"units\[%d\]\.cell_begin = %d: its run of 32 cells leaves cells\[\] \(num_cells = %d\)" % (i_mul, c.free_cells.size - 31, c.free_cells.size),
       edit(i_mul, 2, c.free_cells.size - 31))
    rows = np.array(tfr.multi_add()[0].free_units[-1:], np.int64)             # the run of a MULTI_ADD unit is len[0] * len[1] + sum + overflow cells
    rows[0, 1:4] = 0, 0, 65535
    no(r"units\[0\]\.cell_begin = 0: its run of %d cells leaves cells\[\]" % (65535 * 2 + 9), rows)
    no(r"units\[%d\]: output cell \d+ is also written by units\[%d\]" % (len(base), i_inv), np.vstack([base, base[i_inv:i_inv + 1]]))
    # an output cell that a gate unit of its row writes too: the product's first limb moved onto the output of an arithmetic operation
    row, gate, unit, _, outs = next(u for u in wp.all_units(c) if int(c.gates[u[1]]["type"]) == ARITHMETIC)
    bad = np.array(c.free_cells, np.uint64)
    bad[cb + 16] = outs[0]
    no(r"units\[%d\]: output cell %d \(column %d, row %d\) is also written by unit %d of gate %d of that row" % (i_mul, outs[0], outs[0] // n, outs[0] % n, unit, gate),
       cells=bad)


def test_refusals_of_program_units(program):
    """stage 2, with the expressions of tests/test_gpu_witness_programs.py::test_plan_refusals"""
    v = noop_view()
    good = (1, 2, 4, 6, 2)
    cells = list(range(10))
    unit = [PROGRAM, 0, 0, 1, 2, 0, 0, 0, 0]

    def no(match, rows, programs=(good,), cells=cells):
        refused(program, match, v, [0], rows, cells, programs=None if programs is None else list(programs))
    assert isinstance(plan_host(program, v, [0], [unit], cells, programs=[good]), dict)
    no(r"units\[0\]\.modulus = 1, a program unit names its program there and num_programs = 1", [[9, 1, 0, 1, 2, 0, 0, 0, 0]])
    no(r"units\[1\]\.modulus = 0, a program unit names its program there and num_programs = 0", [[1, 0, 0, 1, 1, 1, 1, 0, 0], unit], programs=())
    no(r"units\[0\]\.len\[0\] = 2, programs\[0\] has num_inputs = 1", [[9, 0, 0, 2, 2, 0, 0, 0, 0]])
    no(r"units\[0\]\.len\[1\] = 3, programs\[0\] has num_outputs = 2", [[9, 0, 0, 1, 3, 0, 0, 0, 0]])
    no(r"units\[0\]\.len\[2\] = 1, a program unit has two operands: unused entries are 0", [[9, 0, 0, 1, 2, 1, 0, 0, 0]])
    no(r"units\[0\]\.len\[5\] = 7, a program unit has two operands", [[9, 0, 0, 1, 2, 0, 0, 0, 7]])
    # a program unit is a free unit: its run, its cells and its outputs are held to the same rules
    no(r"units\[0\]\.cell_begin = 8: its run of 3 cells leaves cells\[\] \(num_cells = 10\)", [[9, 0, 8, 1, 2, 0, 0, 0, 0]])
    no(r"units\[1\]: output cell 2 is also written by units\[0\]", [unit, [9, 0, 1, 1, 2, 0, 0, 0, 0]])
    no(r"units\[0\]: cells\[0\] = 18446744073709551615 is out of range", [unit], cells=[NO_CELL, 1, 2])
    # without programs kind 9 stays an unknown kind
    no(r"units\[0\]\.kind = 9 is not a GLP_WGEN_\* kind", [unit], programs=None)
