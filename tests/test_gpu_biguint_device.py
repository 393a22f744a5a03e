"""csrc/biguint_dev.h as the GPU runs it: the two device functions of witness.hip that hold the limb arithmetic of the free units --
witness_free_unit8 (every count a compile-time 8, unrolled into registers) and witness_free_unit_any (run-time counts, arrays in
scratch) -- on the vectors of tests/biguint_device_vectors.py, which tests/test_biguint_device_vectors.py shows to reach both digit
corrections and the add-back of the division in each instance, at normalisation shifts 0, 31 and between, with operands above the
modulus, every modulus length from 1 to 8 limbs, results truncated and padded, and the inverse where there is none.

Every shape of the set is one free unit placed by hand on cells of its own in a trace of NoopGate rows, which nothing constrains
(as tests/test_witness_free_restate.multi_add places its units); its input cells are inputs of the plan.  K proofs are generated in
lock step, proof k carrying value set k of every shape, in both schedules, into a buffer filled with a sentinel.  Then every cell of
every proof is compared: output cells with witness_free_restate.run_free (Python integers), input cells with what was sent, and every
other cell -- the unplaced outputs among them -- must still hold the sentinel."""
import functools

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import synth
import biguint_device_vectors as V
import witness_free_restate as fr

pytestmark = pytest.mark.gpu

ENV = "GLP_WITNESS_NARROW_MAX"
FORMS = ("0", str(1 << 31))                 # every wave wide; every wave walked
FILL = 0x0BADC0DE0BADC0DE                   # what the buffer holds before a generation: no limb, and no input of the set
LOG_ROWS, WIRES = 9, 80


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def noop_circuit():
    cfg = synth.Config(WIRES, WIRES)
    cfg.proof_of_work_bits = 0
    return synth.Builder(cfg, LOG_ROWS, seed=0, random_from_row=1 << LOG_ROWS).build()


@pytest.fixture(scope="module")
def circuit(ctx):
    gc = glp.Circuit(ctx, noop_circuit())
    yield gc
    gc.free()


@functools.lru_cache(maxsize=None)
def placed(all8):
    """the shapes of one instance as a plan over the NoopGate trace -> (shapes, units, cells, moduli, input cells, input values
    [K][num_inputs], expected buffers [K][num_cells], restated plan, what each cell is)"""
    c = noop_circuit()
    num_cells = WIRES << LOG_ROWS
    index = [i for i, sh in enumerate(V.shapes()) if sh.all8 == all8]
    shs, want = [V.shapes()[i] for i in index], [V.expected()[i] for i in index]
    units, cells, moduli, free, ins, outs = V.place(shs, num_cells)
    inputs = [p for cin in ins for p in cin]
    values = np.array([[v for sh in shs for v in sh.sets[k]] for k in range(V.K)], np.uint64)
    buf = np.full((V.K, num_cells), FILL, np.uint64)
    buf[:, inputs] = values
    what = {}
    for i, (sh, cin, cout) in enumerate(zip(shs, ins, outs)):
        for j, p in enumerate(cin):
            what[p] = (i, "input", j)
        for j, p in cout:
            what[p] = (i, "output", j)
            buf[:, p] = [want[i][k][j] for k in range(V.K)]
    assert len(what) == len(inputs) + sum(len(o) for o in outs) < num_cells // 2          # disjoint runs; most cells are no unit's
    assert not (values == FILL).any()
    pl = fr.plan(c, inputs, free, np.arange(num_cells, dtype=np.int64))
    return shs, units, cells, moduli, inputs, values, buf, pl, what


def _first_difference(shs, what, got, want, form):
    k, p = (int(x[0]) for x in np.nonzero(got != want))
    if p in what:
        i, role, j = what[p]
        where = "%s cell %d of shape %d (%r), inputs %s" % (role, j, i, shs[i], [hex(v) for v in shs[i].sets[k]])
    else:
        where = "a cell of no unit"
    return "form %s, proof %d, cell %d = %#x, expected %#x: %s; %d cells differ in all" % (form, k, p, int(got[k, p]), int(want[k, p]), where, (got != want).sum())


@pytest.mark.parametrize("all8", [True, False], ids=["all8", "any"])
def test_instance_on_every_vector(ctx, circuit, all8, monkeypatch):
    shs, units, cells, moduli, inputs, values, want, pl, what = placed(all8)
    assert 16 <= V.K <= 32 and all(sh.all8 == all8 for sh in shs)
    assert pl.free_info == dict(num_free_units=len(shs), num_stuck_free_units=0, first_stuck_free_unit=None, widest_wave_free_units=len(shs)) and pl.num_waves == 1
    # units are independent: whatever the planner refuses, it refuses here, before any launch
    plans = {}
    for form in FORMS:
        monkeypatch.setenv(ENV, form)
        plans[form] = circuit.witness_plan(inputs, free_units=(units, cells), moduli=moduli)
    for form in FORMS:
        monkeypatch.setenv(ENV, form)
        plan = plans[form]
        assert plan.info == pl.info and plan.free_info == pl.free_info
        assert (plan.cell_waves() == pl.cell_waves).all()
        W = np.full(want.shape, FILL, np.uint64)
        ptr = ctx.dev_alloc(W.nbytes)
        ctx.dev_upload(ptr, W)
        plan.generate(ptr, values, V.K)
        ctx.dev_download(ptr, W)
        ctx.dev_free(ptr)
        assert (W == want).all(), _first_difference(shs, what, W, want, form)
        plan.free()
