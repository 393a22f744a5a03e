"""glp_witness_plan_* / glp_witness_generate / glp_witness_read_cells on the GPU (include/glp.h, "witness generation, the dataflow
half") against tests/witness_plan_restate.py, which tests/test_witness_plan_restate.py pins first: unit tables, the plan's figures and
its whole cell_waves array, the generated values under both execution forms, lock step over 64 zkdsa witnesses from 8 words each, stuck
units, disagreeing sources and the refusals.

The two refusals that depend on the size of a witness are reached through the circuit description alone: glp_circuit_create bounds
degree_bits, not num_wires, and needs no wires array, so a small circuit's description with num_wires raised is past 2^32 cells (or past
the size cap at 4096 proofs) in milliseconds, and both are decided before the witness pointer is touched."""
import copy
import ctypes as C

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding, synth
import witness_plan_restate as wp
from test_witness_plan_restate import CIRCUITS, planned

pytestmark = pytest.mark.gpu

POISON = 0x0BADC0DE0BADC0DE                 # canonical
NARROW_DEFAULT = 256                        # GLP_WITNESS_NARROW_MAX as include/glp.h states it
ENV = "GLP_WITNESS_NARROW_MAX"
ALL_WALKED = str(1 << 31)


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _inputs(desc, ins, K=1):
    flat = desc.wires.reshape(-1)
    return np.tile(np.array([flat[p] for p in ins], np.uint64), (K, 1))


def _generate(ctx, plan, desc, inputs, K, zero_first, poison=POISON):
    """K poisoned buffers generated into -> (device pointer, the witnesses [K][num_wires][n])"""
    W = np.full((K,) + desc.wires.shape, poison, np.uint64)
    ptr = ctx.dev_alloc(W.nbytes)
    ctx.dev_upload(ptr, W)
    plan.generate(ptr, inputs, K, zero_first=zero_first)
    ctx.dev_download(ptr, W)
    return ptr, W


def _check_values(desc, pl, W, zero_first, want=None):
    known = pl.cell_waves >= 0
    want = desc.wires if want is None else want
    for k in range(W.shape[0]):
        assert (W[k][known] == want[known]).all(), "proof %d: %d known cells differ" % (k, (W[k][known] != want[known]).sum())
        assert (W[k][~known] == (0 if zero_first else POISON)).all(), "proof %d: a cell the plan never reaches was written" % k


# ---------------------------------------------------------------------------------------------------- unit tables, plan parity
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_unit_tables_and_plan_parity(ctx, name):
    desc, cls, ins, pl = planned(name)
    gc = glp.Circuit(ctx, desc)
    L = binding.load_library()
    nw = int(desc.num_wires)
    for gi, g in enumerate(desc.gates):
        table = gc.witness_units(gi)
        assert table.shape[0] == len(wp.units(g, nw)) == L.glp_witness_num_units(gc._h, gi)
        union = np.zeros(nw, np.uint8)
        for u in range(table.shape[0]):
            assert list(table[u]) == wp.unit_roles(g, nw, u)
            assert not ((union == 1) & (table[u] == 1)).any()
            union = np.where(table[u] == 1, 1, np.where((table[u] == 2) & (union == 0), 2, union)).astype(np.uint8)
        assert (union == gc.witness_columns(gi)).all()
    assert L.glp_witness_num_units(gc._h, len(desc.gates)) == 0
    plan = gc.witness_plan(ins)
    info = plan.info
    want = dict(pl.info)
    want["stuck_row"] = want["stuck_gate"] = want["stuck_unit"] = None
    assert info == want
    assert (info["num_units"], len(ins), info["num_waves"], info["widest_wave_units"]) == CIRCUITS[name][1]
    assert (plan.cell_waves() == pl.cell_waves).all()
    plan.free()
    gc.free()


# ---------------------------------------------------------------------------------------------------- values, both forms
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_values(ctx, name, monkeypatch):
    desc, cls, ins, pl = planned(name)
    gc = glp.Circuit(ctx, desc)
    flat = desc.wires.reshape(-1)
    ref = wp.generate(pl, [flat[p] for p in ins], np.zeros_like(desc.wires))
    known = pl.cell_waves >= 0
    assert (ref[known] == desc.wires[known]).all()            # the restatement regenerates the builder's witness
    for narrow in ("0", ALL_WALKED, None):
        if narrow is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, narrow)
        plan = gc.witness_plan(ins)
        for K in (1, 3):
            for zero_first in (False, True):
                ptr, W = _generate(ctx, plan, desc, _inputs(desc, ins, K), K, zero_first)
                _check_values(desc, pl, W, zero_first, ref)
                if zero_first:
                    reps = gc.check_witness(dev_wires_ptr=ptr, num_proofs=K, public_inputs=np.tile(desc.public_inputs, (K, 1)))
                    for rep in (reps if K > 1 else [reps]):
                        assert (rep.failed_constraints, rep.failed_rows, rep.failed_copies) == (0, 0, 0), str(rep)
                    if K == 1 and narrow is None:
                        assert gc.verify(gc.prove_device(ptr)), binding.load_library().glp_last_error()
                ctx.dev_free(ptr)
        plan.free()
    gc.free()


# ---------------------------------------------------------------------------------------------------- lock step
def test_lock_step_zkdsa(ctx):
    K = 64
    rng = np.random.default_rng(23)
    descs = [synth.zkdsa_circuit(3, private_key=synth.gl.rand(rng, 4), message=synth.gl.rand(rng, 4)) for _ in range(K)]
    desc, cls, ins, pl = planned("zkdsa3")
    assert len(ins) == 8
    gc = glp.Circuit(ctx, desc)
    plan = gc.witness_plan(ins)
    inputs = np.stack([d.wires.reshape(-1)[ins] for d in descs])
    ptr, W = _generate(ctx, plan, desc, inputs, K, True)
    known = pl.cell_waves >= 0
    host = np.stack([np.where(known, d.wires, 0) for d in descs]).astype(np.uint64)
    assert (W == host).all()
    n = 1 << int(desc.degree_bits)
    pi_cells = [(4 + i) * n + 2 for i in range(4)] + [(12 + i) * n + 1 for i in range(4)] + [(12 + i) * n + 2 for i in range(4)]   # message, public key, signature
    pis = gc.read_cells(ptr, pi_cells, K)
    assert (pis == np.stack([d.public_inputs for d in descs])).all()
    proofs = gc.prove_batch_device(ptr, K, pis)
    assert (proofs == gc.prove_batch(host, pis)).all()
    assert gc.verify_batch(proofs).all()
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ---------------------------------------------------------------------------------------------------- deep and narrow, wide
@pytest.mark.parametrize("log_n", [2, 6])
def test_deep_and_narrow(ctx, log_n, monkeypatch):
    """a Poseidon chain: one unit per wave, every wave walked by one launch"""
    monkeypatch.delenv(ENV, raising=False)
    name = "poseidon-chain%d" % log_n
    desc, cls, ins, pl = planned(name)
    gc = glp.Circuit(ctx, desc)
    plan = gc.witness_plan(ins)
    info = plan.info
    assert info["num_waves"] == CIRCUITS[name][1][2] and info["widest_wave_units"] == 1 <= NARROW_DEFAULT
    ptr, W = _generate(ctx, plan, desc, _inputs(desc, ins), 1, False)
    _check_values(desc, pl, W, False)
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


def test_wide(ctx, monkeypatch):
    """arith_circuit(11) at K = 1 under the default threshold: waves that span several workgroups, 20 ops chained inside each row"""
    monkeypatch.delenv(ENV, raising=False)
    desc = synth.arith_circuit(11)
    cls = wp.classes(desc)
    ins = wp.default_inputs(desc, cls)
    pl = wp.plan(desc, ins, cls)
    gc = glp.Circuit(ctx, desc)
    plan = gc.witness_plan(ins)
    info = plan.info
    assert info["widest_wave_units"] > NARROW_DEFAULT and info["widest_wave_units"] > 256        # the wide launches are really taken
    want = dict(pl.info)
    want["stuck_row"] = want["stuck_gate"] = want["stuck_unit"] = None
    assert info == want and (plan.cell_waves() == pl.cell_waves).all()
    for zero_first in (False, True):
        ptr, W = _generate(ctx, plan, desc, _inputs(desc, ins), 1, zero_first)
        _check_values(desc, pl, W, zero_first)
        if zero_first:
            rep = gc.check_witness(dev_wires_ptr=ptr)
            assert (rep.failed_constraints, rep.failed_rows, rep.failed_copies) == (0, 0, 0), str(rep)
        ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ---------------------------------------------------------------------------------------------------- stuck, disagreeing sources
def test_stuck(ctx):
    desc, cls, ins, _ = planned("zkdsa3")
    n = 1 << int(desc.degree_bits)
    drop = ins.index(0 * n + 3)                              # the first message word: the class of (row 2, col 4) and (row 3, col 0)
    fewer = ins[:drop] + ins[drop + 1:]
    pl = wp.plan(desc, fewer, cls)
    assert pl.info["num_stuck_units"] == 3                   # the signature and the two public-input hashes; the public key still runs
    gc = glp.Circuit(ctx, desc)
    plan = gc.witness_plan(fewer)
    assert plan.info == pl.info
    assert (plan.info["stuck_row"], plan.info["stuck_gate"], plan.info["stuck_unit"]) == pl.stuck[0]
    waves = plan.cell_waves()
    assert (waves == pl.cell_waves).all()
    ptr, W = _generate(ctx, plan, desc, _inputs(desc, fewer), 1, False)
    _check_values(desc, pl, W, False)
    stuck = set(pl.stuck)
    for u in pl.units:
        if (u[0], u[1], u[2]) in stuck:
            for p in u[4]:
                assert waves[p // n, p % n] == -1 and W[0, p // n, p % n] == POISON
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


def test_disagreeing_sources(ctx):
    desc, cls, ins, _ = planned("zkdsa3")
    n = 1 << int(desc.degree_bits)
    pk0 = 12 * n + 1                                         # public key word 0: written by row 1's PoseidonGate, copied to (row 3, col 4)
    gc = glp.Circuit(ctx, desc)
    plan = gc.witness_plan(ins + [pk0])
    assert plan.info["num_stuck_units"] == 0
    values = _inputs(desc, ins + [pk0])
    values[0, -1] = (int(values[0, -1]) + 1) % binding.P
    ptr, W = _generate(ctx, plan, desc, values, 1, True)
    rep = gc.check_witness(dev_wires_ptr=ptr)
    assert rep.failed_copies > 0
    assert W[0, 12, 1] == desc.wires[12, 1] and W[0, 4, 3] == values[0, -1]      # each holds what one of its sources produced
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(match, fn, *args):
    with pytest.raises(glp.GlpError, match=match):
        binding._chk(fn(*args))


def test_refusals(ctx):
    desc, cls, ins, _ = planned("zkdsa3")
    L = binding.load_library()
    gc = glp.Circuit(ctx, desc)
    n, nw = 1 << int(desc.degree_bits), int(desc.num_wires)
    cells = np.array(ins, np.uint64)
    h = C.c_void_p()
    create = L.glp_witness_plan_create
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    # the plan
    _refused("ctx is null", create, None, gc._h, ptr(cells), cells.size, C.byref(h))
    _refused("circuit is null", create, ctx._h, None, ptr(cells), cells.size, C.byref(h))
    _refused("out is null", create, ctx._h, gc._h, ptr(cells), cells.size, None)
    _refused("input_cells is null", create, ctx._h, gc._h, None, cells.size, C.byref(h))
    other = glp.Context(0)
    _refused("circuit belongs to another ctx", create, other._h, gc._h, ptr(cells), cells.size, C.byref(h))
    bad = cells.copy()
    bad[3] = nw * n
    _refused(r"input_cells\[3\] = %d is out of range" % (nw * n), create, ctx._h, gc._h, ptr(bad), bad.size, C.byref(h))
    bad = cells.copy()
    bad[5] = bad[2]
    _refused(r"input_cells\[5\] = %d is listed twice \(also input_cells\[2\]\)" % bad[2], create, ctx._h, gc._h, ptr(bad), bad.size, C.byref(h))
    bad = np.append(cells, np.uint64(4 * n + 1))             # (row 1, col 4) carries the private key word of (row 1, col 0)
    assert cls[4 * n + 1] == cls[0 * n + 1] == 0 * n + 1 and (0 * n + 1) in ins
    _refused(r"input_cells\[%d\] = %d and input_cells\[8\] = %d lie in one copy class" % (ins.index(1), 1, 4 * n + 1), create, ctx._h, gc._h, ptr(bad),
             bad.size, C.byref(h))
    assert not h.value
    with pytest.raises(glp.GlpError, match="role_out is null"):
        binding._chk(L.glp_witness_unit_columns(gc._h, 0, 0, None))
    with pytest.raises(glp.GlpError, match=r"unit = 7, a row of gate \d+ has 1 units"):
        gi = next(i for i, g in enumerate(desc.gates) if int(g["type"]) == binding.GATE_POSEIDON)
        binding._chk(L.glp_witness_unit_columns(gc._h, gi, 7, ptr(np.zeros(nw, np.uint8))))
    # generation
    plan = gc.witness_plan(ins)
    W = np.zeros(desc.wires.shape, np.uint64)
    dev = ctx.dev_alloc(W.nbytes)
    vals = _inputs(desc, ins)
    gen = L.glp_witness_generate
    _refused("ctx is null", gen, None, plan._h, 1, ptr(vals), C.c_void_p(dev), 0)
    _refused("plan is null", gen, ctx._h, None, 1, ptr(vals), C.c_void_p(dev), 0)
    _refused("dev_wires is null", gen, ctx._h, plan._h, 1, ptr(vals), None, 0)
    _refused("input_values is null", gen, ctx._h, plan._h, 1, None, C.c_void_p(dev), 0)
    _refused("plan belongs to another ctx", gen, other._h, plan._h, 1, ptr(vals), C.c_void_p(dev), 0)
    _refused(r"num_proofs = 0 outside 1\.\.4096", gen, ctx._h, plan._h, 0, ptr(vals), C.c_void_p(dev), 0)
    _refused(r"num_proofs = 4097 outside 1\.\.4096", gen, ctx._h, plan._h, 4097, ptr(vals), C.c_void_p(dev), 0)
    _refused("flags = 0x2 has bits other than", gen, ctx._h, plan._h, 1, ptr(vals), C.c_void_p(dev), 2)
    bad = np.tile(vals, (2, 1))
    bad[1, 6] = binding.P
    _refused(r"input_values: proof 1, input 6 = 0xffffffff00000001 is not a canonical", gen, ctx._h, plan._h, 2, ptr(bad), C.c_void_p(dev), 0)
    # read_cells
    out = np.zeros(4, np.uint64)
    rd = L.glp_witness_read_cells
    _refused("dev_wires is null", rd, ctx._h, gc._h, 1, None, ptr(cells), 4, ptr(out))
    _refused("cells is null", rd, ctx._h, gc._h, 1, C.c_void_p(dev), None, 4, ptr(out))
    _refused("out is null", rd, ctx._h, gc._h, 1, C.c_void_p(dev), ptr(cells), 4, None)
    _refused("circuit belongs to another ctx", rd, other._h, gc._h, 1, C.c_void_p(dev), ptr(cells), 4, ptr(out))
    bad = cells.copy()
    bad[1] = nw * n + 5
    _refused(r"cells\[1\] = %d is out of range" % (nw * n + 5), rd, ctx._h, gc._h, 1, C.c_void_p(dev), ptr(bad), 4, ptr(out))
    ctx.dev_free(dev)
    plan.free()
    other.close()
    gc.free()


def test_size_refusals(ctx):
    """num_wires * n at the bound of the decoded sigma (plan, read_cells) and the size cap of glp_witness_generate, on circuit
    descriptions whose num_wires alone is raised"""
    L = binding.load_library()
    h = C.c_void_p()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    one = np.zeros(1, np.uint64)
    small = ctx.dev_alloc(64)
    # 2^13 rows x (2^19 + 1) wires = 2^32 + 2^13 cells, and x 2^19 wires = 2^32 cells exactly: position 2^32 - 1 is not a cell either
    for nw in ((1 << 19) + 1, 1 << 19):
        desc = copy.copy(synth.arith_circuit(13))
        desc.num_wires = nw
        gc = glp.Circuit(ctx, desc)
        cells = nw << 13
        _refused(r"num_wires \* 2\^degree_bits = %d positions, a plan addresses fewer than 2\^32" % cells, L.glp_witness_plan_create, ctx._h, gc._h,
                 ptr(one), 1, C.byref(h))
        assert not h.value
        _refused(r"num_wires \* 2\^degree_bits = %d positions, cells are named below 2\^32" % cells, L.glp_witness_read_cells, ctx._h, gc._h, 1,
                 C.c_void_p(small), ptr(one), 1, ptr(one))
        gc.free()
    # 4096 proofs x (2^18 + 1) wires x 2^3 rows x 8 bytes is past the 64 GiB cap; at 4095 proofs of 2^18 wires it is not refused for size
    base, cls, ins, _ = planned("zkdsa3")
    desc = copy.copy(base)
    desc.num_wires = (1 << 18) + 1
    gc = glp.Circuit(ctx, desc)
    plan = gc.witness_plan(ins)
    assert plan.info["num_stuck_units"] == 0 and plan.info["num_units"] == 5
    vals = np.tile(_inputs(base, ins), (4096, 1))
    _refused(r"wires too large \(num_proofs \* num_wires \* 2\^degree_bits words\)", L.glp_witness_generate, ctx._h, plan._h, 4096, ptr(vals),
             C.c_void_p(small), 0)
    plan.free()
    gc.free()
    ctx.dev_free(small)


def test_closing_the_context_frees_its_plans():
    desc, cls, ins, _ = planned("zkdsa3")
    c = glp.Context(0)
    gc = glp.Circuit(c, desc)
    plan = gc.witness_plan(ins)
    assert plan._h
    c.close()
    assert plan._h is None
    plan.free()
