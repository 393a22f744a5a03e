"""Random cells of a witness plan on the GPU (include/glp.h, "witness generation, the dataflow half", RANDOM CELLS):
glp_witness_plan_create_rand, k_witness_random and glp_witness_generate against tests/witness_random_restate.py -- the PRF over the
oracle's Poseidon and the restated planner over inputs + random cells -- and, for zero-knowledge circuits of the two builders, against
the witnesses the builders hold: a zk witness generated from the words a caller sets, proved and verified.

What a generated zk witness must be, cell by cell (`_expected`): a random cell holds its PRF value; every other member of a random
cell's copy class (row r2 of a blinding pair) holds that value too; every other cell the plan reaches holds the builder's value for the
same inputs; a cell the plan never reaches (padding rows, which the synthetic builder leaves random) holds what the buffer held, 0 with
GLP_WITNESS_GEN_ZERO_FIRST.  The seed is fixed (glp_ctx_set_salt_seed) with seed3 = p - 2, so that seed3 + k wraps at member 2."""
import ctypes as C
import functools

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding, gadgets, synth
import witness_plan_restate as wp
import witness_program_restate as wpr
import witness_random_restate as rr
from test_gpu_zk import _check_zk_proof
from test_witness_plan_restate import planned
from test_witness_random_host import noop_circuit, refusals, scattered

pytestmark = pytest.mark.gpu

P = binding.P
SEED = [11, 22, 33, P - 2]
POISON = 0x0BADC0DE0BADC0DE                 # canonical
ENV = "GLP_WITNESS_NARROW_MAX"
ALL_WALKED = str(1 << 31)


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    c.set_salt_seed(SEED)
    yield c
    c.close()


def _generate(ctx, plan, shape, inputs, K, zero_first, poison=POISON):
    W = np.full((K,) + tuple(shape), poison, np.uint64)
    ptr = ctx.dev_alloc(W.nbytes)
    ctx.dev_upload(ptr, W)
    plan.generate(ptr, inputs, K, zero_first=zero_first)
    ctx.dev_download(ptr, W)
    return ptr, W


def _info(pl):
    """the restated figures as the binding reports them: the stuck_* fields are None unless a unit is stuck"""
    out = dict(pl.info)
    if not out["num_stuck_units"]:
        out["stuck_row"] = out["stuck_gate"] = out["stuck_unit"] = None
    return out


def _clean(reps):
    return all((r.failed_constraints, r.failed_rows, r.failed_copies) == (0, 0, 0) for r in (reps if isinstance(reps, list) else [reps]))


# ------------------------------------------------------------------------------------------------ 1. PRF and scatter
@pytest.mark.parametrize("num_random", [1, 7, 8, 9, 8 * 256 + 3])
def test_prf_and_scatter(ctx, oracle, num_random):
    """a single partial block, a full block, a full block plus one, and a count past one workgroup of lanes with a partial tail"""
    c = noop_circuit()
    K = 3
    ins = [5, 64 * 80 - 1, 1000]
    rnd = scattered(num_random, skip=ins)
    vals = np.array([[7 + k, P - 1, 1 << 32] for k in range(K)], np.uint64)
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(ins, random_cells=rnd)
    assert plan.num_random == num_random and plan.num_inputs == 3
    pl = rr.plan(c, ins, rnd, cls=np.arange(80 * 64, dtype=np.int64))
    assert plan.info == _info(pl) and (plan.cell_waves() == pl.cell_waves).all()
    assert plan.info["num_cells_known"] == num_random + 3
    for zero_first in (False, True):
        fill = 0 if zero_first else POISON
        ptr, W = _generate(ctx, plan, c.wires.shape, vals, K, zero_first)
        ctx.dev_free(ptr)
        for k in range(K):
            want = rr.generate(oracle, pl, vals[k], SEED, np.full(c.wires.shape, fill, np.uint64), k)
            assert (want.reshape(-1)[rnd] == rr.values(oracle, SEED, num_random, k)).all() and (want == fill).sum() == 80 * 64 - num_random - 3
            assert (W[k] == want).all(), "proof %d: %d cells differ" % (k, (W[k] != want).sum())
    if num_random >= 8:                      # seed3 + 2 wrapped to 0: member 2 is the PRF of (11, 22, 33, 0)
        assert (W[2].reshape(-1)[rnd[:8]] == rr.block(oracle, SEED[:3] + [0], 0)).all()
    plan.free()
    gc.free()


# ------------------------------------------------------------------------------------------------ 2. real zk circuits, 2 query rounds
def _zk_config():
    return synth.Config.standard_recursion_zk_config(num_query_rounds=2)       # the smallest degree blinding_counts gives


@functools.lru_cache(maxsize=None)
def zk_zkdsa(K=4):
    """-> (member circuits, classes, input cells, restated plan): K zkdsa witnesses of one zk circuit, from 8 words each"""
    rng = np.random.default_rng(31)
    cs = [synth.zkdsa_circuit(config=_zk_config(), private_key=synth.gl.rand(rng, 4), message=synth.gl.rand(rng, 4), blinding_seed=k) for k in range(K)]
    c = cs[0]
    assert all((d.sigmas == c.sigmas).all() and (d.witness_random_cells == c.witness_random_cells).all() for d in cs)
    n = 1 << int(c.degree_bits)
    cls = wp.classes(c)
    ins = wp.default_inputs(c, cls)
    assert ins == sorted((p // 8) * n + p % 8 for p in planned("zkdsa3")[2]) and len(ins) == 8           # the cells of the non-zk circuit
    return cs, cls, ins, rr.plan(c, ins, c.witness_random_cells, cls=cls)


@functools.lru_cache(maxsize=None)
def zk_smt():
    """-> (member circuits, classes, input cells, restated plan): the 16-level inclusion circuit under the zk config, an included and
    a missing key"""
    tree = gadgets.SparseMerkleTree()
    for k, v in ((1, 2), (12, 1), (5, 51)):
        tree.insert(gadgets.hash_out_from_u128(k), gadgets.hash_out_from_u128(v))
    cs = [gadgets.smt_inclusion_circuit(tree, gadgets.hash_out_from_u128(key), config=_zk_config()) for key in (5, 9)]
    c = cs[0]
    for d in cs:
        assert (d.sigmas == c.sigmas).all() and (d.constants == c.constants).all() and (d.free_units == c.free_units).all()
        assert (d.witness_inputs == c.witness_inputs).all() and (d.witness_zero_inputs == c.witness_zero_inputs).all()
        assert (d.witness_random_cells == c.witness_random_cells).all() and (d.free_cells == c.free_cells).all()
    plain = gadgets.smt_inclusion_circuit(tree, gadgets.hash_out_from_u128(5))
    n, n0 = 1 << int(c.degree_bits), 1 << int(plain.degree_bits)
    move = lambda cells: [int(p) // n0 * n + int(p) % n0 for p in cells]
    assert [int(p) for p in c.witness_inputs] == move(plain.witness_inputs) and [int(p) for p in c.witness_zero_inputs] == move(plain.witness_zero_inputs)
    ins = [int(p) for p in c.witness_inputs] + [int(p) for p in c.witness_zero_inputs]
    cls = wp.classes(c)
    free = wpr.from_arrays(c.free_units, c.free_cells, c.moduli, c.witness_programs)
    return cs, cls, ins, rr.plan(c, ins, c.witness_random_cells, free=free, cls=cls)


def _blinding_shape(c, first_row):
    """the builder's list against blinding_counts: r rows x all wires, z pair rows x routed wires, the unused PublicInputGate wires"""
    cfg = _zk_config()
    r, z, lg = synth.blinding_counts(cfg, first_row)
    n = 1 << lg
    assert lg == c.degree_bits
    rc = c.witness_random_cells
    assert rc.dtype == np.uint64 and rc.size == cfg.num_wires * r + cfg.num_routed_wires * z + cfg.num_wires - 4 == len(set(rc.tolist()))
    rows, cols = rc.astype(np.int64) % n, rc.astype(np.int64) // n
    r1 = first_row + r + 2 * np.arange(z)
    assert set(rows[:cfg.num_wires * r].tolist()) == set(range(first_row, first_row + r))
    pair = slice(cfg.num_wires * r, cfg.num_wires * r + cfg.num_routed_wires * z)
    assert set(rows[pair].tolist()) == set(r1.tolist()) and cols[pair].max() == cfg.num_routed_wires - 1      # r2 = r1 + 1 is the copy: not listed
    assert len(set(rows[pair.stop:].tolist())) == 1 and sorted(cols[pair.stop:].tolist()) == list(range(4, cfg.num_wires))
    return r1


def _expected(oracle, d, cls, pl, k, fill=0):
    """the witness of member k, whose builder's circuit is d, cell by cell (the module's docstring)"""
    rc = d.witness_random_cells.astype(np.int64)
    flat_known = (pl.cell_waves >= 0).reshape(-1)
    E = np.where(flat_known, d.wires.reshape(-1), np.uint64(fill)).astype(np.uint64)
    lut = np.zeros(cls.size, np.uint64)
    lut[cls[rc]] = rr.values(oracle, SEED, rc.size, k)
    in_random_class = np.zeros(cls.size, bool)
    in_random_class[cls[rc]] = True
    mask = in_random_class[cls]
    assert flat_known[mask].all()
    E[mask] = lut[cls[mask]]
    return E.reshape(d.wires.shape), mask.reshape(d.wires.shape)


def _prove_and_verify(ctx, oracle, gc, cs, ptr, W, pis):
    """glp_prove_batch on the generated device witnesses; glp_verify, glp_verify_batch and the oracle's checks of tests/test_gpu_zk.py"""
    K = len(cs)
    proofs = gc.prove_batch_device(ptr, K, pis)
    assert all(gc.verify(p) for p in proofs), binding.load_library().glp_last_error()
    assert gc.verify_batch(proofs).all()
    digest = gc.digest()
    for k in range(K):
        class D:
            pass
        d = D()
        d.__dict__.update(cs[k].__dict__)
        d.wires, d.circuit_digest = W[k], digest
        _check_zk_proof(oracle, d, gc, proofs[k], seed=SEED, k=k)


def test_zk_zkdsa_from_eight_words(ctx, oracle, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    cs, cls, ins, pl = zk_zkdsa()
    K, c = len(cs), cs[0]
    n = 1 << int(c.degree_bits)
    r1 = _blinding_shape(c, 6)
    assert synth.zkdsa_circuit(3).witness_random_cells.size == 0 and synth.zkdsa_circuit(3).witness_random_cells.dtype == np.uint64
    gc = glp.Circuit(ctx, c)
    assert gc.zero_knowledge
    plan = gc.witness_plan(ins, random_cells=c.witness_random_cells)
    assert plan.num_inputs == 8 and plan.num_random == c.witness_random_cells.size
    assert plan.info["num_stuck_units"] == 0 and plan.info == _info(pl) and (plan.cell_waves() == pl.cell_waves).all()
    inputs = np.stack([d.wires.reshape(-1)[ins] for d in cs])
    ptr, W = _generate(ctx, plan, c.wires.shape, inputs, K, True)
    for k in range(K):
        E, mask = _expected(oracle, cs[k], cls, pl, k)
        assert (W[k][~mask] == E[~mask]).all(), "proof %d: %d cells outside the random classes differ" % (k, (W[k][~mask] != E[~mask]).sum())
        assert (W[k][:80, r1 + 1] == W[k][:80, r1]).all()                       # row r2 of every pair = row r1
        assert (W[k] == E).all(), "proof %d: %d random cells differ" % (k, (W[k] != E).sum())
    pi_cells = [(4 + i) * n + 2 for i in range(4)] + [(12 + i) * n + 1 for i in range(4)] + [(12 + i) * n + 2 for i in range(4)]   # message, public key, signature
    pis = gc.read_cells(ptr, pi_cells, K)
    assert (pis == np.stack([d.public_inputs for d in cs])).all()
    assert _clean(gc.check_witness(dev_wires_ptr=ptr, num_proofs=K, public_inputs=pis))
    _prove_and_verify(ctx, oracle, gc, cs, ptr, W, pis)
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


def test_zk_smt_inclusion_from_its_inputs(ctx, oracle, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    cs, cls, ins, pl = zk_smt()
    K, c = len(cs), cs[0]
    r1 = _blinding_shape(c, c.gadget_rows)
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(ins, free_units=(c.free_units, c.free_cells), moduli=c.moduli, programs=c.witness_programs, random_cells=c.witness_random_cells)
    assert plan.num_inputs == len(ins) and plan.num_random == c.witness_random_cells.size
    assert plan.info["num_stuck_units"] == 0 and plan.free_info["num_stuck_free_units"] == 0
    assert plan.info == _info(pl) and plan.free_info == pl.free_info and (plan.cell_waves() == pl.cell_waves).all()
    inputs = np.stack([d.wires.reshape(-1)[ins] for d in cs])
    ptr, W = _generate(ctx, plan, c.wires.shape, inputs, K, True)
    for k in range(K):
        E, mask = _expected(oracle, cs[k], cls, pl, k)
        assert (W[k][~mask] == E[~mask]).all(), "proof %d: %d cells outside the random classes differ" % (k, (W[k][~mask] != E[~mask]).sum())
        assert (W[k][:80, r1 + 1] == W[k][:80, r1]).all()
        assert (W[k] == E).all(), "proof %d: %d random cells differ" % (k, (W[k] != E).sum())
    pis = np.stack([d.public_inputs for d in cs])
    assert _clean(gc.check_witness(dev_wires_ptr=ptr, num_proofs=K, public_inputs=pis))
    _prove_and_verify(ctx, oracle, gc, cs, ptr, W, pis)
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ------------------------------------------------------------------------------------------------ 3. both forms
def test_both_forms_agree(ctx, oracle, monkeypatch):
    cs, cls, ins, pl = zk_zkdsa()
    K, c = len(cs), cs[0]
    gc = glp.Circuit(ctx, c)
    inputs = np.stack([d.wires.reshape(-1)[ins] for d in cs])
    got = []
    for narrow in ("0", ALL_WALKED):
        monkeypatch.setenv(ENV, narrow)
        plan = gc.witness_plan(ins, random_cells=c.witness_random_cells)
        ptr, W = _generate(ctx, plan, c.wires.shape, inputs, K, False)
        ctx.dev_free(ptr)
        plan.free()
        got.append(W)
    assert (got[0] == got[1]).all()
    E, _ = _expected(oracle, cs[K - 1], cls, pl, K - 1, fill=POISON)
    assert (got[0][K - 1] == E).all()
    gc.free()


# ------------------------------------------------------------------------------------------------ 4, 5. fresh and fixed seeds
def test_fresh_seeds_differ_in_every_random_cell(oracle):
    cs, cls, ins, pl = zk_zkdsa()
    c = cs[0]
    c2 = glp.Context(0)
    try:
        c2.set_salt_seed(None)
        gc = glp.Circuit(c2, c)
        plan = gc.witness_plan(ins, random_cells=c.witness_random_cells)
        inputs = c.wires.reshape(-1)[ins][None]
        _, mask = _expected(oracle, c, cls, pl, 0)
        Ws = []
        for _ in range(2):
            ptr, W = _generate(c2, plan, c.wires.shape, inputs, 1, True)
            assert _clean(gc.check_witness(dev_wires_ptr=ptr, public_inputs=c.public_inputs))
            c2.dev_free(ptr)
            Ws.append(W[0])
        assert (Ws[0][~mask] == Ws[1][~mask]).all()
        assert (Ws[0][mask] != Ws[1][mask]).all()                # a collision has probability about 2^-64 per cell
        assert (Ws[0][mask] < np.uint64(P)).all() and (Ws[1][mask] < np.uint64(P)).all()
        plan.free()
        gc.free()
    finally:
        c2.close()


def test_a_fixed_seed_repeats(ctx):
    cs, cls, ins, pl = zk_zkdsa()
    c = cs[0]
    gc = glp.Circuit(ctx, c)
    plan = gc.witness_plan(ins, random_cells=c.witness_random_cells)
    inputs = np.stack([d.wires.reshape(-1)[ins] for d in cs[:2]])
    Ws = []
    for _ in range(2):
        ptr, W = _generate(ctx, plan, c.wires.shape, inputs, 2, True)
        ctx.dev_free(ptr)
        Ws.append(W)
    assert (Ws[0] == Ws[1]).all()
    plan.free()
    gc.free()


# ------------------------------------------------------------------------------------------------ 6. refusals through the C ABI
def test_refusals(ctx):
    desc = planned("zkdsa3")[0]
    gc = glp.Circuit(ctx, desc)
    L = binding.load_library()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    for match, ins, rnd, null in refusals():
        ic, rc = np.array(ins, np.uint64), np.array(rnd, np.uint64)
        with pytest.raises(glp.GlpError, match="glp_witness_plan_create_rand: " + match):
            binding._chk(L.glp_witness_plan_create_rand(ctx._h, gc._h, ptr(ic), ic.size, None if null else ptr(rc), rc.size, None, 0, None, 0, None, 0,
                                                        None, 0, C.byref(h)))
        assert not h.value
    assert L.glp_witness_plan_num_random(None) == 0
    with pytest.raises(glp.GlpError, match=r"random_cells\[0\] = %d is out of range" % desc.wires.size):
        gc.witness_plan(planned("zkdsa3")[2], random_cells=[desc.wires.size])
    gc.free()


# ------------------------------------------------------------------------------------------------ 7. the num_random = 0 case
def test_no_random_cells_is_create_prog(ctx):
    """glp_witness_plan_create_rand with num_random = 0 against glp_witness_plan_create_prog on the same request (free units, a unit
    program): the same figures, cell_waves and generated values, which are the builder's witness"""
    tree = gadgets.SparseMerkleTree()
    for k, v in ((1, 2), (2, 7)):
        tree.insert(gadgets.hash_out_from_u128(k), gadgets.hash_out_from_u128(v))
    c = gadgets.smt_inclusion_circuit(tree, gadgets.hash_out_from_u128(1), n_levels=3)
    assert c.witness_random_cells.size == 0 and c.witness_random_cells.dtype == np.uint64
    ins = [int(p) for p in c.witness_inputs] + [int(p) for p in c.witness_zero_inputs]
    gc = glp.Circuit(ctx, c)
    kw = dict(free_units=(c.free_units, c.free_cells), moduli=c.moduli, programs=c.witness_programs)
    prog, rand = gc.witness_plan(ins, **kw), gc.witness_plan(ins, random_cells=c.witness_random_cells, **kw)
    assert rand.num_random == 0 == prog.num_random
    info = rand.info
    assert info == prog.info and rand.free_info == prog.free_info and (rand.cell_waves() == prog.cell_waves()).all()
    assert info["num_stuck_units"] == 0
    known = rand.cell_waves() >= 0
    vals = c.wires.reshape(-1)[ins][None]
    out = []
    for plan in (prog, rand):
        ptr, W = _generate(ctx, plan, c.wires.shape, vals, 1, False)
        ctx.dev_free(ptr)
        out.append(W[0])
        plan.free()
    assert (out[0] == out[1]).all()
    assert (out[1][known] == c.wires[known]).all() and (out[1][~known] == POISON).all()
    gc.free()
