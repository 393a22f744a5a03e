"""Free units of witness generation on the GPU (include/glp.h, "witness generation, the dataflow half", FREE UNITS):
glp_witness_plan_create_ex / glp_witness_plan_free_info / glp_witness_generate against tests/witness_free_restate.py, which
tests/test_witness_free_restate.py pins to the gadget builders first, and tests/test_biguint_host.py pins to Python integers.

Per kind, one circuit of one gadget call is generated for K proofs in lock step, proof k carrying edge operand set k; the expected
witness of proof k is the builder run on those operands (for the addition with a + b = m, where the builder says `>=` and the reference
`>`, it is the restatement).  Then inputs outside a generator's domain, one whole secp256k1 signature from its 40 words, a withheld
inverse, and every refusal.

Inputs of a plan here are `witness_inputs` -- what a caller sets -- followed by `witness_zero_inputs`, cells of value 0 that the unused
operations of partly filled rows read (gadgets.py, `_attach_free_units`)."""
import ctypes as C
import functools

import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.gadgets_ecdsa as E
from plonky2_lib_amd import binding
import witness_free_restate as fr
import witness_plan_restate as wp
from test_witness_free_restate import OPS, build_op, no_addition_hits_the_modulus, planned

pytestmark = pytest.mark.gpu

FP, FN, P = E.FP, E.FN, binding.P
ENV = "GLP_WITNESS_NARROW_MAX"
FORMS = ("0", str(1 << 31))                 # every wave wide; every wave walked


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _rand(rng, m):
    return int.from_bytes(rng.bytes(40), "little") % m


def _flip_pairs(which, count, rng):
    """k, k + 1 either side of a sign flip of k1 (which = 2) or k2 (3)"""
    out = []
    while len(out) < 2 * count:
        lo, hi = sorted(_rand(rng, FN) for _ in range(2))
        if fr.glv_decompose(lo)[which] == fr.glv_decompose(hi)[which]:
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fr.glv_decompose(mid)[which] == fr.glv_decompose(lo)[which] else (lo, mid)
        out += [(lo,), (hi,)]
    return out


def edge_sets(name):
    """the operand sets of the K proofs of one kind: the named edges of the issue, filled up with random ones to 16"""
    rng = np.random.default_rng(sorted(OPS).index(name))
    if name == "is_equal":
        sets = [(5, 5), (0, 0), (P - 1, 0), (0, P - 1), (1, 2), (P - 1, P - 1), (1 << 32, (1 << 32) - 1)]
        fill = lambda: (_rand(rng, P), _rand(rng, P))
    elif name in ("add", "sub", "mul"):
        m = FN if name == "sub" else FP
        sets = [(m - 1, m - 1), (m - 5, 5), (m - 5, 6), (3, 9), (9, 3), (7, 7), (0, 0), (0, m - 1), (m - 1, 0), (1, m - 1), (1 << 255, 1 << 255), (m // 2, m // 2 + 1),
                ((1 << 128) - 1, (1 << 128) + 1)]
        fill = lambda: (_rand(rng, m), _rand(rng, m))
    elif name == "inv":
        sets = [(1,), (FN - 1,), (2,), ((FN + 1) // 2,), (3,), (FN - 2,), (1 << 255,), (0xFFFFFFFF,), (1 << 32,)]
        fill = lambda: (_rand(rng, FN - 1) + 1,)
    elif name == "div_rem":
        big = (1 << 384) - 1                                 # the quotient has 12 - 8 + 1 = 5 limbs: the builder wants a / b below 2^160
        sets = [(5, (1 << 255) + 9), (0, 1), ((1 << 160) - 1, 1), (big, (1 << 256) - 1), (big, 1 << 255), ((1 << 256) - 1, (1 << 256) - 1),
                ((1 << 300) + 1, (1 << 200) - 1), (3 << 382, (1 << 224) | 1), (1 << 161, 3), (12345, 12345), (12345, 12346),
                ((0x80000000 << 64) | 3, (0x20000000 << 64) | 1)]

        def fill():
            b = _rand(rng, 1 << int(rng.integers(1, 257))) + 1
            return _rand(rng, 1 << min(159, 383 - b.bit_length())) * b + _rand(rng, b), b
    else:
        sets = [(0,), (1,), (FN - 1,), (2,), (FN // 2,), (FN // 2 + 1,)] + _flip_pairs(2, 2, rng) + _flip_pairs(3, 2, rng)
        fill = lambda: (_rand(rng, FN),)
    while len(sets) < 16:
        sets.append(fill())
    return sets


@functools.lru_cache(maxsize=None)
def lock_step(name):
    """-> (circuit of set 0, inputs [K][num_inputs], expected witnesses [K][num_wires][n], restated plan)"""
    c0, cls, ins, free, pl = planned(name)
    sets = edge_sets(name)
    inputs, want = [], []
    for values in sets:
        c = build_op(name, values)
        assert (c.sigmas == c0.sigmas).all() and (c.free_cells == c0.free_cells).all() and (c.constants == c0.constants).all()
        vals = [int(c.wires.reshape(-1)[p]) for p in ins]
        if name == "add" and sum(values) == FP:          # the reference's strict `>`: sum = m, overflow = 0
            w = fr.generate(pl, vals, np.zeros_like(c.wires))
            k_sum, k_over = free[0].outs[:8], free[0].outs[8]
            assert fr._big(w.reshape(-1)[k_sum]) == FP and w.reshape(-1)[k_over] == 0 and (w != c.wires).any()
        else:
            w = c.wires
        inputs.append(vals)
        want.append(w)
    return c0, np.array(inputs, np.uint64), np.stack(want).astype(np.uint64), pl


def _plan(gc, c, ins=None, units=None):
    ins = list(c.witness_inputs) + list(c.witness_zero_inputs) if ins is None else ins
    return gc.witness_plan(ins, free_units=(c.free_units if units is None else units, c.free_cells), moduli=c.moduli)


def _generate(ctx, plan, c, inputs, K):
    W = np.full((K,) + c.wires.shape, 0x0BADC0DE0BADC0DE, np.uint64)
    ptr = ctx.dev_alloc(W.nbytes)
    ctx.dev_upload(ptr, W)
    plan.generate(ptr, inputs, K, zero_first=True)
    ctx.dev_download(ptr, W)
    return ptr, W


def _clean(reps):
    return all((r.failed_constraints, r.failed_rows, r.failed_copies) == (0, 0, 0) for r in (reps if isinstance(reps, list) else [reps]))


# ---------------------------------------------------------------------------------------------------- per kind, K proofs in lock step
@pytest.mark.parametrize("name", sorted(OPS))
def test_kind_in_lock_step(ctx, name, monkeypatch):
    c, inputs, want, pl = lock_step(name)
    K = inputs.shape[0]
    assert 16 <= K <= 32
    gc = glp.Circuit(ctx, c)
    for form in FORMS:
        monkeypatch.setenv(ENV, form)
        plan = _plan(gc, c)
        assert plan.info == pl.info and plan.free_info == pl.free_info
        assert plan.free_info["num_stuck_free_units"] == 0 and plan.info["num_stuck_units"] == 0
        assert (plan.cell_waves() == pl.cell_waves).all()
        ptr, W = _generate(ctx, plan, c, inputs, K)
        for k in range(K):
            assert (W[k] == want[k]).all(), "form %s, proof %d: %d cells differ" % (form, k, (W[k] != want[k]).sum())
        assert _clean(gc.check_witness(dev_wires_ptr=ptr, num_proofs=K, public_inputs=np.tile(c.public_inputs, (K, 1))))
        ctx.dev_free(ptr)
        plan.free()
    gc.free()


def test_multi_add_in_lock_step(ctx, monkeypatch):
    """NONNATIVE_MULTI_ADD, which no gadget of the builders emits: units placed by hand on cells nothing constrains
    (test_witness_free_restate.multi_add): 0, 1, 3, 17 and 65 summands, summands of 0, 1, 2, 3, 8 and 18 limbs, two moduli, 3 x (m - 1),
    unreduced summands, cells >= 2^32"""
    from test_witness_free_restate import MULTI_ADD_PROOFS, MULTI_ADD_UNITS, multi_add
    c, ins, free, pl, values = multi_add()
    K = MULTI_ADD_PROOFS
    want = np.stack([fr.generate(pl, values[k], np.zeros_like(c.wires)) for k in range(K)])
    gc = glp.Circuit(ctx, c)
    for form in FORMS:
        monkeypatch.setenv(ENV, form)
        plan = _plan(gc, c, ins=ins)
        assert plan.info == pl.info and plan.free_info == pl.free_info and plan.free_info["num_free_units"] == 1 + len(MULTI_ADD_UNITS)
        assert (plan.cell_waves() == pl.cell_waves).all()
        ptr, W = _generate(ctx, plan, c, values, K)
        for k in range(K):
            assert (W[k] == want[k]).all(), "form %s, proof %d: %d cells differ" % (form, k, (W[k] != want[k]).sum())
        assert _clean(gc.check_witness(dev_wires_ptr=ptr, num_proofs=K, public_inputs=np.tile(c.public_inputs, (K, 1))))
        ctx.dev_free(ptr)
        plan.free()
    # the run of a MULTI_ADD unit is len[0] * len[1] + sum + overflow cells: the planner holds it to cells[]
    rows = np.array(c.free_units, np.int64)
    rows[-1, 3] = 65535
    with pytest.raises(glp.GlpError, match=r"units\[%d\]\.cell_begin = %d: its run of %d cells leaves cells\[\]" % (len(rows) - 1, rows[-1, 2], 65535 * 2 + 9)):
        gc.witness_plan(ins, free_units=(rows, c.free_cells), moduli=c.moduli)
    gc.free()


# ---------------------------------------------------------------------------------------------------- outside a generator's domain
@pytest.mark.parametrize("name,values", [("inv", (0,)), ("div_rem", ((1 << 300) + 5, 0)), ("mul", (3, 5))])
def test_out_of_domain(ctx, name, values, monkeypatch):
    """x = 0, a divisor of 0, an operand cell >= 2^32: ordinary values on bounded loops; GLP_OK, the restated fixed values, and a
    witness the checker rejects by row"""
    c, cls, ins, free, pl = planned(name)
    vals = [int(c.wires.reshape(-1)[p]) for p in ins]
    nin = len(c.witness_inputs)
    limbs = [l for v, ln in zip(values, OPS[name][1]) for l in fr._limbs(v, ln)]
    vals[:nin] = limbs
    if name == "mul":
        vals[0] = 3 + (7 << 32)                              # read as its low 32 bits by the generator, as it stands by the gates
    ref = fr.generate(pl, vals, np.zeros_like(c.wires))
    f = free[0]
    flat = ref.reshape(-1)
    if name == "inv":
        assert not flat[f.outs].any()                        # inv = div = 0
    elif name == "div_rem":
        assert not flat[f.outs].any()                        # div = rem = 0
    else:
        assert fr._big(flat[f.outs[:8]]) == 15
    gc = glp.Circuit(ctx, c)
    for form in FORMS:
        monkeypatch.setenv(ENV, form)
        plan = _plan(gc, c)
        ptr, W = _generate(ctx, plan, c, np.array([vals], np.uint64), 1)
        assert (W[0] == ref).all(), "form %s: %d cells differ" % (form, (W[0] != ref).sum())
        rep = gc.check_witness(dev_wires_ptr=ptr)
        assert not rep.ok and (rep.row is not None or rep.copy_row is not None), str(rep)
        ctx.dev_free(ptr)
        plan.free()
    gc.free()


# ---------------------------------------------------------------------------------------------------- one signature
@functools.lru_cache(maxsize=None)
def signature_circuit(seed):
    return E.ecdsa_circuit(E.random_signatures(1, seed=seed))


def test_one_signature_from_its_40_words(ctx, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    cs = [signature_circuit(0), signature_circuit(1)]
    c = cs[0]
    assert int(c.degree_bits) == 17 and c.witness_inputs.size == 40
    for d in cs:
        # the only input on which builder and reference differ does not occur, so the comparison below may leave out no cell
        assert no_addition_hits_the_modulus(d, fr.from_arrays(d.free_units, d.free_cells, d.moduli))
        assert (d.sigmas == c.sigmas).all() and (d.free_cells == c.free_cells).all() and (d.witness_inputs == c.witness_inputs).all()
    msg, (r, s), pk = E.random_signatures(1, seed=0)[0]
    words = [l for v in (msg, r, s, pk[0], pk[1]) for l in fr._limbs(v, 8)]
    assert [int(v) for v in c.wires.reshape(-1)[c.witness_inputs.astype(np.int64)]] == words
    nz = c.witness_zero_inputs.size
    gc = glp.Circuit(ctx, c)
    plan = _plan(gc, c)
    info, finfo = plan.info, plan.free_info
    assert info["num_stuck_units"] == 0 and finfo["num_stuck_free_units"] == 0 and finfo["num_free_units"] == c.free_units.shape[0]
    for K in (1, 2):
        inputs = np.array([[int(v) for v in d.wires.reshape(-1)[d.witness_inputs.astype(np.int64)]] + [0] * nz for d in cs[:K]], np.uint64)
        ptr, W = _generate(ctx, plan, c, inputs, K)
        for k in range(K):
            assert (W[k] == cs[k].wires).all(), "K = %d, proof %d: %d cells differ" % (K, k, (W[k] != cs[k].wires).sum())
        assert _clean(gc.check_witness(dev_wires_ptr=ptr, num_proofs=K, public_inputs=np.tile(c.public_inputs, (K, 1))))
        if K == 1:
            assert gc.verify(gc.prove_device(ptr)), binding.load_library().glp_last_error()
        ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ---------------------------------------------------------------------------------------------------- stuck
def test_a_withheld_inverse_is_stuck(ctx):
    c, cls, ins, free, _ = planned("curve_add")
    inv = [i for i, f in enumerate(free) if f.kind == fr.INV]
    pl = fr.plan(c, ins, free, cls, withhold=inv)
    gc = glp.Circuit(ctx, c)
    plan = _plan(gc, c, units=np.delete(c.free_units, inv, axis=0))
    assert plan.info == pl.info and plan.free_info == pl.free_info
    assert plan.free_info["first_stuck_free_unit"] == pl.stuck_free[0] and plan.free_info["num_stuck_free_units"] == len(pl.stuck_free) > 0
    assert (plan.info["stuck_row"], plan.info["stuck_gate"], plan.info["stuck_unit"]) == pl.stuck[0]
    waves = plan.cell_waves()
    assert (waves == pl.cell_waves).all()
    vals = np.array([[int(c.wires.reshape(-1)[p]) for p in ins]], np.uint64)
    ptr, W = _generate(ctx, plan, c, vals, 1)
    assert (W[0] == np.where(waves >= 0, c.wires, 0)).all()         # what is not stuck is still generated, the rest is untouched
    ctx.dev_free(ptr)
    plan.free()
    gc.free()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx):
    c, cls, ins, free, _ = planned("curve_add")
    L = binding.load_library()
    gc = glp.Circuit(ctx, c)
    n, nw = 1 << int(c.degree_bits), int(c.num_wires)
    ncells = nw * n
    h = C.c_void_p()
    inputs = np.array(ins, np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None

    def units_of(rows):
        u = np.zeros(len(rows), binding.FREE_UNIT_DTYPE)
        rows = np.asarray(rows, np.int64).reshape(-1, 9)
        u["kind"], u["modulus"], u["cell_begin"], u["len"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:]
        return u

    def refused(match, rows=None, cells=None, moduli=None, num_moduli=None, inputs=inputs):
        u = units_of(c.free_units if rows is None else rows)
        fc = np.ascontiguousarray(c.free_cells if cells is None else cells, dtype=np.uint64)
        md = np.ascontiguousarray(c.moduli if moduli is None else moduli, dtype=np.uint32)
        with pytest.raises(glp.GlpError, match=match):
            binding._chk(L.glp_witness_plan_create_ex(ctx._h, gc._h, ptr(inputs), inputs.size, ptr(u), u.size, ptr(fc), fc.size, ptr(md),
                                                      md.size // 8 if num_moduli is None else num_moduli, C.byref(h)))
        assert not h.value

    base = np.array(c.free_units, np.int64)
    kinds = [int(k) for k in base[:, 0]]
    i_mul, i_sub, i_inv = kinds.index(fr.MUL), kinds.index(fr.SUB), kinds.index(fr.INV)

    def edit(i, col, value):
        rows = base.copy()
        rows[i, col] = value
        return rows
    refused(r"units\[%d\]\.kind = 9 is not a GLP_WGEN_\* kind" % i_mul, edit(i_mul, 0, 9))
    refused(r"units\[%d\]\.kind = 0 is not a GLP_WGEN_\* kind" % i_mul, edit(i_mul, 0, 0))
    eq = [[fr.EQUALITY, 0, 0, 1, 2, 1, 1, 0, 0]]
    refused(r"units\[0\]\.len\[1\] = 2, that operand of kind 1 is 1 cell", eq)
    refused(r"units\[%d\]\.len\[3\] = 2, that operand of kind 4 is 1 cell" % i_sub, edit(i_sub, 3 + 3, 2))
    refused(r"units\[%d\]\.len\[3\] = 1, kind 6 has 3 operands: unused entries are 0" % i_inv, edit(i_inv, 3 + 3, 1))
    refused(r"units\[0\]\.len\[1\] = 5, GLV_SECP256K1 has k of 8 and k1, k2 of 4 limbs", [[fr.GLV, 0, 0, 8, 5, 4, 1, 1, 0]])
    refused(r"units\[%d\]\.len\[0\] = 19, an operand has at most GLP_WGEN_MAX_LIMBS = 18 limbs" % i_mul, edit(i_mul, 3, 19))
    refused(r"units\[0\]\.len\[1\] = 9, a divisor has at most 8 limbs", [[fr.DIV_REM, 0, 0, 12, 9, 4, 9, 0, 0]])
    refused(r"units\[%d\]\.modulus = 1, num_moduli = 1" % i_mul, edit(i_mul, 1, 1))
    refused(r"units\[%d\]\.modulus = 0, num_moduli = 0" % next(i for i, k in enumerate(kinds) if 2 <= k <= 6), num_moduli=0)
    refused(r"units\[0\]\.modulus = 1, kind 7 has no modulus: 0", [[fr.DIV_REM, 1, 0, 1, 1, 1, 1, 0, 0]])
    even = np.array(c.moduli, np.uint32)
    even[0, 0] &= 0xFFFFFFFE
    refused(r"moduli\[0\] is even", moduli=even)
    refused(r"moduli\[0\] = 1 is below 3", moduli=np.array([[1, 0, 0, 0, 0, 0, 0, 0]], np.uint32))
    cb = int(base[i_mul, 2])
    bad = np.array(c.free_cells, np.uint64)
    bad[cb + 3] = ncells
    refused(r"units\[%d\]: cells\[%d\] = %d is out of range" % (i_mul, cb + 3, ncells), cells=bad)
    bad = np.array(c.free_cells, np.uint64)
    bad[cb + 3] = binding.WGEN_NO_CELL                       # an input cell may not be left out
    refused(r"units\[%d\]: cells\[%d\] = %d is out of range" % (i_mul, cb + 3, binding.WGEN_NO_CELL), cells=bad)
    refused(r"units\[%d\]\.cell_begin = %d: its run of 32 cells leaves cells\[\] \(num_cells = %d\)" % (i_mul, c.free_cells.size - 31, c.free_cells.size),
            edit(i_mul, 2, c.free_cells.size - 31))
    twice = np.vstack([base, base[i_inv:i_inv + 1]])
    refused(r"units\[%d\]: output cell \d+ is also written by units\[%d\]" % (len(base), i_inv), twice)
    # an output cell that a gate unit of its row writes too: the product's first limb moved onto the output of an arithmetic operation
    us = wp.all_units(c)
    row, gate, unit, _, outs = next(u for u in us if int(c.gates[u[1]]["type"]) == binding.GATE_ARITHMETIC)
    bad = np.array(c.free_cells, np.uint64)
    bad[cb + 16] = outs[0]
    refused(r"units\[%d\]: output cell %d \(column %d, row %d\) is also written by unit %d of gate %d of that row" % (i_mul, outs[0], outs[0] // n, outs[0] % n, unit, gate),
            cells=bad)
    with pytest.raises(glp.GlpError, match="units is null, num_units = 3"):
        binding._chk(L.glp_witness_plan_create_ex(ctx._h, gc._h, ptr(inputs), inputs.size, None, 3, None, 0, None, 0, C.byref(h)))
    with pytest.raises(glp.GlpError, match="plan is null"):
        binding._chk(L.glp_witness_plan_free_info(None, None))
    # what stays allowed: an output cell whose class holds an input; an output that is not placed
    f = free[i_mul]
    plan = _plan(gc, c, ins=ins + [f.outs[0]])
    assert plan.info["num_stuck_units"] == 0
    plan.free()
    ok = np.array(c.free_cells, np.uint64)
    ok[cb + 16 + 15] = binding.WGEN_NO_CELL                  # the top limb of the overflow
    plan = gc.witness_plan(ins, free_units=(c.free_units, ok), moduli=c.moduli)
    assert plan.free_info["num_free_units"] == len(free)
    plan.free()
    # a plan without free units is the old entry point
    plain = gc.witness_plan(ins)
    assert plain.free_info == dict(num_free_units=0, num_stuck_free_units=0, first_stuck_free_unit=None, widest_wave_free_units=0)
    assert plain.info["num_stuck_units"] > 0
    plain.free()
    gc.free()
