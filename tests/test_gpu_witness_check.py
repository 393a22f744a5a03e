"""glp_witness_check on the GPU (include/glp.h, "witness checker") against tests/witness_check_restate.py, field for field on every
gate type, and for the limb gates (types 4-12 and 14) also against the oracle's prover and verifier as a second judge.
tests/test_witness_check.py and tests/test_limb_gates_restate.py pin the restatement first."""
import copy
import ctypes as C

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding, synth
import limb_gates_restate as lg
import perm_restate as pr
import witness_check_restate as wr
import zeta_identity_recursion as zr
from test_recursion_gates import PARAMS, _role_columns

pytestmark = pytest.mark.gpu

P = wr.P
REC = synth.Config.standard_recursion_config
REC_ZK = synth.Config.standard_recursion_zk_config
ARITH3 = dict(num_const_rows=2, num_noop_rows=1)      # what fits 2^3 rows
ALL_TYPES = set(range(19)) | {20, 21, 22}


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _bump(W, col, row, delta=1):
    W[col, row] = (int(W[col, row]) + delta) % P


def _same(got, rep, by_gate):
    """the library's report of one witness against the restatement's"""
    assert got.as_tuple() == wr.as_tuple(rep), (got.as_tuple(), wr.as_tuple(rep))
    assert got.rows_failed_by_gate == by_gate
    assert got.ok == (wr.as_tuple(rep)[:3] == (0, 0, 0))


def _gate_of_type(desc, t):
    return next(i for i, g in enumerate(desc.gates) if int(g["type"]) == t)


# ---------------------------------------------------------------------------------------------------- 1. clean, every gate type
CLEAN = {
    "arith": lambda: synth.arith_circuit(3, **ARITH3),
    "ext": lambda: synth.ext_gates_circuit(3),
    "recursion-default": lambda: synth.recursion_gates_circuit(3, REC(), params=PARAMS["default"]),
    "recursion-odd": lambda: synth.recursion_gates_circuit(3, REC(), params=PARAMS["odd"]),
    "u32": lambda: synth.u32_circuit(6),
    "ecdsa": lambda: synth.ecdsa_shape_circuit(5),
    "keccak": lambda: synth.keccak_shape_circuit(5),
    "zkdsa": lambda: synth.zkdsa_circuit(3),
    "poseidon-chain": lambda: synth.poseidon_chain_circuit(2),
    "smt": lambda: synth.smt_shape_circuit(4),
    "recursion-zk": lambda: synth.recursion_gates_circuit(3, REC_ZK(), blinding_seed=3),      # with plonky2's blinding rows
    "zkdsa-zk": lambda: synth.zkdsa_circuit(3, REC_ZK(), blinding_seed=3),
}


@pytest.mark.parametrize("name", sorted(CLEAN))
def test_clean_witnesses_are_clean(ctx, name):
    desc = CLEAN[name]()
    assert desc.zero_knowledge == name.endswith("-zk")
    gc = glp.Circuit(ctx, desc)
    rep = gc.check_witness(by_gate=True)
    assert (rep.failed_constraints, rep.failed_rows, rep.failed_copies) == (0, 0, 0) and rep.ok, str(rep)
    assert rep.rows_failed_by_gate == [0] * len(desc.gates) and str(rep) == "witness satisfies the circuit"
    gc.free()


def test_clean_circuits_cover_every_gate_type():
    """the gate tables of the circuits above hold, together, all 22 gate types"""
    seen = {int(g["type"]) for name in CLEAN if not name.endswith("-zk") for g in CLEAN[name]().gates}
    assert seen == ALL_TYPES, sorted(ALL_TYPES - seen)


# ---------------------------------------------------------------------------------------------------- 2. exact reports
def _roles(desc, t, g):
    """{role: wire column} to change on a row of gate g: an input, an output and a limb or bit column of the limb gates"""
    p0, p1 = int(g["p0"]), int(g["p1"])
    if t in synth.RECURSION_GATES:
        return _role_columns(desc, t, g)
    if t == synth.GATE_COMPARISON:
        lay = lg.comparison_layout(p0, p1)
        return {"first input": 0, "result": 2, "most significant diff": 3, "chunk": lay["second_chunks"] + p1 - 1,
                "chunks equal": lay["equal"], "diff bit": lay["msd_bits"] + lay["chunk_bits"]}
    if t == synth.GATE_RANDOM_ACCESS:
        lay = lg.random_access_layout(p0, p1)
        o = lay["per_copy"] * (lay["copies"] - 1)
        return {"index": o, "claimed element": o + 1, "index bit": lay["bits"] + p0 * lay["copies"] - 1, "extra constant": lay["extras"]}
    na = p0 + 3                                   # U32AddMany: wires per op
    return {
        synth.GATE_CONSTANT: {"wire": p0 - 1},
        synth.GATE_PUBLIC_INPUT: {"hash word": 2},
        synth.GATE_ARITHMETIC: {"multiplicand": 4 * (p0 - 1), "addend": 4 * (p0 // 2) + 2, "output": 4 * (p0 - 1) + 3},
        synth.GATE_BASE_SUM: {"sum": 0, "limb": p0},
        synth.GATE_ARITHMETIC_EXTENSION: {"multiplicand": 8 * (p0 - 1) + 1, "addend": 8 * (p0 - 1) + 5, "output": 8 * (p0 - 1) + 6},
        synth.GATE_MUL_EXTENSION: {"multiplicand": 6 * (p0 - 1) + 2, "output": 6 * (p0 - 1) + 5},
        synth.GATE_REDUCING: {"alpha": 3, "coefficient": 6 + p0 - 1, "old accumulator": 4, "output": 0},
        synth.GATE_REDUCING_EXTENSION: {"alpha": 2, "coefficient": 6 + 2 * (p0 - 1) + 1, "accumulator": 6 + 2 * p0, "output": 1},
        synth.GATE_POSEIDON: {"input": 3, "output": lg.POS_OUT + 5, "swap": lg.POS_SWAP, "delta": lg.POS_DELTA + 1, "first full S-box": lg.POS_FULL0 + 13,
                              "partial S-box": lg.POS_PARTIAL + 10, "last full S-box": lg.POS_WIRES - 1},
        synth.GATE_U32_INTERLEAVE: {"input": 2 * (p0 - 1), "output": 2 * (p0 - 1) + 1, "bit": 34 * p0 - 1},
        synth.GATE_UNINTERLEAVE_U32: {"input": 3 * (p0 - 1), "evens": 3 * (p0 - 1) + 1, "odds": 3 * (p0 - 1) + 2, "bit": 67 * p0 - 1},
        synth.GATE_UNINTERLEAVE_B32: {"input": 3 * (p0 - 1), "evens": 3 * (p0 - 1) + 1, "odds": 3 * (p0 - 1) + 2, "bit": 67 * p0 - 2},
        synth.GATE_U32_ARITHMETIC: {"multiplicand": 6 * (p0 - 1) + 1, "addend": 6 * (p0 - 1) + 2, "output low": 6 * (p0 - 1) + 3,
                                    "output high": 6 * (p0 - 1) + 4, "inverse": 5, "limb": 38 * p0 - 1},
        synth.GATE_U32_ADD_MANY: {"addend": na * (p1 - 1), "carry in": na * (p1 - 1) + p0, "result": na * (p1 - 1) + p0 + 1,
                                  "carry out": na * p1 - 1, "result limb": na * p1 + 3, "carry limb": (na + 18) * p1 - 1},
        synth.GATE_U32_SUBTRACTION: {"x": 5 * (p0 - 1), "borrow in": 5 * (p0 - 1) + 2, "result": 3, "borrow out": 5 * (p0 - 1) + 4, "limb": 21 * p0 - 1},
        synth.GATE_U32_RANGE_CHECK: {"input": p0 - 1, "limb": 17 * p0 - 1},
    }[t]


EXACT = {name: make for name, make in CLEAN.items() if not name.endswith("-zk")}            # every family without blinding rows


@pytest.mark.parametrize("name", sorted(EXACT))
def test_reports_equal_the_restatement(ctx, name):
    desc = EXACT[name]()
    gc = glp.Circuit(ctx, desc)
    sm = wr.decode_sigmas(desc)
    cases = []
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        if t == synth.GATE_NOOP:
            continue
        assert t in wr.HAS_BODY
        r = int(zr.gate_rows(desc, gi)[-1])
        for role, col in sorted(_roles(desc, t, g).items()):
            W = desc.wires.copy()
            _bump(W, col, r, 1 + len(cases))
            cases.append((t, role, W))
    pis = np.tile(np.asarray(desc.public_inputs, np.uint64), (len(cases), 1))          # zkdsa has public inputs: one set per member
    got = gc.check_witness(np.stack([W for _, _, W in cases]), public_inputs=pis, by_gate=True)         # every case a member of one call
    for (t, role, W), rep_gpu in zip(cases, got):
        rep, by_gate = wr.check(desc, W, sigma_map=sm)
        assert rep["failed_constraints"] >= 1, (t, role)
        _same(rep_gpu, rep, by_gate)
    gc.free()


def test_exact_reports_cover_every_restated_type():
    seen = {int(g["type"]) for name in EXACT for g in EXACT[name]().gates}
    assert seen == set(wr.HAS_BODY) == ALL_TYPES, sorted(ALL_TYPES - seen)


# ---------------------------------------------------------------------------------------------------- 3. the limb gates, against the oracle
OTHER = set(lg.LIMB_GATES)            # the types the oracle campaign judges (the restatement had no body for them when it was written)


def gate_width(t, p0, p1):
    """wire columns a gate of the types below constrains, from the gates' definitions (include/glp.h GLP_GATE_*)"""
    cb = -(-p0 // p1) if t == synth.GATE_COMPARISON else 0
    return {synth.GATE_POSEIDON: 135, synth.GATE_U32_INTERLEAVE: 34 * p0, synth.GATE_UNINTERLEAVE_U32: 67 * p0, synth.GATE_UNINTERLEAVE_B32: 67 * p0,
            synth.GATE_U32_ARITHMETIC: 38 * p0, synth.GATE_U32_ADD_MANY: (p0 + 3 + 18) * p1, synth.GATE_U32_SUBTRACTION: 21 * p0,
            synth.GATE_U32_RANGE_CHECK: 17 * p0, synth.GATE_COMPARISON: 4 + 5 * p1 + cb + 1,
            synth.GATE_RANDOM_ACCESS: (2 + (1 << p0) + p0) * (p1 & 0xFFFF) + (p1 >> 16)}[t]


CAMPAIGN = {"ecdsa": lambda: synth.ecdsa_shape_circuit(5), "keccak": lambda: synth.keccak_shape_circuit(5),
            "poseidon-chain": lambda: synth.poseidon_chain_circuit(2)}
CAMPAIGN_SEED, CAMPAIGN_DRAWS = 2, 8


def campaign(desc, seed=CAMPAIGN_SEED, draws=CAMPAIGN_DRAWS):
    """[(gate index, row, column)]: per gate of a type in OTHER, `draws` single cells on its rows.  Five columns
    are drawn over the whole width of the trace, three over the advice columns the gate leaves unused where it leaves any (a gate as
    wide as the trace -- PoseidonGate at 135 wires, U32RangeCheckGate with 8 limbs at 136 -- constrains every cell of its rows)."""
    rng = np.random.default_rng(seed)
    nw = int(desc.num_wires)
    out = []
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        if t not in OTHER:
            continue
        rows = zr.gate_rows(desc, gi)
        width = gate_width(t, int(g["p0"]), int(g["p1"]))
        assert width <= nw
        for k in range(draws):
            lo = width if k >= 5 and width < nw else 0
            out.append((gi, int(rows[rng.integers(0, len(rows))]), int(rng.integers(lo, nw))))
    return out


def oracle_verdicts(oracle, desc, cells):
    """True per cell iff the oracle's proof of the witness with that cell changed is accepted by the oracle's verifier.  The judge
    proves the same circuit with proof_of_work_bits = 0: the grinding is most of a small proof's time and judges nothing here."""
    d = copy.copy(desc)
    d.proof_of_work_bits = 0
    oc = oracle.OracleCircuit(d)
    out = []
    for gi, r, c in cells:
        W = desc.wires.copy()
        _bump(W, c, r)
        rc, proof = oc.prove(wires=W)
        assert rc == 0
        out.append(oc.verify(proof) == 0)
    return out


def both_verdicts_reached(desc, cells, verdicts):
    """per gate type of the campaign (OTHER) that leaves a column unused: accepted and rejected both occur"""
    nw = int(desc.num_wires)
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        if t not in OTHER:
            continue
        seen = {v for (gj, _, _), v in zip(cells, verdicts) if gj == gi}
        want = {True, False} if gate_width(t, int(g["p0"]), int(g["p1"])) < nw else {False}
        assert seen == want, "gate %d (type %d): verdicts %s, wanted %s" % (gi, t, sorted(seen), sorted(want))




@pytest.mark.parametrize("name", sorted(CAMPAIGN))
def test_campaign_against_the_oracle(ctx, oracle, name):
    desc = CAMPAIGN[name]()
    cells = campaign(desc)
    verdicts = oracle_verdicts(oracle, desc, cells)
    both_verdicts_reached(desc, cells, verdicts)
    gc = glp.Circuit(ctx, desc)
    sm = wr.decode_sigmas(desc)
    Ws = []
    for gi, r, c in cells:
        W = desc.wires.copy()
        _bump(W, c, r)
        Ws.append(W)
    for k0 in range(0, len(Ws), 16):
        reps = gc.check_witness(np.stack(Ws[k0:k0 + 16]), by_gate=True)
        for k, ((gi, r, c), ok, rep) in enumerate(zip(cells[k0:k0 + 16], verdicts[k0:k0 + 16], reps), k0):
            assert rep.ok == ok, "gate %d row %d column %d: oracle %s, checker: %s" % (gi, r, c, "accepts" if ok else "rejects", rep)
            if rep.ok:
                continue
            g = desc.gates[gi]
            assert rep.failed_rows <= 1
            if rep.failed_constraints:
                assert rep.row == r and rep.gate == gi and rep.constraint < int(g["num_constraints"]) and 0 < rep.value < P
                assert rep.rows_failed_by_gate == [1 if i == gi else 0 for i in range(len(desc.gates))]
            else:
                assert rep.failed_copies and r in (rep.copy_row, rep.to_row)
            if rep.failed_copies:                       # the copies are the restatement's business whatever the gate
                want = wr.check(desc, Ws[k], sigma_map=sm)[0]
                assert rep.as_tuple()[2:3] + rep.as_tuple()[7:] == wr.as_tuple(want)[2:3] + wr.as_tuple(want)[7:]
    gc.free()


def test_campaign_covers_the_other_types():
    """every limb gate type is on a row of one of the three circuits (and both_verdicts_reached has seen the checker reject a change on
    it)"""
    seen = {int(g["type"]) for name in CAMPAIGN for g in CAMPAIGN[name]().gates}
    assert seen & OTHER == OTHER == {4, 5, 6, 7, 8, 9, 10, 11, 12, 14} and len(campaign(CAMPAIGN["ecdsa"]())) == 6 * CAMPAIGN_DRAWS


# ---------------------------------------------------------------------------------------------------- 4. copies
def test_one_changed_cell_of_a_copy_cycle(ctx):
    desc = synth.arith_circuit(3, **ARITH3)
    gc = glp.Circuit(ctx, desc)
    sm = wr.decode_sigmas(desc)
    gi = _gate_of_type(desc, synth.GATE_ARITHMETIC)
    r = int(zr.gate_rows(desc, gi)[1])
    W = desc.wires.copy()
    _bump(W, 1, r)                                    # column 1 of the arithmetic rows is one cycle over all of them
    rep, by_gate = wr.check(desc, W, sigma_map=sm)
    assert rep["failed_copies"] == 2
    _same(gc.check_witness(W, by_gate=True), rep, by_gate)
    gc.free()


def _recoset(desc, k_is):
    """the same circuit over other coset shifts: sigma(j, i) = k_is[j'] w^i' rewritten"""
    d = copy.copy(desc)
    sm = wr.decode_sigmas(desc)
    lg = int(desc.degree_bits)
    w = wr.root_of_unity(lg)
    d.k_is = np.asarray(k_is, np.uint64)
    d.sigmas = np.array(desc.sigmas, np.uint64)
    for (j, i), (j2, i2) in sm.items():
        d.sigmas[j, i] = int(k_is[j2]) * pow(w, i2, P) % P
    d.circuit_digest = np.zeros(4, np.uint64)
    return d


def test_arbitrary_coset_shifts_and_a_sigma_on_no_coset(ctx):
    base = synth.arith_circuit(4)
    k_is = pr.synthetic(4, 80, 80, 8, 2, seed=5).k_is          # distinct cosets, not powers of 7: k_ratio == 0
    assert int(k_is[2]) != int(k_is[1]) ** 2 % P
    desc = _recoset(base, k_is)
    gc = glp.Circuit(ctx, desc)
    assert gc.check_witness().ok
    sm = wr.decode_sigmas(desc)
    gi = _gate_of_type(desc, synth.GATE_ARITHMETIC)
    r = int(zr.gate_rows(desc, gi)[3])
    W = desc.wires.copy()
    _bump(W, 1, r)
    rep, by_gate = wr.check(desc, W, sigma_map=sm)
    assert rep["failed_copies"] == 2
    _same(gc.check_witness(W, by_gate=True), rep, by_gate)
    gc.free()
    # one sigma word on no coset: a malformed circuit, refused by name
    n = 1 << 4
    cosets = {pow(int(k), n, P) for k in k_is}
    x = next(v for v in range(3, 100) if pow(v, n, P) not in cosets)
    bad = copy.copy(desc)
    bad.sigmas = desc.sigmas.copy()
    bad.sigmas[7, 11] = x
    gc = glp.Circuit(ctx, bad)
    with pytest.raises(glp.GlpError, match=r"sigmas\[7\]\[11\]") as e:
        gc.check_witness()
    assert e.value.code == -1
    with pytest.raises(glp.GlpError, match=r"sigmas\[7\]\[11\]"):       # and again: a refused decode is not kept with the circuit
        gc.check_witness()
    gc.free()


# ---------------------------------------------------------------------------------------------------- 5. more than one workgroup
@pytest.fixture(scope="module")
def arith10(ctx):
    desc = synth.arith_circuit(10, num_noop_rows=0)          # ArithmeticGate rows up to row 1023: four workgroups of 256 rows
    gc = glp.Circuit(ctx, desc)
    yield desc, gc, wr.decode_sigmas(desc)
    gc.free()


@pytest.mark.parametrize("rows", [(1023,), (700, 300), (255, 256)])
@pytest.mark.parametrize("col", ["output", "cycle"])
def test_failures_across_workgroups(arith10, rows, col):
    desc, gc, sm = arith10
    gi = _gate_of_type(desc, synth.GATE_ARITHMETIC)
    ops = int(desc.gates[gi]["p0"])
    c = 4 * (ops - 1) + 3 if col == "output" else 1          # the last output feeds nothing; column 1 is a copy cycle over the rows
    W = desc.wires.copy()
    for r in rows:
        assert int(desc.constants[int(desc.gates[gi]["selector_index"]), r]) == gi
        _bump(W, c, r)
    rep, by_gate = wr.check(desc, W, sigma_map=sm)
    assert (rep["failed_rows"], rep["row"]) == (len(rows), min(rows)) and rep["failed_constraints"] == len(rows)
    if col == "output":
        assert rep["failed_copies"] == 0
    else:                                             # a changed cell against its image and the cell it is the image of; changed neighbours agree
        assert len(rows) <= rep["failed_copies"] <= 2 * len(rows) and rep["copy_row"] <= min(rows)
    _same(gc.check_witness(W, by_gate=True), rep, by_gate)


# ---------------------------------------------------------------------------------------------------- 6. K = 3 in one call
def test_three_witnesses_in_one_call(ctx):
    desc = synth.ecdsa_shape_circuit(5)
    gc = glp.Circuit(ctx, desc)
    W = np.stack([desc.wires, desc.wires, desc.wires])
    gi = _gate_of_type(desc, synth.GATE_U32_ARITHMETIC)
    _bump(W[1], 3, int(zr.gate_rows(desc, gi)[0]))
    three = gc.check_witness(W, by_gate=True)
    alone = [gc.check_witness(W[k], by_gate=True) for k in range(3)]
    assert [r.ok for r in three] == [True, False, True]
    for a, b in zip(three, alone):
        assert a.as_tuple() == b.as_tuple() and a.rows_failed_by_gate == b.rows_failed_by_gate
    assert three[1].gate == gi and three[1].gate_type == synth.GATE_U32_ARITHMETIC and "U32ArithmeticGate" in str(three[1])
    gc.free()


# ---------------------------------------------------------------------------------------------------- 7. public inputs
def test_one_wrong_public_input(ctx, oracle):
    pi = [3, 1 << 40, 5]
    desc = synth.arith_circuit(3, public_inputs=pi, pi_hash=oracle.hash_no_pad(pi), **ARITH3)
    gc = glp.Circuit(ctx, desc)
    assert gc.check_witness().ok
    rep = gc.check_witness(public_inputs=[3, (1 << 40) + 1, 5], by_gate=True)
    gi = _gate_of_type(desc, synth.GATE_PUBLIC_INPUT)
    assert (rep.failed_constraints, rep.failed_rows, rep.failed_copies, rep.row, rep.gate, rep.constraint) == (4, 1, 0, 0, gi, 0)
    assert rep.rows_failed_by_gate == [1 if i == gi else 0 for i in range(len(desc.gates))]
    want, by_gate = wr.check(desc, public_inputs=[3, (1 << 40) + 1, 5])
    _same(rep, want, by_gate)
    gc.free()


# ---------------------------------------------------------------------------------------------------- 8. with the GPU generators
@pytest.mark.parametrize("name,gate,col", [("u32", synth.GATE_U32_INTERLEAVE, 0), ("poseidon-chain", synth.GATE_POSEIDON, 0)])
def test_routed_columns_filled_on_the_gpu(ctx, name, gate, col):
    desc = CLEAN[name]()
    gc = glp.Circuit(ctx, desc)
    nr = int(desc.num_routed_wires)
    gi = _gate_of_type(desc, gate)
    r = int(zr.gate_rows(desc, gi)[0])
    d = ctx.dev_alloc(desc.wires.nbytes)
    for change in (False, True):
        W = desc.wires.copy()
        W[nr:] = 0                                     # only the routed columns travel
        if change:
            _bump(W, col, r)                           # a routed input of a generator: its routed outputs no longer follow from it
        ctx.dev_upload(d, np.ascontiguousarray(W))
        gc.witness_fill(d, only_advice=True)
        rep = gc.check_witness(dev_wires_ptr=d, by_gate=True)
        if not change:
            assert rep.ok, str(rep)
        else:
            assert not rep.ok and rep.failed_constraints and (rep.row, rep.gate) == (r, gi), str(rep)
    ctx.dev_free(d)
    gc.free()


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(ctx):
    L = glp.load_library()
    desc = synth.zkdsa_circuit(3)                      # 12 public inputs
    gc = glp.Circuit(ctx, desc)
    W = np.ascontiguousarray(np.stack([desc.wires, desc.wires]))
    pi = np.ascontiguousarray(np.stack([desc.public_inputs, desc.public_inputs]).astype(np.uint64))
    reps = (binding._WitnessReport * 2)()
    wp, pp = W.ctypes.data_as(C.c_void_p), pi.ctypes.data_as(C.c_void_p)

    def refused(needle, *args):
        assert L.glp_witness_check(*args) == -1
        assert needle in L.glp_last_error().decode(), L.glp_last_error().decode()
    assert L.glp_witness_check(ctx._h, gc._h, 2, wp, 0, pp, reps, None) == 0 and not reps[0].failed_constraints and not reps[1].failed_copies
    refused("ctx is null", None, gc._h, 2, wp, 0, pp, reps, None)
    refused("circuit is null", ctx._h, None, 2, wp, 0, pp, reps, None)
    refused("wires is null", ctx._h, gc._h, 2, None, 0, pp, reps, None)
    refused("reports_out is null", ctx._h, gc._h, 2, wp, 0, pp, None, None)
    refused("public_inputs is null", ctx._h, gc._h, 2, wp, 0, None, reps, None)
    refused("num_proofs = 0", ctx._h, gc._h, 0, wp, 0, pp, reps, None)
    refused("num_proofs = 4097", ctx._h, gc._h, 4097, wp, 0, pp, reps, None)
    word = W[0].size + 5 * W.shape[2] + 3              # proof 1, column 5, row 3
    for v in (P, (1 << 64) - 1):
        keep = int(W[1, 5, 3])
        W[1, 5, 3] = v
        refused("wires: proof 1, word %d = 0x%016x" % (word - W[0].size, v), ctx._h, gc._h, 2, wp, 0, pp, reps, None)
        W[1, 5, 3] = keep
        keep = int(pi[1, 7])
        pi[1, 7] = v
        refused("public_inputs: proof 1, word 7 = 0x%016x" % v, ctx._h, gc._h, 2, wp, 0, pp, reps, None)
        pi[1, 7] = keep
    assert L.glp_witness_check(ctx._h, gc._h, 2, wp, 0, pp, reps, None) == 0 and not reps[1].failed_constraints
    gc.free()


# ---------------------------------------------------------------------------------------------------- 10. non-interference
def test_check_leaves_proofs_and_witness_alone(ctx):
    desc = synth.arith_circuit(5)
    gc = glp.Circuit(ctx, desc)
    before = gc.prove()
    bad = desc.wires.copy()
    _bump(bad, 1, 9)
    assert not gc.check_witness(bad).ok and gc.check_witness().ok
    assert (gc.prove() == before).all()
    W = np.ascontiguousarray(desc.wires.copy())
    assert int(W[0, 0]) == 0                           # the public-input hash of no public inputs
    W[0, 0] = P                                        # a device word >= p is reduced as it is loaded: p is 0
    d = ctx.dev_alloc(W.nbytes)
    ctx.dev_upload(d, W)
    assert gc.check_witness(dev_wires_ptr=d).ok
    back = np.empty_like(W)
    ctx.dev_download(d, back)
    assert back.tobytes() == W.tobytes()
    W[0, 0] = 0
    _bump(W, 1, 9)
    ctx.dev_upload(d, W)
    rep = gc.check_witness(dev_wires_ptr=d)
    assert rep.as_tuple() == gc.check_witness(W).as_tuple() and not rep.ok
    ctx.dev_download(d, back)
    assert back.tobytes() == W.tobytes()
    ctx.dev_free(d)
    gc.free()


# ---------------------------------------------------------------------------------------------------- 11. the hand-off file tool
def test_check_glpc_on_the_golden_file(ctx, tmp_path):
    import io
    import os
    from plonky2_lib_amd.tools import check_glpc
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zkdsa_2_3_v2.glpc")
    out = io.StringIO()
    assert check_glpc.check_file(golden, out=out) is True and "witness satisfies the circuit" in out.getvalue()
    out = io.StringIO()
    assert check_glpc.check_file(golden, refill=True, out=out) is True
    assert check_glpc.main([golden]) == 0
    # one wire word of a copy of the file changed, the file rewritten through glp_circuit_file_write: that row and its gate are named
    with glp.CircuitFile(golden) as cf:
        d = copy.copy(cf.desc)
        d.wires = np.array(cf.desc.wires, np.uint64)
        d.public_inputs = np.array(cf.desc.public_inputs, np.uint64)
        gi = _gate_of_type(d, synth.GATE_POSEIDON)
        r = int(zr.gate_rows(d, gi)[1])
        _bump(d.wires, 100, r)                       # an S-box input of the last full rounds: an advice wire, in no copy
        path = str(tmp_path / "changed.glpc")
        glp.write_circuit_file(path, d)
    out = io.StringIO()
    assert check_glpc.check_file(path, out=out) is False
    text = out.getvalue()
    assert "row %d: gate %d (PoseidonGate) constraint" % (r, gi) in text and "1 of its" in text, text
    assert check_glpc.main([path]) == 1
    assert check_glpc.main([str(tmp_path / "missing.glpc")]) == 2
