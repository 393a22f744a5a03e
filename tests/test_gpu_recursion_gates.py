"""The recursion gates (ExponentiationGate, CosetInterpolationGate, PoseidonMdsGate) through every GPU entry point: glp_prove,
glp_prove_device, the stepped session, glp_prove_batch (host and device transcripts, host and device wires), glp_witness_fill, the
staged witness, glp_verify, glp_verify_batch, under both hashers and with zero knowledge.  The oracle cannot evaluate these gates, so
the independent check is tests/zeta_identity_recursion.py (pinned to the oracle by tests/test_recursion_gates.py)."""
import os

import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
import zeta_identity as zi
import zeta_identity_recursion as zr

pytestmark = pytest.mark.gpu

P = zi.P
EXP, COSET, MDS = synth.GATE_EXPONENTIATION, synth.GATE_COSET_INTERPOLATION, synth.GATE_POSEIDON_MDS
PRESETS = {"rec": synth.Config.standard_recursion_config, "ecc": synth.Config.standard_ecc_config}
SETS = {"exp": (EXP,), "coset": (COSET,), "mds": (MDS,), "all": synth.RECURSION_GATES}
PARAMS = {
    "default": None,
    "n2": {COSET: (1, 2), EXP: (1, 0)},
    "d8": {COSET: (4, 8), EXP: (7, 0)},
    "odd": {COSET: (3, 3), EXP: (63, 0)},
}
CATEGORIES = ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q")


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _last_error():
    return glp.load_library().glp_last_error().decode()


def _prove_and_check(ctx, desc, hasher=0):
    desc.hasher = hasher
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    assert gc.verify(proof), _last_error()
    assert gc.verify_batch(proof[None, :]).all()
    assert zr.check(desc, proof, gc.digest(), hasher)
    return gc, proof


def _gate_index(desc, t):
    return next(i for i, g in enumerate(desc.gates) if int(g["type"]) == t)


# ---------------------------------------------------------------------------------------------------- 1. prove / verify / checker
@pytest.mark.parametrize("lg", [3, 5, 8, 12, 16])
@pytest.mark.parametrize("hasher", [0, 1])
def test_prove_verify_check(ctx, oracle, lg, hasher):
    """each gate alone, all three, and all three mixed with the ext gates; both presets alternate with the size"""
    preset = "rec" if lg % 2 else "ecc"
    for name, gates in list(SETS.items()) + [("mixed", synth.RECURSION_GATES)]:
        mixed = name == "mixed"
        if mixed and lg < 4:
            continue
        pi = [lg, 1 << 33, hasher] if mixed else []
        desc = synth.recursion_gates_circuit(lg, PRESETS[preset](), seed=lg + 17 * hasher, gates=gates, mix_ext=mixed,
                                             public_inputs=pi, pi_hash=oracle.hash_no_pad(pi) if pi else None)
        gc, _ = _prove_and_check(ctx, desc, hasher)
        gc.free()


@pytest.mark.parametrize("name", ["n2", "d8", "odd"])
def test_parameter_sets(ctx, name):
    for lg, preset in ((4, "rec"), (9, "ecc")):
        desc = synth.recursion_gates_circuit(lg, PRESETS[preset](), seed=5, params=PARAMS[name], mix_ext=True)
        gc, _ = _prove_and_check(ctx, desc)
        gc.free()


# ---------------------------------------------------------------------------------------------------- 2. tampering
def test_tampered_openings_are_rejected(ctx):
    desc = synth.recursion_gates_circuit(6, PRESETS["rec"](), seed=8, mix_ext=True)
    gc, proof = _prove_and_check(ctx, desc)
    lay = zi.proof_layout(desc)
    bad = []
    for name in CATEGORIES:
        o, _ = lay[name]
        p = proof.copy()
        p[o] = (int(p[o]) + 1) % P
        assert not gc.verify(p), name
        assert not zr.check(desc, p, gc.digest()), name
        bad.append(p)
    assert not gc.verify_batch(np.stack(bad)).any()
    gc.free()


def _broken_columns(desc, t, g):
    p0, p1 = int(g["p0"]), int(g["p1"])
    if t == EXP:
        return [(p0 + 2 + p0 // 2, "intermediate"), (p0 + 1, "output"), (2 * p0 + 1, "last intermediate")]
    if t == MDS:
        return [(24, "output 0.0"), (47, "output 11.1")]
    lay = zr.coset_layout(p0, p1)
    return [(lay["value"], "evaluation value"), (lay["evals"] + 1, "intermediate eval"), (lay["prods"] + 2 * lay["ni"] - 1, "intermediate prod"),
            (lay["shifted"], "shifted point")]


@pytest.mark.parametrize("t", synth.RECURSION_GATES)
def test_broken_constraint_is_rejected(ctx, t):
    desc = synth.recursion_gates_circuit(6, PRESETS["rec"](), seed=21)
    gc = glp.Circuit(ctx, desc)
    dig = gc.digest()
    gi = _gate_index(desc, t)
    row = int(zr.gate_rows(desc, gi)[-1])
    batch = []
    for col, what in _broken_columns(desc, t, desc.gates[gi]):
        w = desc.wires.copy()
        w[col, row] = (int(w[col, row]) + 1) % P
        assert any(zr.row_constraints(desc, gi, row, wires=w)), what
        proof = gc.prove(wires=w)
        assert not gc.verify(proof), what
        assert not zr.check(desc, proof, dig), what
        batch.append(proof)
    assert not gc.verify_batch(np.stack(batch)).any()
    gc.free()


# ---------------------------------------------------------------------------------------------------- 3. path equality
def _all_paths_equal(ctx, oracle, desc, K=3):
    """glp_prove == glp_prove_device == stepped session == members of glp_prove_batch (host / device transcripts, host / device wires)"""
    from test_gpu_prove import _stepped_proof
    gc = glp.Circuit(ctx, desc)
    desc.circuit_digest = gc.digest()
    ref = gc.prove()
    assert gc.verify(ref) and zr.check(desc, ref, gc.digest(), int(getattr(desc, "hasher", 0)))
    w = np.ascontiguousarray(desc.wires)
    dp = ctx.dev_alloc(w.nbytes)
    try:
        ctx.dev_upload(dp, w)
        dev = gc.prove_device(dp)
    finally:
        ctx.dev_free(dp)
    assert (dev == ref).all(), "device: first mismatch at word %d" % int(np.argmax(dev != ref))
    got = _stepped_proof(gc, oracle, desc)
    assert (got == ref).all(), "session: first mismatch at word %d" % int(np.argmax(got != ref))
    wires = np.stack([w] * K)
    pis = np.stack([np.asarray(desc.public_inputs, np.uint64)] * K)
    if int(desc.num_challenges) != 2:
        # glp_prove_batch exists for two challenges only (batch_check in csrc/prover_stages.inc, whatever the gates): there is no batch
        # proof to compare, so what is pinned is the refusal.  prove, device and session above all went through k_quotient<NCH, 1>.
        with pytest.raises(glp.GlpError) as e:
            gc.prove_batch(wires, pis)
        assert e.value.code == -1 and "num_challenges" in str(e.value)
        gc.free()
        return
    for host_transcript in (False, True):
        if host_transcript:
            os.environ["GLP_BATCH_HOST_TRANSCRIPT"] = "1"
        try:
            proofs = gc.prove_batch(wires, pis)
            dptr = ctx.dev_alloc(wires.nbytes)
            try:
                ctx.dev_upload(dptr, wires)
                devb = gc.prove_batch_device(dptr, K, pis)
            finally:
                ctx.dev_free(dptr)
        finally:
            os.environ.pop("GLP_BATCH_HOST_TRANSCRIPT", None)
        for k in range(K):
            assert (proofs[k] == ref).all(), (host_transcript, k, int(np.argmax(proofs[k] != ref)))
            assert (devb[k] == ref).all(), (host_transcript, k, int(np.argmax(devb[k] != ref)))
    assert gc.verify_batch(proofs).all()
    gc.free()


@pytest.mark.parametrize("lg,preset,nch", [(4, "rec", 2), (10, "ecc", 2), (5, "rec", 1), (7, "ecc", 3)])
def test_paths_agree(ctx, oracle, lg, preset, nch):
    """num_challenges 2 takes the per-gate launches, 1 and 3 the monolithic kernel (for which the library has no batch path)"""
    pi = [7, 8, lg]
    desc = synth.recursion_gates_circuit(lg, PRESETS[preset](), seed=3 + nch, num_challenges=nch, mix_ext=True, public_inputs=pi,
                                         pi_hash=oracle.hash_no_pad(pi))
    _all_paths_equal(ctx, oracle, desc)


def test_batch_of_different_witnesses(ctx):
    K = 5
    descs = [synth.recursion_gates_circuit(5, PRESETS["rec"](), seed=5, witness_seed=100 + k) for k in range(K)]
    gc = glp.Circuit(ctx, descs[0])
    wires = np.stack([d.wires for d in descs])
    proofs = gc.prove_batch(wires)
    for k in range(K):
        single = gc.prove(wires=wires[k])
        assert (proofs[k] == single).all(), (k, int(np.argmax(proofs[k] != single)))
        assert zr.check(descs[k], proofs[k], gc.digest())
    assert not (proofs[0] == proofs[1]).all()
    assert gc.verify_batch(proofs).all()
    gc.free()


# ---------------------------------------------------------------------------------------------------- 4. zero knowledge
def test_zero_knowledge(ctx):
    desc = synth.recursion_gates_circuit(5, synth.Config.standard_recursion_zk_config(), seed=6, mix_ext=True)
    assert desc.zero_knowledge and desc.degree_bits > 5
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    assert gc.verify(proof), _last_error()
    assert gc.verify_batch(proof[None, :]).all()
    gc.free()


# ---------------------------------------------------------------------------------------------------- 5. witness fill
def _expected_roles(t, g, nw):
    p0, p1 = int(g["p0"]), int(g["p1"])
    role = np.zeros(nw, np.uint8)
    if t == EXP:
        role[0:p0 + 1] = 2
        role[p0 + 1:2 * p0 + 2] = 1
    elif t == MDS:
        role[0:24] = 2
        role[24:48] = 1
    else:
        lay = zr.coset_layout(p0, p1)
        role[0:lay["value"]] = 2
        role[lay["value"]:lay["wires"]] = 1
    return role


@pytest.mark.parametrize("name", ["default", "odd"])
def test_witness_fill(ctx, name):
    desc = synth.recursion_gates_circuit(7, PRESETS["rec"](), seed=31, params=PARAMS[name])
    gc = glp.Circuit(ctx, desc)
    honest = np.ascontiguousarray(desc.wires).copy()
    nr = desc.num_routed_wires
    zeroed = honest.copy()
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        if t not in synth.RECURSION_GATES:
            continue
        role = gc.witness_columns(gi)
        assert (role == _expected_roles(t, g, desc.num_wires)).all(), t
        zeroed[np.ix_(np.nonzero(role == 1)[0], zr.gate_rows(desc, gi))] = 0
    assert (zeroed != honest).any()
    ref = gc.prove()
    for only_advice in (False, True):
        d = ctx.dev_alloc(zeroed.nbytes)
        try:
            ctx.dev_upload(d, zeroed)
            gc.witness_fill(d, only_advice=only_advice)
            got = np.empty_like(zeroed)
            ctx.dev_download(d, got)
            if not only_advice:
                assert (got == honest).all(), np.argwhere(got != honest)[:4].tolist()
                assert (gc.prove_device(d) == ref).all()
            else:
                assert (got[:nr] == zeroed[:nr]).all()                        # routed columns untouched
                assert (got[nr:] == honest[nr:]).all()                        # the advice intermediates restored
        finally:
            ctx.dev_free(d)
    # a witness staged with its routed columns only: the advice columns are derived on the GPU
    w0 = honest.copy()
    w0[nr:] = 0
    d = ctx.dev_alloc(w0.nbytes)
    try:
        ctx.dev_upload(d, w0)
        gc.witness_fill(d, only_advice=True)
        resident = gc.prove_device(d)
    finally:
        ctx.dev_free(d)
    pinned = ctx.host_alloc((nr, 1 << desc.degree_bits))
    pinned[:] = honest[:nr]
    st = gc.stage_witness(pinned, routed_only=True)
    staged = gc.prove_staged(st)
    st.free()
    ctx.host_free(pinned)
    assert (staged == resident).all() and gc.verify(staged) and zr.check(desc, staged, gc.digest())
    gc.free()


# ---------------------------------------------------------------------------------------------------- 6. creation
def _create_error(ctx, desc, fragment=None):
    with pytest.raises(glp.GlpError) as e:
        glp.Circuit(ctx, desc)
    if fragment is not None:
        assert fragment in str(e.value), str(e.value)
    return e.value.code


def test_bad_descriptions(ctx):
    def fresh(cfg=None, gates=synth.RECURSION_GATES, params=None):
        return synth.recursion_gates_circuit(4, cfg or PRESETS["rec"](), seed=2, gates=gates, params=params)

    def gate(desc, t):
        return next(g for g in desc.gates if int(g["type"]) == t)
    unsupported = "is not supported"
    d = fresh()                                   # a parameter of 0
    g = gate(d, EXP); g["p0"] = 0; g["num_constraints"] = 1
    assert _create_error(ctx, d, unsupported) == -1
    d = fresh()
    g = gate(d, COSET); g["p0"] = 0
    assert _create_error(ctx, d, unsupported) == -1
    d = fresh()                                   # d < 2
    gate(d, COSET)["p1"] = 1
    assert _create_error(ctx, d, unsupported) == -1
    d = fresh()
    gate(d, COSET)["p1"] = 0
    assert _create_error(ctx, d, unsupported) == -1
    d = fresh()                                   # d > N = 16
    g = gate(d, COSET); g["p1"] = 17; g["num_constraints"] = 4
    assert _create_error(ctx, d, unsupported) == -1
    d = fresh()                                   # 64 points: beyond the 32-entry table
    gate(d, COSET)["p0"] = 6
    assert _create_error(ctx, d, unsupported) == -1
    d = fresh()                                   # PoseidonMdsGate takes no parameters
    gate(d, MDS)["p0"] = 1
    assert _create_error(ctx, d, unsupported) == -1
    d = fresh()                                   # 67 power bits: 136 wires > 135
    g = gate(d, EXP); g["p0"] = 67; g["num_constraints"] = 68; d.num_gate_constraints = 68
    assert _create_error(ctx, d, "wires") == -1
    d = fresh()                                   # 32 points at degree 2: 7 + 64 + 4 * 30 = 191 wires > 135
    g = gate(d, COSET); g["p0"] = 5; g["p1"] = 2; g["num_constraints"] = 124; d.num_gate_constraints = 124
    assert _create_error(ctx, d, "wires") == -1
    d = fresh(synth.Config(135, 40), gates=(EXP,), params={EXP: (30, 0)})      # 39 bits: 80 wires fit, 41 routed inputs > 40
    g = gate(d, EXP); g["p0"] = 39; g["num_constraints"] = 40; d.num_gate_constraints = 40
    assert _create_error(ctx, d, "routed") == -1
    d = fresh(synth.Config(135, 40), gates=(COSET,))                            # 32 points: 87 wires fit, 69 routed inputs > 40
    g = gate(d, COSET); g["p0"] = 5; g["p1"] = 8; g["num_constraints"] = 20; d.num_gate_constraints = 20
    assert _create_error(ctx, d, "routed") == -1
    d = fresh(synth.Config(135, 40), gates=(EXP,), params={EXP: (30, 0)})      # PoseidonMdsGate routes 48 wires > 40
    g = gate(d, EXP); g["type"] = MDS; g["p0"] = 0; g["num_constraints"] = 24
    assert _create_error(ctx, d, "routed") == -1
    for t in synth.RECURSION_GATES:               # a constraint count that disagrees with the parameters
        d = fresh()
        gate(d, t)["num_constraints"] += 1
        d.num_gate_constraints += 1
        assert _create_error(ctx, d, "num_constraints") == -1
    d = fresh()                                   # degree 8 next to ExponentiationGate under two selectors: 8 + 2 > 8 + 1
    g = gate(d, COSET)
    assert int(g["group_end"]) - int(g["group_start"]) == 2 and d.num_selectors == 2
    g["p1"] = 8                                   # still 2 intermediates: wires and constraint count do not change
    assert _create_error(ctx, d, "exceeds") == -1
    for t in (19, 23):
        d = fresh()
        gate(d, EXP)["type"] = t
        assert _create_error(ctx, d, unsupported) == -3
    gc = glp.Circuit(ctx, fresh())               # the unmodified description is accepted
    gc.free()


# ---------------------------------------------------------------------------------------------------- 7. full size
def test_full_size_mixed_circuit(ctx):
    desc = synth.recursion_gates_circuit(20, PRESETS["rec"](), seed=4, mix_ext=True)
    gc, proof = _prove_and_check(ctx, desc)
    gc.free()
