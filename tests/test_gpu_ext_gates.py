"""plonky2's extension-field gates (ArithmeticExtension, MulExtension, Reducing, ReducingExtension) through every GPU entry point:
glp_prove, the stepped session, glp_prove_batch (host and device wires), glp_witness_fill, glp_verify, glp_verify_batch, under both
hashers.  The oracle cannot evaluate these gates, so the independent check is tests/zeta_identity.py (pinned to the oracle by
tests/test_ext_gates.py)."""
import os

import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
import zeta_identity as zi

pytestmark = pytest.mark.gpu

PRESETS = {"rec": synth.Config.standard_recursion_config, "ecc": synth.Config.standard_ecc_config}
SETS = {"ae": (15,), "me": (16,), "red": (17,), "rex": (18,), "all": synth.EXT_GATES}
QUOTIENT_REASON = "Mismatch between evaluation and opening of quotient polynomial"


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
    assert zi.check(desc, proof, gc.digest(), hasher)
    return gc, proof


# ---------------------------------------------------------------------------------------------------- 1. prove / verify / checker
@pytest.mark.parametrize("lg", [3, 5, 7, 9, 12, 16])
@pytest.mark.parametrize("preset", sorted(PRESETS))
@pytest.mark.parametrize("nch", [2, 3])
def test_prove_verify_check(ctx, oracle, lg, preset, nch):
    for name, gates in SETS.items():
        pi = [lg, 1 << 33, nch] if name == "all" else []
        desc = synth.ext_gates_circuit(lg, PRESETS[preset](), seed=lg + 17 * nch, num_challenges=nch, gates=gates,
                                       public_inputs=pi, pi_hash=oracle.hash_no_pad(pi) if pi else None)
        gc, _ = _prove_and_check(ctx, desc)
        gc.free()


# ---------------------------------------------------------------------------------------------------- 2. stepped session
def test_stepped_session_equals_prove(ctx, oracle):
    from test_gpu_prove import _stepped_proof
    for lg, preset in ((5, "rec"), (10, "ecc")):
        pi = [7, 8]
        desc = synth.ext_gates_circuit(lg, PRESETS[preset](), seed=3, public_inputs=pi, pi_hash=oracle.hash_no_pad(pi))
        gc = glp.Circuit(ctx, desc)
        desc.circuit_digest = gc.digest()
        ref = gc.prove()
        got = _stepped_proof(gc, oracle, desc)
        assert (got == ref).all(), "first mismatch at word %d" % int(np.argmax(got != ref))
        assert gc.verify(got) and zi.check(desc, got, gc.digest())
        gc.free()


# ---------------------------------------------------------------------------------------------------- 3. batch prover / verifier
@pytest.mark.parametrize("lg,K", [(3, 4), (4, 64), (5, 4), (5, 64), (9, 4)])
def test_batch_equals_single(ctx, lg, K):
    cfg = PRESETS["rec" if lg % 2 else "ecc"]()
    descs = [synth.ext_gates_circuit(lg, cfg, seed=5, witness_seed=100 + k) for k in range(K)]
    gc = glp.Circuit(ctx, descs[0])
    wires = np.stack([d.wires for d in descs])
    proofs = gc.prove_batch(wires)
    for k in range(K):
        single = gc.prove(wires=wires[k])
        assert (proofs[k] == single).all(), (k, int(np.argmax(proofs[k] != single)))
    for k in (0, K - 1):
        assert zi.check(descs[k], proofs[k], gc.digest())
    # device-resident wires
    dptr = ctx.dev_alloc(wires.nbytes)
    ctx.dev_upload(dptr, np.ascontiguousarray(wires))
    dev = gc.prove_batch_device(dptr, K)
    ctx.dev_free(dptr)
    assert (dev == proofs).all()
    ok = gc.verify_batch(proofs)
    assert ok.all()
    os.environ["GLP_VERIFY_HOST_TRANSCRIPT"] = "1"
    try:
        ok_h = gc.verify_batch(proofs)
    finally:
        del os.environ["GLP_VERIFY_HOST_TRANSCRIPT"]
    assert ok_h.all()
    gc.free()


# ---------------------------------------------------------------------------------------------------- 4. KeccakGoldilocksConfig
def test_keccak_config(ctx, oracle):
    pi = [1, 2, 3]
    desc = synth.ext_gates_circuit(8, PRESETS["ecc"](), seed=9, public_inputs=pi, pi_hash=oracle.hash_no_pad(pi))
    gc, proof = _prove_and_check(ctx, desc, hasher=1)
    assert gc.verify_batch(proof[None, :]).all()
    gc.free()


# ---------------------------------------------------------------------------------------------------- 5. tampering
def _tamper_columns(t, p0):
    """(column, what) pairs: one constrained output / accumulator wire per component."""
    if t == 15:
        return [(6, "op0 out.0"), (8 * (p0 - 1) + 7, "last out.1")]
    if t == 16:
        return [(4, "op0 out.0"), (6 * (p0 - 1) + 5, "last out.1")]
    cw = 1 if t == 17 else 2
    return [(6 + cw * p0, "acc0.0"), (6 + cw * p0 + 1, "acc0.1"), (0, "output.0"), (1, "output.1")]


@pytest.mark.parametrize("t", synth.EXT_GATES)
def test_tampered_wire_is_rejected(ctx, t):
    desc = synth.ext_gates_circuit(6, PRESETS["rec"](), seed=21)
    gc = glp.Circuit(ctx, desc)
    dig = gc.digest()
    gi = next(i for i, g in enumerate(desc.gates) if int(g["type"]) == t)
    row = int(np.nonzero(desc.constants[0] == gi)[0][-1])
    batch = []
    for col, what in _tamper_columns(t, int(desc.gates[gi]["p0"])):
        w = desc.wires.copy()
        w[col, row] = (int(w[col, row]) + 1) % zi.P
        proof = gc.prove(wires=w)
        assert not gc.verify(proof), what
        assert QUOTIENT_REASON in _last_error(), (what, _last_error())
        assert not zi.check(desc, proof, dig), what
        batch.append(proof)
    ok, why = gc.verify_batch(np.stack(batch), reasons=True)
    assert not ok.any() and all(QUOTIENT_REASON in r for r in why), why
    gc.free()


# ---------------------------------------------------------------------------------------------------- 6. witness fill
def _expected_roles(t, p0, nw):
    role = np.zeros(nw, np.uint8)
    if t in (15, 16):
        st = 8 if t == 15 else 6
        for i in range(p0):
            role[st * i:st * i + st - 2] = 2
            role[st * i + st - 2:st * i + st] = 1
    else:
        cw = 1 if t == 17 else 2
        role[0:2] = 1
        role[2:6 + cw * p0] = 2
        role[6 + cw * p0:6 + cw * p0 + 2 * (p0 - 1)] = 1
    return role


@pytest.mark.parametrize("preset", sorted(PRESETS))
def test_witness_fill(ctx, preset):
    desc = synth.ext_gates_circuit(7, PRESETS[preset](), seed=31)
    gc = glp.Circuit(ctx, desc)
    honest = desc.wires.copy()
    nr = desc.num_routed_wires
    scrambled = honest.copy()
    rng = np.random.default_rng(5)
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        if t not in synth.EXT_GATES:
            continue
        role = gc.witness_columns(gi)
        assert (role == _expected_roles(t, int(g["p0"]), desc.num_wires)).all(), t
        rows = np.nonzero(desc.constants[0] == gi)[0]
        cols = np.nonzero(role == 1)[0]
        scrambled[np.ix_(cols, rows)] = synth.gl.rand(rng, (len(cols), len(rows)))
    assert (scrambled != honest).any()
    for only_advice in (False, True):
        d = ctx.dev_alloc(scrambled.nbytes)
        ctx.dev_upload(d, scrambled)
        gc.witness_fill(d, only_advice=only_advice)
        got = np.empty_like(scrambled)
        ctx.dev_download(d, got)
        if not only_advice:
            assert (got == honest).all(), np.argwhere(got != honest)[:4].tolist()
            proof = gc.prove_device(d)
            assert gc.verify(proof) and zi.check(desc, proof, gc.digest())
            assert (proof == gc.prove()).all()
        else:
            assert (got[:nr] == scrambled[:nr]).all()                     # routed columns untouched
            assert (got[nr:] == honest[nr:]).all()                        # advice outputs / accumulators restored
        ctx.dev_free(d)
    gc.free()


# ---------------------------------------------------------------------------------------------------- 7. bad descriptions
def _create_error(ctx, desc):
    with pytest.raises(glp.GlpError) as e:
        glp.Circuit(ctx, desc)
    return e.value.code


def test_bad_descriptions(ctx):
    def fresh(cfg=None, gates=synth.EXT_GATES):
        return synth.ext_gates_circuit(3, cfg or PRESETS["rec"](), seed=2, gates=gates)

    def gate(desc, t):
        return next(g for g in desc.gates if int(g["type"]) == t)
    d = fresh()                                   # 44 base coefficients: 136 wires > 135
    g = gate(d, 17); g["p0"] = 44; g["num_constraints"] = 88; d.num_gate_constraints = 88
    assert _create_error(ctx, d) == -1
    d = fresh()                                   # 33 ext coefficients: 136 wires > 135
    g = gate(d, 18); g["p0"] = 33; g["num_constraints"] = 66
    assert _create_error(ctx, d) == -1
    d = fresh()                                   # constraint count that does not match p0
    gate(d, 15)["num_constraints"] = 19
    assert _create_error(ctx, d) == -1
    d = fresh()
    g = gate(d, 16); g["p0"] = 0; g["num_constraints"] = 0
    assert _create_error(ctx, d) == -1
    d = fresh()                                   # ArithmeticExtensionGate needs two gate constants
    d.constants = np.ascontiguousarray(d.constants[:-1]); d.num_constants -= 1
    assert _create_error(ctx, d) == -1
    d = fresh(synth.Config(135, 40), gates=(17,))  # 6 + 40 routed inputs > 40 routed wires (124 wires fit)
    g = gate(d, 17); g["p0"] = 40; g["num_constraints"] = 80; d.num_gate_constraints = 80
    assert _create_error(ctx, d) == -1
    d = fresh(synth.Config(135, 40), gates=(18,))  # 6 + 2 * 20 > 40
    g = gate(d, 18); g["p0"] = 20; g["num_constraints"] = 40; d.num_gate_constraints = 40
    assert _create_error(ctx, d) == -1
    d = fresh()
    gate(d, 15)["type"] = 19
    assert _create_error(ctx, d) == -3
    gc = glp.Circuit(ctx, fresh())               # the unmodified description is accepted
    gc.free()


# ---------------------------------------------------------------------------------------------------- 8. full size
def test_full_size_mixed_circuit(ctx):
    desc = synth.ext_gates_circuit(20, PRESETS["rec"](), seed=4)
    gc, proof = _prove_and_check(ctx, desc)
    gc.free()
