"""glp_verify_batch (the verifier for batch self-checking, query rounds on the GPU): on batches with tampered
members its accept / reject verdicts and its rejection reasons must equal glp_verify's (host code) proof by proof, and both must agree
with the oracle verifier -- section by section of the proof (caps, openings, FRI caps, query leaves, Merkle paths, fold evaluations,
final polynomial, proof-of-work witness, public inputs).  Mirrors what every reference driver does after proving:
`data.verify(proof)` [REF src/zkdsa/circuits/mod.rs:341-347, src/ecdsa/gadgets/ecdsa.rs:349-352]."""
import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
import proof_sections

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _sections(desc):
    """word ranges of a proof by section: tests/proof_sections.py, the map written from the documented layout (include/glp.h)"""
    return proof_sections.legacy_ranges(desc)


def _tampered_batch(proof, desc, rng):
    sec = _sections(desc)
    assert max(v[1] for v in sec.values()) == len(proof)
    names, batch = ["untouched"], [proof.copy()]
    for name, (lo, hi) in sec.items():
        bad = proof.copy()
        pos = int(rng.integers(lo, hi))
        bad[pos] = np.uint64((int(bad[pos]) + 1) % glp.P)
        names.append(name)
        batch.append(bad)
    nc = proof.copy()
    nc[sec["openings"][0] + 3] = np.uint64(glp.P + 1)               # not a canonical field element
    names.append("non_canonical"); batch.append(nc)
    names.append("untouched_again"); batch.append(proof.copy())
    return names, np.stack(batch)


@pytest.mark.parametrize("which", ["zkdsa", "ecdsa", "smt", "arith_rec"])
def test_verdicts_and_reasons_equal_the_host_verifier(ctx, oracle, which):
    desc = {"zkdsa": lambda: synth.zkdsa_circuit(3), "ecdsa": lambda: synth.ecdsa_shape_circuit(7, seed=8),
            "smt": lambda: synth.smt_shape_circuit(10, seed=9),                      # two FRI reductions
            "arith_rec": lambda: synth.arith_circuit(12, synth.Config.standard_recursion_config(), seed=2)}[which]()
    gc = glp.Circuit(ctx, desc)
    oc = oracle.OracleCircuit(desc)
    proof = gc.prove()
    names, batch = _tampered_batch(proof, desc, np.random.default_rng(7))
    ok, reasons = gc.verify_batch(batch, reasons=True)
    L = glp.load_library()
    for k, name in enumerate(names):
        host_ok = gc.verify(batch[k])
        host_reason = "" if host_ok else L.glp_last_error().decode()
        assert bool(ok[k]) == host_ok, (name, reasons[k], host_reason)
        assert reasons[k] == host_reason, (name, reasons[k], host_reason)
        if name != "non_canonical":
            assert (oc.verify(batch[k]) == 0) == host_ok, name
        assert bool(ok[k]) == name.startswith("untouched"), (name, reasons[k])
    # the reasons name the stage that caught it
    by = dict(zip(names, reasons))
    assert "Merkle proof" in by["q0_path1"] and "initial tree 1" in by["q0_path1"]
    assert "proof of work" in by["pow"].lower()
    assert "canonical" in by["non_canonical"]
    gc.free()


def test_host_and_device_transcripts_of_the_verifier_agree(ctx):
    """PoseidonGoldilocksConfig runs the K transcripts on the device (the prover's kernels over the uploaded proofs); GLP_VERIFY_HOST_TRANSCRIPT=1
    keeps them on host threads (what KeccakGoldilocksConfig always does): same verdicts, same reasons, on a batch tampered section by section."""
    import os
    desc = synth.smt_shape_circuit(10, seed=9)
    gc = glp.Circuit(ctx, desc)
    names, batch = _tampered_batch(gc.prove(), desc, np.random.default_rng(23))
    dev_ok, dev_why = gc.verify_batch(batch, reasons=True)
    os.environ["GLP_VERIFY_HOST_TRANSCRIPT"] = "1"
    try:
        host_ok, host_why = gc.verify_batch(batch, reasons=True)
    finally:
        del os.environ["GLP_VERIFY_HOST_TRANSCRIPT"]
    assert list(dev_ok) == list(host_ok) and list(dev_why) == list(host_why), list(zip(names, dev_why, host_why))
    assert dev_ok[0] and dev_ok[-1] and dev_ok.sum() == 2
    gc.free()


def test_keccak_config_batch(ctx, oracle):
    """KeccakGoldilocksConfig: KeccakHash<25> paths and caps on the device side of the verifier"""
    desc = synth.zkdsa_circuit(3)
    desc.hasher, desc.circuit_digest = 1, None
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    names, batch = _tampered_batch(proof, desc, np.random.default_rng(11))
    ok, reasons = gc.verify_batch(batch, reasons=True)
    L = glp.load_library()
    for k, name in enumerate(names):
        host_ok = gc.verify(batch[k])
        assert bool(ok[k]) == host_ok and reasons[k] == ("" if host_ok else L.glp_last_error().decode()), (name, reasons[k])
    assert ok[0] and ok[-1] and ok.sum() == 2
    gc.free()


def test_a_batch_of_different_proofs(ctx, oracle):
    """256 zkdsa proofs from glp_prove_batch, two of them damaged: exactly those two are rejected"""
    rng = np.random.default_rng(500)
    K = 256
    descs = [synth.zkdsa_circuit(3, seed=5, private_key=synth.gl.rand(rng, 4), message=synth.gl.rand(rng, 4)) for _ in range(K)]
    gc = glp.Circuit(ctx, descs[0])
    proofs = gc.prove_batch(np.stack([d.wires for d in descs]), np.stack([d.public_inputs for d in descs]))
    assert gc.verify_batch(proofs).all()
    proofs[17, 40] ^= np.uint64(1)
    proofs[200, gc.proof_words - 20] ^= np.uint64(1)
    ok = gc.verify_batch(proofs)
    assert not ok[17] and not ok[200] and ok.sum() == K - 2
    with pytest.raises(glp.GlpError):
        gc.verify_batch(proofs[:, :-1])
    gc.free()


def _three_witnesses(which):
    """three descriptions of ONE circuit with three different witnesses (the first is the circuit's own)"""
    if which == "smt10":
        # two reductions.  The builder draws no input to redraw, but a BaseSumGate<2> row (wire 0 = sum of the 63 bits in wires 1..63) holds a
        # value that only its bit 0 ties to other rows: members 1 and 2 flip bit 1, bit 2 of the first such row
        descs = [synth.smt_shape_circuit(10, seed=9) for _ in range(3)]
        w = np.asarray(descs[0].wires)
        rows = [r for r in np.nonzero((w[1:64] <= 1).all(axis=0) & (w[0] > 1))[0]
                if sum(int(w[1 + j, r]) << j for j in range(63)) == int(w[0, r])]
        assert rows, "no BaseSumGate<2> row found"
        for k in (1, 2):
            wk = np.array(descs[k].wires, np.uint64)
            wk[1 + k, rows[0]] ^= np.uint64(1)
            wk[0, rows[0]] ^= np.uint64(1 << k)
            descs[k].wires = wk
        return descs
    rng = np.random.default_rng(77)
    keys = [dict(private_key=synth.gl.rand(rng, 4), message=synth.gl.rand(rng, 4)) for _ in range(3)]
    if which == "zk":           # salted leaves, two rounds: the "zk" case of tests/test_gpu_verify_sweep.py
        return [synth.zkdsa_circuit(config=synth.Config.standard_recursion_zk_config(num_query_rounds=2), blinding_seed=7, **kw) for kw in keys]
    descs = [synth.zkdsa_circuit(3, **kw) for kw in keys]       # "keccak": KeccakHash<25> caps and paths
    for d in descs:
        d.hasher, d.circuit_digest = 1, None
    return descs


@pytest.mark.parametrize("which", ["smt10", "zk", "keccak"])
def test_each_member_is_checked_against_its_own_caps(ctx, which):
    """K = 3 proofs of different witnesses, so every member carries caps of its own (the sweeps tile one proof; the 256 different proofs above
    are zkdsa under Poseidon: no reductions, unsalted leaves): all accepted, by glp_verify too.  Then members 0 and 1 trade their query
    sections: the transcript of neither moves, so the query rounds are what rejects both, for glp_verify's reason, and member 2 stays accepted."""
    descs = _three_witnesses(which)
    gc = glp.Circuit(ctx, descs[0])
    proofs = gc.prove_batch(np.stack([d.wires for d in descs]), np.stack([d.public_inputs for d in descs]))
    capw = 4 << descs[0].cap_height
    assert len({proofs[k, :capw].tobytes() for k in range(3)}) == 3, "the members share a wires cap"
    assert list(gc.verify_batch(proofs)) == [True] * 3
    assert all(gc.verify(p) for p in proofs)
    secs = proof_sections.sections(descs[0])
    assert proof_sections.tiles(secs, gc.proof_words)
    lo, hi = min(s.lo for s in secs if s.q is not None), max(s.hi for s in secs if s.q is not None)
    swapped = proofs.copy()
    swapped[0, lo:hi], swapped[1, lo:hi] = proofs[1, lo:hi], proofs[0, lo:hi]
    ok, reasons = gc.verify_batch(swapped, reasons=True)
    assert list(ok) == [False, False, True] and reasons[2] == ""
    L = glp.load_library()
    for k in (0, 1):
        assert not gc.verify(swapped[k])
        assert reasons[k] == L.glp_last_error().decode() and reasons[k].startswith("Invalid Merkle proof (query 0, initial tree"), (k, reasons[k])
    assert gc.verify(swapped[2])
    gc.free()


def test_headline_shape_proof(ctx, oracle):
    """one proof of the 2^16-row, 136-wire shape (depth-15 paths, arity-16 folds): device verdict = host verdict = oracle verdict"""
    desc = synth.arith_circuit(16, synth.Config.standard_ecc_config(), seed=16)
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    bad = proof.copy(); bad[len(bad) // 2] ^= np.uint64(1)
    ok, reasons = gc.verify_batch(np.stack([proof, bad, proof]), reasons=True)
    assert list(ok) == [True, False, True] and gc.verify(proof) and not gc.verify(bad)
    assert reasons[1] == glp.load_library().glp_last_error().decode()
    gc.free()
