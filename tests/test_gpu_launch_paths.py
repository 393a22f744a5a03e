"""Oracle parity on every launch path of the prover (launch_matrix.py names the paths and the circuits that reach them):
for each case the HIP proof equals the oracle's word for word, section by section, and both verifiers accept it; on
boundary-valued wires the (unsatisfying) proofs are still word-equal and both verifiers reject them; glp_verify_batch gives
glp_verify's verdicts and reasons; with two challenges glp_prove_batch (device and host transcripts) returns the single
proof.  Then each FRI leaf-hash form, forced through the context thresholds, on a few of the circuits."""
import os

import numpy as np
import pytest

import launch_matrix as lm
import plonky2_lib_amd as glp

pytestmark = pytest.mark.gpu

SPECIAL = np.array([0, 1, 2, 3, glp.P - 1, glp.P - 2, glp.P - 3, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 0xFFFFFFFF00000000,
                    0xFFFFFFFE00000001, 0xFFFFFFFEFFFFFFFF, 1 << 63, (1 << 63) - 1, 0xFFFFFFFF], dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


_ref, _sections, _assert_equal, _prove_batch = lm.oracle_ref, lm.head_sections, lm.assert_sections_equal, lm.prove_batch


def _boundary_wires(desc):
    """test_gpu_prove.py::test_prove_parity_on_boundary_valued_wires: 70 % of the cells boundary values of the field and its limbs"""
    rng = np.random.default_rng(99)
    w = SPECIAL[rng.integers(0, len(SPECIAL), size=desc.wires.shape)]
    keep = rng.random(desc.wires.shape) < 0.3
    w[keep] = desc.wires[keep]
    return w


@pytest.mark.parametrize("case", lm.CASES, ids=[c.id for c in lm.CASES])
def test_launch_path_parity(ctx, oracle, case):
    desc, oc, ref = _ref(oracle, case.id)
    assert case.paths <= lm.launch_plan(desc)
    gc = glp.Circuit(ctx, desc)
    assert gc.proof_words == oc.proof_words
    assert (gc.constants_sigmas_cap() == oc.cs_cap).all()
    got = gc.prove()
    _assert_equal(got, ref, desc, "prove")
    assert oc.verify(got) == 0 and gc.verify(got)

    # boundary-valued wires: the same transcript on both sides, and both verifiers reject the proof
    w = _boundary_wires(desc)
    rc, bref = oc.prove(wires=w)
    bgot = gc.prove(wires=w)
    _assert_equal(bgot, bref, desc, "boundary wires")
    assert not gc.verify(bgot) and oc.verify(bgot) != 0

    # the batch verifier against the host verifier, verdict and reason
    bad = got.copy()
    pos = _sections(desc)["openings"].start + 1
    bad[pos] = np.uint64((int(bad[pos]) + 1) % glp.P)
    ok, why = gc.verify_batch(np.stack([got, bad]), reasons=True)
    L = glp.load_library()
    for k, proof in enumerate((got, bad)):
        host_ok = gc.verify(proof)
        host_why = "" if host_ok else L.glp_last_error().decode()
        assert bool(ok[k]) == host_ok and why[k] == host_why, (k, why[k], host_why)
    assert list(ok) == [True, False]

    # many proofs per launch (two challenges only): device and host transcripts
    if desc.num_challenges == 2:
        K = case.batch_k
        assert lm.BATCH_PATHS.get(case.id, set()) <= lm.launch_plan(desc, K=K)
        for host in (False, True):
            proofs = _prove_batch(gc, desc, K, host)
            for k in range(K):
                _assert_equal(proofs[k], ref, desc, "prove_batch K=%d proof %d%s" % (K, k, " (host transcript)" if host else ""))
    gc.free()


@pytest.mark.parametrize("form", sorted(lm.MERKLE_FORMS))
def test_forced_merkle_forms(oracle, form):
    """Each FRI leaf-hash form (merkle.hip: one sponge per lane / per quad of lanes / per 12 of 16 lanes) forced by the
    thresholds a context reads at creation, through prove and prove_batch, against the oracle."""
    keys = ("GLP_MERKLE_COOP_MAX", "GLP_MERKLE_QUAD_MAX")
    cm, qm = lm.MERKLE_FORMS[form]
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(dict(zip(keys, (str(cm), str(qm)))))
    try:
        c2 = glp.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        for cid in lm.FORM_CASES:
            desc, oc, ref = _ref(oracle, cid)
            assert "fri_leaf_" + form in lm.launch_plan(desc, coop_max=cm, quad_max=qm)
            gc = glp.Circuit(c2, desc)
            got = gc.prove()
            _assert_equal(got, ref, desc, "%s / %s prove" % (cid, form))
            proofs = _prove_batch(gc, desc, 2)
            for k in range(2):
                _assert_equal(proofs[k], ref, desc, "%s / %s prove_batch proof %d" % (cid, form, k))
            gc.free()
    finally:
        c2.close()
