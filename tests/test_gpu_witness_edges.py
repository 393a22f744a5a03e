"""glp_witness_fill, glp_witness_check and the prover on the edge rows of tests/witness_edge_rows.py: hand-chosen inputs at the corners
where the row-local generators branch (inverse wire 0, field result p - 2^32, carry 15, first / last index, 0^0, a point on the
coset, ...) and inputs outside the gates' domains.  Three statements of the gates meet here: the generators of csrc/witness.hip, the
constraints of gate_terms / witness_check.inc, and the CPU restatements tests/witness_fill_restate.py and tests/witness_check_restate.py
(pinned to the oracle by tests/test_limb_gates_restate.py, test_witness_fill_restate.py and test_witness_edge_rows.py).  Everything is
exact equality mod p."""
import numpy as np
import pytest

import plonky2_lib_amd as glp
import witness_check_restate as wr
import witness_edge_rows as we
import witness_fill_restate as wf
import zeta_identity_recursion as zr

pytestmark = pytest.mark.gpu

P = we.P
CIRCUITS = {ec.name: ec for ec in we.circuits()}
CIRCUITS["U32Subtraction-workgroups"] = we.subtraction_across_workgroups()       # rows 0, 255, 256, 511 of 2^9: two workgroups of the fill


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _gpu_fill(ctx, gc, w, only_advice):
    w = np.ascontiguousarray(w)
    d = ctx.dev_alloc(w.nbytes)
    ctx.dev_upload(d, w)
    gc.witness_fill(d, only_advice=only_advice)
    out = np.empty_like(w)
    ctx.dev_download(d, out)
    return out, d


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_fill_equals_the_restatement(ctx, name):
    ec = CIRCUITS[name]
    desc = ec.desc
    gc = glp.Circuit(ctx, desc)
    for gi, g in enumerate(desc.gates):
        assert [int(x) for x in gc.witness_columns(gi)] == wf.roles(g, desc.num_wires), gi
    written = we.role_mask(desc)
    w = we.scramble_outputs(ec, 41)
    assert (w != desc.wires)[written].all() and (w == desc.wires)[~written].all()
    nr = desc.num_routed_wires
    for only_advice in (False, True):
        got, d = _gpu_fill(ctx, gc, w, only_advice)
        ctx.dev_free(d)
        bad = we.first_mismatch(got, wf.fill(desc, w, only_advice))
        assert bad is None, "only_advice %d: (column %d, row %d) = 0x%x, restated 0x%x" % ((only_advice,) + bad)
        assert (got == w)[~written].all()                       # nothing outside role 1 was written
        if only_advice:
            assert (got[:nr] == w[:nr]).all()
    gc.free()


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_check_equals_the_restatement(ctx, name):
    ec = CIRCUITS[name]
    desc = ec.desc
    gc = glp.Circuit(ctx, desc)
    got, d = _gpu_fill(ctx, gc, we.scramble_outputs(ec, 43), False)
    rep_gpu = gc.check_witness(dev_wires_ptr=d, by_gate=True)
    ctx.dev_free(d)
    rep, by_gate = wr.check(desc, got)
    assert rep_gpu.as_tuple() == wr.as_tuple(rep), (rep_gpu.as_tuple(), wr.as_tuple(rep))
    assert rep_gpu.rows_failed_by_gate == by_gate
    if ec.in_domain:
        assert rep_gpu.ok and rep_gpu.as_tuple()[:3] == (0, 0, 0)
    else:                                                       # every table row fails; the first one is named with its value
        assert rep_gpu.failed_rows == len(ec.rows) and rep_gpu.row == ec.row_of[0] and 0 < rep_gpu.value < P
        assert int(desc.gates[rep_gpu.gate]["type"]) == ec.type and rep_gpu.failed_copies == 0
    gc.free()


@pytest.mark.parametrize("name", sorted(n for n, ec in CIRCUITS.items() if ec.in_domain))
def test_prove_from_the_filled_witness(ctx, oracle, name):
    ec = CIRCUITS[name]
    desc = ec.desc
    early = ec.type <= 14                                       # the oracle has generators and constraint bodies up to type 14
    oc = oracle.OracleCircuit(desc) if early else None          # derives the circuit digest
    gc = glp.Circuit(ctx, desc)
    got, d = _gpu_fill(ctx, gc, we.scramble_outputs(ec, 47), False)
    proof = gc.prove_device(d)
    ctx.dev_free(d)
    assert gc.verify(proof)
    digest = gc.digest()
    assert zr.check(desc, proof, digest, 0)
    if early:
        assert (digest == np.asarray(desc.circuit_digest, np.uint64)).all()
        assert oc.verify(proof) == 0
        rc, ref = oc.prove(wires=got)
        assert rc == 0 and (proof == ref).all(), "first mismatch at word %d" % int(np.argmax(proof != ref))
    gc.free()
