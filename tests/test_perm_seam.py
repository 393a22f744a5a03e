"""The permutation argument at the commitment seam (glp_perm_num_polys, glp_perm_zs_commit, glp_perm_quotient_values), the part that
needs no GPU.
1. tests/perm_restate.py splits coset_quotient.quotient_values into the permutation terms and the caller's gate sums: for a circuit
   with gates, over LDE rows from the oracle, perm_quotient(.., gate_sums(..)) is quotient_values word for word.
2. the synthetic circuits of the GPU tests close (Z(g^n) = 1) and their quotient is quotient_values' of a circuit without gates.
3. the entry points are declared, exported, bound and named in INTEGRATION.md; glp_perm_num_polys and the refusals that need no device.
The device side is tests/test_gpu_perm_seam.py."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
import coset_quotient as cq
import perm_restate as pr
import zeta_identity as zi

NEW = ["glp_perm_num_polys", "glp_perm_zs_commit", "glp_perm_quotient_values"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lde_rows(oracle, values, rate_bits, sub_bits):
    """row-major [M][ncols] values on g <W_M> of the polynomials with these values on H"""
    step = 1 << (rate_bits - sub_bits)
    return np.stack([oracle.lde(oracle.ifft(v), rate_bits)[::step] for v in np.asarray(values, np.uint64)], axis=1)


def test_permutation_terms_plus_gate_sums_is_the_whole_quotient(oracle):
    desc = cq.seam_circuit(oracle)
    rb = int(desc.rate_bits)
    sub_bits = int(desc.quotient_degree_factor).bit_length() - 1
    nc = int(desc.num_constants)
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0
    betas, gammas, alphas, _zeta, pih = zi.challenges(desc, proof, desc.circuit_digest)
    zp = cq.zs_partial_products(desc, desc.wires, betas, gammas)
    cs = np.concatenate([np.asarray(desc.constants, np.uint64), np.asarray(desc.sigmas, np.uint64)])
    rows = [lde_rows(oracle, v, rb, sub_bits) for v in (cs, desc.wires, zp)]
    want = cq.quotient_values(desc, rows[0], rows[1], rows[2], sub_bits, betas, gammas, alphas, pih)
    gs = pr.gate_sums(desc, rows[0], rows[1], alphas, pih)
    assert gs.any(), "the circuit's gates contribute nothing: the split is not exercised"
    got = pr.perm_quotient(desc, rows[0][:, nc:], rows[1], rows[2], sub_bits, betas, gammas, alphas, gs)
    assert got.shape == want.shape and (got == want).all(), "first mismatch at %s" % (np.argwhere(got != want)[:1],)
    # the map is linear in the gate sums: without them, the caller adds alpha^T gate_sums / Z_H itself
    bare = pr.perm_quotient(desc, rows[0][:, nc:], rows[1], rows[2], sub_bits, betas, gammas, alphas, None)
    assert (bare != want).any()


@pytest.mark.parametrize("shape", [(3, 135, 80, 8, 2, 3), (4, 20, 13, 5, 3, 3)])
def test_synthetic_circuits_close_and_match_the_gateless_quotient(oracle, shape):
    lg, nw, nr, chunk, nch, sub_bits = shape
    desc = pr.synthetic(lg, nw, nr, chunk, nch, seed=lg * 1000 + nr)
    rng = np.random.default_rng(5)
    betas, gammas, alphas = (oracle.rand_field(rng, (nch,)) for _ in range(3))
    zp = cq.zs_partial_products(desc, desc.wires, betas, gammas)          # asserts Z(g^n) == 1
    assert zp.shape == (glp_perm_polys(nr, chunk, nch), 1 << lg)
    rows = [lde_rows(oracle, v, 3, sub_bits) for v in (desc.sigmas, desc.wires, zp)]
    want = cq.quotient_values(desc, rows[0], rows[1], rows[2], sub_bits, betas, gammas, alphas, [0, 0, 0, 0])
    got = pr.perm_quotient(desc, rows[0], rows[1], rows[2], sub_bits, betas, gammas, alphas)
    assert (got == want).all()
    # another witness of the same circuit: same sigmas, other wires, and it closes as well
    other = pr.synthetic(lg, nw, nr, chunk, nch, seed=lg * 1000 + nr, wires_seed=77)
    assert (other.sigmas == desc.sigmas).all() and (other.wires != desc.wires).any()
    cq.zs_partial_products(other, other.wires, betas, gammas)


def glp_perm_polys(nr, chunk, nch):
    return nch * (-(-nr // chunk))


def test_new_functions_are_declared_exported_and_bound():
    glp.build_library()
    declared = glp.exported_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", glp.library_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = glp.load_library()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in declared, name + " is not declared in include/glp.h"
        assert name in exported, name + " is not exported by libglprover.so"
        assert getattr(L, name).argtypes, name + " has no argtypes in binding.py"
        assert "fn " + name + "(" in integration, name + " is missing from INTEGRATION.md's extern block"
    for name in ("perm_zs_commit", "perm_quotient_values"):
        assert hasattr(glp.Context, name)
    assert callable(glp.perm_num_polys) and callable(glp.perm_desc)


def _bag(nr, chunk, nch, nw=None, lg=3, k_is=None):
    return SimpleNamespace(degree_bits=lg, num_wires=nr if nw is None else nw, num_routed_wires=nr, num_challenges=nch,
                           quotient_degree_factor=chunk, k_is=pr.plonky2_k_is(nr) if k_is is None else k_is)


def test_perm_num_polys():
    glp.build_library()
    assert glp.perm_num_polys(_bag(80, 8, 2, 135)) == 20
    assert glp.perm_num_polys(_bag(13, 5, 3, 20)) == 9
    assert glp.perm_num_polys(_bag(80, 80, 1)) == 1                      # one chunk: Z alone
    assert glp.perm_num_polys(_bag(80, 1, 4)) == 320
    L = glp.load_library()
    assert L.glp_perm_num_polys(None) == 0 and b"desc" in L.glp_last_error()
    for bad, needle in ((_bag(80, 0, 2), "chunk_size"), (_bag(80, 8, 0), "num_challenges"), (_bag(80, 8, 5), "num_challenges"),
                        (_bag(8, 8, 2, nw=7), "num_routed_wires"), (_bag(13, 5, 3, lg=25), "log_n")):
        assert glp.perm_num_polys(bad) == 0 and needle in L.glp_last_error().decode(), needle
    k = pr.plonky2_k_is(4)
    k[2] = cq.P
    assert glp.perm_num_polys(_bag(4, 2, 2, k_is=k)) == 0 and "k_is[2]" in L.glp_last_error().decode()
    d, _keep = glp.perm_desc(_bag(4, 2, 2))
    d.num_routed_wires = 0
    assert L.glp_perm_num_polys(C.byref(d)) == 0 and b"num_routed_wires" in L.glp_last_error()
    d, _keep = glp.perm_desc(_bag(4, 2, 2))
    d.k_is = None
    assert L.glp_perm_num_polys(C.byref(d)) == 0 and b"k_is" in L.glp_last_error()


def test_refusals_that_need_no_device():
    L = glp.load_library()
    h = C.c_void_p()
    z = (C.c_uint64 * 8)(1, 2, 3, 4, 5, 6, 7, 8)
    d, _keep = glp.perm_desc(_bag(2, 2, 2, lg=1))
    calls = [
        lambda: L.glp_perm_zs_commit(None, C.byref(d), 1, z, 0, z, 0, z, z, 1, 0, 0, None, C.byref(h)),
        lambda: L.glp_perm_zs_commit(None, None, 1, z, 0, z, 0, z, z, 1, 0, 0, None, C.byref(h)),
        lambda: L.glp_perm_quotient_values(None, C.byref(d), 1, None, 0, None, None, 0, z, z, z, None, 0, z, 0),
    ]
    for call in calls:
        assert call() == -1 and b"null" in L.glp_last_error()
        assert not h.value
    assert binding._PermDesc.k_is.offset == 24 and C.sizeof(binding._PermDesc) == 32      # the C struct: five u32, padding, a pointer
