"""The many-proof form of the commitment seam (glp_batch_many_from_*, glp_batch_member, glp_fri_begin_many, ...), the part that needs no
GPU: every new entry point is declared in include/glp.h, exported by the built library, bound with argument types in binding.py and
declared in INTEGRATION.md's extern block; the refusals the library can give without a context.  The device side is
tests/test_gpu_fri_many.py."""
import ctypes as C
import os
import subprocess

import plonky2_lib_amd as glp

NEW = ["glp_batch_many_from_values", "glp_batch_many_from_coeffs", "glp_batch_num_proofs", "glp_batch_member", "glp_batch_caps",
       "glp_fri_begin_many", "glp_fri_num_proofs", "glp_fri_queries_many", "glp_pow_search_many", "glp_fri_prove_many"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for name in ("batch_many_from_values", "batch_many_from_coeffs", "pow_search_many"):
        assert hasattr(glp.Context, name)
    for name in ("member", "num_proofs", "caps"):
        assert hasattr(glp.Batch, name)
    assert callable(glp.fri_prove_many) and hasattr(glp.FriOpeningsMany, "queries")


def test_refusals_that_need_no_device():
    L = glp.load_library()
    h = C.c_void_p()
    z = (C.c_uint64 * 2)(1, 2)
    assert L.glp_batch_num_proofs(None) == 0 and L.glp_fri_num_proofs(None) == 0
    calls = [
        lambda: L.glp_batch_many_from_values(None, z, 0, 2, 1, 0, 1, 0, 0, None, C.byref(h)),
        lambda: L.glp_batch_many_from_coeffs(None, z, 0, 2, 1, 0, 1, 0, 0, None, C.byref(h)),
        lambda: L.glp_batch_member(None, 0, C.byref(h)),
        lambda: L.glp_batch_caps(None, z),
        lambda: L.glp_fri_begin_many(None, None, 2, z, C.byref(h)),
        lambda: L.glp_fri_queries_many(None, z, z),
        lambda: L.glp_pow_search_many(None, 0, 1, z, None, 0, 0, z),
        lambda: L.glp_fri_prove_many(None, None, 2, z, z, None, 0, z, z),
    ]
    for call in calls:
        assert call() == -1 and b"null" in L.glp_last_error()
        assert not h.value
