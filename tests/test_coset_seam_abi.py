"""The caller's-quotient block of include/glp.h at the C boundary, without a GPU: the three symbols are exported, and
glp_batch_lde_values answers a null batch with GLP_ERR_ARG before it touches a device, as the other accessors do."""
import subprocess

import plonky2_lib_amd as glp

SEAM = ("glp_batch_lde_values", "glp_coset_ifft", "glp_batch_from_coset_values")
GLP_ERR_ARG = -1


def test_seam_symbols_are_declared_and_exported():
    glp.build_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", glp.library_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = glp.exported_symbols()
    for s in SEAM:
        assert s in declared and s in exported, s


def test_lde_values_of_a_null_batch_is_an_argument_error():
    L = glp.load_library()
    rc = L.glp_batch_lde_values(None, 0, 1, 0, 0, 1, glp.LDE_ROW_MAJOR, None, 0)
    assert rc == GLP_ERR_ARG
    assert b"glp_batch_lde_values" in L.glp_last_error() and b"null" in L.glp_last_error()
