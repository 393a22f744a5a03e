"""The caller-defined running arguments of include/glp.h at the C boundary, without a GPU: the two symbols are declared, exported,
bound and named in INTEGRATION.md; the header's GLP_RUN_* constants are the binding's; and both entry points answer a null context
with GLP_ERR_ARG before they touch a device."""
import os
import re
import subprocess

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("glp_gate_program_rows", "glp_running_columns")
GLP_ERR_ARG = -1


def test_new_symbols_are_declared_exported_bound_and_documented():
    glp.build_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", glp.library_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = glp.exported_symbols()
    L = glp.load_library()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert s in declared, s + " is not declared in include/glp.h"
        assert s in exported, s + " is not exported by libglprover.so"
        assert getattr(L, s).argtypes, s + " has no argtypes in binding.py"
        assert "fn " + s + "(" in integration, s + " is missing from INTEGRATION.md's extern block"
    assert hasattr(glp.GateProgram, "rows") and hasattr(glp.Context, "running_columns")


def test_header_constants_are_the_bindings():
    hdr = open(os.path.join(ROOT, "include", "glp.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (GLP_RUN_\w+) (\d+)u", hdr)}
    assert consts == {"GLP_RUN_SUM": glp.RUN_SUM, "GLP_RUN_PRODUCT": glp.RUN_PRODUCT} == {"GLP_RUN_SUM": 0, "GLP_RUN_PRODUCT": 1}
    assert (binding.RUN_SUM, binding.RUN_PRODUCT) == (glp.RUN_SUM, glp.RUN_PRODUCT)
    # the restatement's names for them
    import running_restate as rr
    assert (rr.SUM, rr.PRODUCT) == (glp.RUN_SUM, glp.RUN_PRODUCT)


def test_a_null_context_is_an_argument_error():
    L = glp.load_library()
    assert L.glp_gate_program_rows(None, None, 1, 4, None, None, 0, None, None, 0) == GLP_ERR_ARG
    assert b"glp_gate_program_rows" in L.glp_last_error() and b"null" in L.glp_last_error()
    assert L.glp_running_columns(None, 0, 1, 1, 1, 4, None, None, 16, 0, None, 0, None) == GLP_ERR_ARG
    assert b"glp_running_columns" in L.glp_last_error() and b"null" in L.glp_last_error()
