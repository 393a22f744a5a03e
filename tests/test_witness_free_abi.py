"""The C side of the free units (include/glp.h: glp_witness_free_unit, struct glp_witness_plan_free_info, GLP_WGEN_*) against the
binding's mirrors, from a C99 program that prints the header's own sizes and offsets.  Every refusal of glp_witness_plan_create_ex comes
after the context check, and a context needs a GPU: the refusals are in tests/test_gpu_witness_free.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from plonky2_lib_amd import binding, gadgets

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "glp.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(glp_witness_free_unit), offsetof(glp_witness_free_unit, kind), offsetof(glp_witness_free_unit, modulus),
           offsetof(glp_witness_free_unit, cell_begin), offsetof(glp_witness_free_unit, len));
    printf("%zu %zu %zu %zu %zu\n", sizeof(struct glp_witness_plan_free_info), offsetof(struct glp_witness_plan_free_info, num_free_units),
           offsetof(struct glp_witness_plan_free_info, num_stuck_free_units), offsetof(struct glp_witness_plan_free_info, first_stuck_free_unit),
           offsetof(struct glp_witness_plan_free_info, widest_wave_free_units));
    printf("%u %u %u %u %u %u %u %u %u %llu\n", GLP_WGEN_EQUALITY, GLP_WGEN_NONNATIVE_ADD, GLP_WGEN_NONNATIVE_MULTI_ADD, GLP_WGEN_NONNATIVE_SUB,
           GLP_WGEN_NONNATIVE_MUL, GLP_WGEN_NONNATIVE_INV, GLP_WGEN_BIGUINT_DIV_REM, GLP_WGEN_GLV_SECP256K1, GLP_WGEN_MAX_LIMBS,
           (unsigned long long)GLP_WGEN_NO_CELL);
    printf("%zu\n", sizeof(struct glp_witness_plan_info));
    return 0;
}
"""


def test_struct_layouts_and_constants(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(HERE, "include"), str(src), "-o", str(exe)])
    unit, info, consts, plan_info = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    U, I = binding._WitnessFreeUnit, binding._WitnessPlanFreeInfo
    assert unit == [C.sizeof(U), U.kind.offset, U.modulus.offset, U.cell_begin.offset, U.len.offset] == [24, 0, 4, 8, 12]
    dt = binding.FREE_UNIT_DTYPE
    assert [dt.itemsize] + [dt.fields[f][1] for f in ("kind", "modulus", "cell_begin", "len")] == unit
    assert info == [C.sizeof(I)] + [getattr(I, f).offset for f, _ in I._fields_]
    kinds = [binding.WGEN_EQUALITY, binding.WGEN_NONNATIVE_ADD, binding.WGEN_NONNATIVE_MULTI_ADD, binding.WGEN_NONNATIVE_SUB, binding.WGEN_NONNATIVE_MUL,
             binding.WGEN_NONNATIVE_INV, binding.WGEN_BIGUINT_DIV_REM, binding.WGEN_GLV_SECP256K1]
    assert consts == kinds + [binding.WGEN_MAX_LIMBS, binding.WGEN_NO_CELL] == list(range(1, 9)) + [18, 2 ** 64 - 1]
    assert kinds == [gadgets.WGEN_EQUALITY, gadgets.WGEN_NONNATIVE_ADD, gadgets.WGEN_NONNATIVE_MULTI_ADD, gadgets.WGEN_NONNATIVE_SUB, gadgets.WGEN_NONNATIVE_MUL,
                     gadgets.WGEN_NONNATIVE_INV, gadgets.WGEN_BIGUINT_DIV_REM, gadgets.WGEN_GLV_SECP256K1] and gadgets.WGEN_NO_CELL == binding.WGEN_NO_CELL
    assert plan_info == [C.sizeof(binding._WitnessPlanInfo)]                # the existing struct is as it was


def test_new_entry_points_are_declared_and_exported():
    import plonky2_lib_amd as glp
    glp.build_library()
    declared = glp.exported_symbols()
    assert "glp_witness_plan_create_ex" in declared and "glp_witness_plan_free_info" in declared and "glp_witness_plan_create" in declared
    L = glp.load_library()
    assert L.glp_witness_plan_create_ex.argtypes[-1] == C.POINTER(C.c_void_p) and len(L.glp_witness_plan_create_ex.argtypes) == 11


def test_binding_refuses_malformed_free_units_before_the_call():
    """Circuit.witness_plan's own checks need no handle: a unit row that does not fit its C fields, moduli that are no rows of 8."""
    import pytest
    plan = binding.Circuit.witness_plan
    fake = type("FakeCircuit", (), {"ctx": None, "_h": None})()
    with pytest.raises(binding.GlpError, match="does not fit its C type"):
        plan(fake, [], free_units=(np.array([[5, 0, 0, 8, 8, 8, 1 << 16, 0, 0]]), []), moduli=np.zeros((1, 8)))
    with pytest.raises(binding.GlpError, match="moduli has 7 words"):
        plan(fake, [], free_units=(np.array([[5, 0, 0, 8, 8, 8, 8, 0, 0]]), np.zeros(32)), moduli=np.zeros(7))
    with pytest.raises(binding.GlpError, match="moduli without free_units"):
        plan(fake, [], moduli=np.zeros((1, 8)))
