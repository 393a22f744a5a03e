"""The witness checker (glp_witness_check), the part that needs no GPU.
1. tests/witness_check_restate.py reports clean on satisfied synthetic circuits and exactly what was planted after single-cell changes
   (constraints and copies), so the GPU tests may compare the library against it.
2. glp_witness_check is declared, exported, bound and named in INTEGRATION.md; a null context is GLP_ERR_ARG.
The device side is tests/test_gpu_witness_check.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding, synth
import witness_check_restate as wr
import zeta_identity_recursion as zr

P = wr.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = (0, 0, 0) + (None,) * 10
ARITH3 = dict(num_const_rows=2, num_noop_rows=1)      # what fits 2^3 rows: public inputs, two constant rows, four arithmetic rows, a NoopGate row


def _circuits():
    return {"arith": synth.arith_circuit(3, **ARITH3), "ext": synth.ext_gates_circuit(5),
            # 2^4 rows: the smallest trace that holds the eight gate types of the mixed unit
            "recursion": synth.recursion_gates_circuit(4, synth.Config.standard_recursion_config(), mix_ext=True)}


@pytest.fixture(scope="module")
def circuits():
    return _circuits()


@pytest.mark.parametrize("name", ["arith", "ext", "recursion"])
def test_restatement_reports_clean(circuits, name):
    desc = circuits[name]
    assert all(int(g["type"]) in wr.HAS_BODY for g in desc.gates)
    rep, by_gate = wr.check(desc)
    assert wr.as_tuple(rep) == CLEAN and by_gate == [0] * len(desc.gates)


def _gate_of_type(desc, t):
    return next(i for i, g in enumerate(desc.gates) if int(g["type"]) == t)


def test_restatement_names_a_planted_constraint(circuits):
    desc = circuits["arith"]
    gi = _gate_of_type(desc, synth.GATE_ARITHMETIC)
    ops = int(desc.gates[gi]["p0"])
    sm = wr.decode_sigmas(desc)
    rows = [int(r) for r in zr.gate_rows(desc, gi)]
    # the output of the last operation feeds nothing: one constraint, no copy
    for r, delta in ((rows[0], 1), (rows[-1], 5)):
        W = desc.wires.copy()
        col = 4 * (ops - 1) + 3
        assert sm[(col, r)] == (col, r)
        W[col, r] = (int(W[col, r]) + delta) % P
        rep, by_gate = wr.check(desc, W, sigma_map=sm)
        assert wr.as_tuple(rep) == (1, 1, 0, r, gi, ops - 1, delta) + (None,) * 6
        assert by_gate == [1 if i == gi else 0 for i in range(len(desc.gates))]
    # two rows, two constraints in the later one (an addend of op 1 is also the output of op 0): the first is the earlier row
    W = desc.wires.copy()
    W[4 * (ops - 1) + 3, rows[2]] = (int(W[4 * (ops - 1) + 3, rows[2]]) + 3) % P
    W[4 * (ops - 1) + 2, rows[1]] = (int(W[4 * (ops - 1) + 2, rows[1]]) + 1) % P
    rep, by_gate = wr.check(desc, W, sigma_map=sm)
    c1 = int(desc.constants[desc.num_selectors + 1, rows[1]])
    assert (rep["failed_constraints"], rep["failed_rows"], rep["row"], rep["gate"], rep["constraint"]) == (2, 2, rows[1], gi, ops - 1)
    assert rep["value"] == (P - c1) % P and by_gate[gi] == 2


def test_restatement_names_a_wrong_public_input():
    pi = [3, 1 << 40]
    from plonky2_lib_amd import poseidon_py
    desc = synth.arith_circuit(3, public_inputs=pi, **ARITH3, pi_hash=np.array(poseidon_py.hash_no_pad(pi), np.uint64))
    assert wr.as_tuple(wr.check(desc)[0]) == CLEAN
    rep, by_gate = wr.check(desc, public_inputs=[3, (1 << 40) + 1])
    gi = _gate_of_type(desc, synth.GATE_PUBLIC_INPUT)
    assert (rep["failed_constraints"], rep["failed_rows"], rep["failed_copies"], rep["row"], rep["gate"], rep["constraint"]) == (4, 1, 0, 0, gi, 0)
    assert by_gate == [1 if i == gi else 0 for i in range(len(desc.gates))]


def test_restatement_names_a_planted_copy(circuits):
    desc = circuits["arith"]
    gi = _gate_of_type(desc, synth.GATE_ARITHMETIC)
    rows = [int(r) for r in zr.gate_rows(desc, gi)]
    sm = wr.decode_sigmas(desc)
    r = rows[1]                                   # column 1 of the arithmetic rows is one copy cycle over all of them
    cycle = [(1, x) for x in rows]
    assert sm[(1, r)] in cycle and sm[(1, r)] != (1, r)
    before = next(c for c in cycle if sm[c] == (1, r))
    W = desc.wires.copy()
    old = int(W[1, r])
    W[1, r] = (old + 1) % P
    rep, _ = wr.check(desc, W, sigma_map=sm)
    assert rep["failed_copies"] == 2              # the cell against its image, and the cell whose image it is
    first = min((before[1], before[0]), (r, 1))
    assert (rep["copy_row"], rep["copy_col"]) == first
    if first == (r, 1):
        assert (rep["to_col"], rep["to_row"]) == sm[(1, r)] and (rep["copy_value"], rep["to_value"]) == ((old + 1) % P, old)
    else:
        assert (rep["to_col"], rep["to_row"]) == (1, r) and (rep["copy_value"], rep["to_value"]) == (old, (old + 1) % P)
    assert rep["failed_rows"] == 1 and rep["row"] == r and rep["constraint"] == 0        # m1 of operation 0


def test_restatement_refuses_a_sigma_on_no_coset(circuits):
    desc = circuits["arith"]
    keep = int(desc.sigmas[2, 5])
    desc.sigmas[2, 5] = 0
    with pytest.raises(ValueError, match=r"sigmas\[2\]\[5\]"):
        wr.decode_sigmas(desc)
    desc.sigmas[2, 5] = keep


def test_unknown_gate_types_still_get_copies():
    """every assigned gate type has a body now; the unassigned type 19 is what is left to answer UNKNOWN for"""
    desc = synth.u32_circuit(6)
    rep, by_gate = wr.check(desc)
    assert wr.as_tuple(rep) == CLEAN and by_gate == [0] * len(desc.gates)
    gi = _gate_of_type(desc, synth.GATE_U32_INTERLEAVE)
    desc.gates[gi] = dict(desc.gates[gi], type=19)
    assert 19 not in wr.HAS_BODY
    rep, by_gate = wr.check(desc)
    assert rep["failed_constraints"] == wr.UNKNOWN and rep["row"] == wr.UNKNOWN and rep["failed_copies"] == 0
    assert by_gate == [wr.UNKNOWN if i == gi else 0 for i in range(len(desc.gates))]


def test_new_function_is_declared_exported_and_bound():
    glp.build_library()
    name = "glp_witness_check"
    out = subprocess.check_output(["nm", "-D", "--defined-only", glp.library_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = glp.load_library()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert name in glp.exported_symbols(), name + " is not declared in include/glp.h"
    assert name in exported, name + " is not exported by libglprover.so"
    assert getattr(L, name).argtypes, name + " has no argtypes in binding.py"
    assert "fn " + name + "(" in integration, name + " is missing from INTEGRATION.md's extern block"
    assert hasattr(glp.Circuit, "check_witness")
    assert C.sizeof(binding._WitnessReport) == 88 and binding._WitnessReport.value.offset == 40 and binding._WitnessReport.to_row.offset == 64
    assert set(binding.GATE_TYPE_NAMES) == set(range(19)) | {20, 21, 22}


def test_null_context_is_refused():
    L = glp.load_library()
    rep = binding._WitnessReport()
    z = (C.c_uint64 * 8)()
    assert L.glp_witness_check(None, None, 1, z, 0, None, C.byref(rep), None) == -1 and b"ctx is null" in L.glp_last_error()


def test_report_text():
    r = binding._WitnessReport(failed_constraints=2, failed_rows=3, failed_copies=1, row=37, gate=4, constraint=12, value=0xAB, copy_row=12,
                               copy_col=5, to_col=0, to_row=40, copy_value=0xA, to_value=0xB)
    rep = glp.WitnessReport(r, [0, 1, 2, 3, 8])
    assert not rep.ok
    assert str(rep) == ("row 37: gate 4 (U32ArithmeticGate) constraint 12 = 0xab; 3 failing rows; first broken copy (col 5, row 12) = 0xa -> "
                        "(col 0, row 40) = 0xb; 1 broken copies")
    assert glp.WitnessReport(binding._WitnessReport()).ok
