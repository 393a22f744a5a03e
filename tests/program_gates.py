"""Twin circuits for GLP_GATE_PROGRAM (include/glp.h, "GATE PROGRAMS IN A CIRCUIT"): a description D whose chosen gates keep their
constants, sigmas, selectors and constraint counts but bring their constraints as gate programs, traced from the restated bodies
(zeta_identity.gate_constraints, zeta_identity_recursion, limb_gates_restate) through gate_program.TraceField and closed with END
IMM(1).  Every constraint value of D' is the field element it is in D, so digest, caps and every proof word must be equal."""
import copy

import numpy as np

from plonky2_lib_amd import gate_program as gp
import zeta_identity_recursion as zr

P = gp.P
GATE_PROGRAM = 23
EXTREMES = (0, 1, P - 1, (1 << 32) - 1)


def assembler(desc):
    """-> (asm, F, constants (selectors first), wires, public-input hash) of a program that is a gate of `desc`"""
    asm = gp.Assembler([int(desc.num_constants), int(desc.num_wires)], num_params=4)
    return (asm, gp.TraceField(asm), [asm.col(0, j) for j in range(int(desc.num_constants))],
            [asm.col(1, j) for j in range(int(desc.num_wires))], [asm.param(j) for j in range(4)])


def close(asm, F, values):
    for v in values:
        asm.emit(F.lift(v))
    asm.end(asm.imm(1))
    return asm.assemble(hoist_emits=True, sink_single_use=True)        # PoseidonGate's MDS layers fit the 24 registers only so


def trace_gate(desc, g):
    """the unfiltered constraints of built-in gate g of desc as a program (what gate_program_restate.trace_circuit emits for one
    gate, minus its filter)"""
    asm, F, cs, lw, pih = assembler(desc)
    return close(asm, F, zr.gate_constraints(F, g, cs[int(desc.num_selectors):], lw, pih))


def twin(desc, which=None):
    """-> (D', programs): the gates with index in `which` (default: every gate that has constraints) become type 23"""
    d2 = copy.copy(desc)
    d2.gates = [dict(g) for g in desc.gates]
    programs = []
    for i, g in enumerate(d2.gates):
        if int(g["num_constraints"]) == 0 or (which is not None and i not in which):
            continue
        prog = trace_gate(desc, desc.gates[i])
        assert prog.max_constraints == int(g["num_constraints"])
        g.update(type=GATE_PROGRAM, p0=len(programs), p1=0)
        programs.append(prog)
    assert programs
    return d2, programs


def mixed_group(desc):
    """the index of one gate with constraints whose selector group holds another gate with constraints, in a circuit of several
    selectors (so the filter has the UNUSED factor and a program gate shares a group with a built-in one)"""
    assert int(desc.num_selectors) > 1
    for i, g in enumerate(desc.gates):
        others = [h for j, h in enumerate(desc.gates) if j != i and int(h["selector_index"]) == int(g["selector_index"]) and int(h["num_constraints"])]
        if int(g["num_constraints"]) and others:
            return i
    raise AssertionError("no selector group with two constrained gates")


def extreme_columns(rows, cols, phase=0):
    """[cols][rows] of EXTREMES such that every pair of neighbouring columns meets every pair of values"""
    r = np.arange(rows, dtype=np.int64)
    return np.array([[EXTREMES[(i // 4 ** ((c + phase) % 2)) % 4] for i in r] for c in range(cols)], np.uint64)
