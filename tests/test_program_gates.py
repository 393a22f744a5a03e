"""glp_gate_program_circuit_check (include/glp.h, "GATE PROGRAMS IN A CIRCUIT") without a GPU: the in-circuit rules, each refusal
naming the instruction and the field, and the degree / column walk on the programs traced from the restated gate bodies -- every
built-in gate type's program must report the wires, constants, constraints and (where gate_shapes.h sets one) degree of gate_shape,
restated here from the gates' definitions.

The verifier's host interpreter needs a circuit handle, which only a device makes: it is pinned on the GPU, in
tests/test_gpu_program_gates.py, against both verifiers and the twins' proofs."""
import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
from plonky2_lib_amd import gate_program as gp
import program_gates as pg


def _refused(fn, *needles):
    with pytest.raises(glp.GlpError) as e:
        fn()
    assert e.value.code == -1, str(e.value)                # GLP_ERR_ARG
    for needle in needles:
        assert needle in str(e.value), str(e.value)


def _asm(nc=3, nw=8, num_params=4):
    asm = gp.Assembler([nc, nw], num_params=num_params)
    return asm, gp.TraceField(asm)


def _body(asm, F):
    """d - (a b + c)^2 k: reads wires 0..3 and constant 2, degree 5, one constraint"""
    t = F.add(F.mul(asm.col(1, 0), asm.col(1, 1)), asm.col(1, 2))
    return F.sub(asm.col(1, 3), F.mul(F.mul(t, t), asm.col(0, 2)))


def test_symbols_are_declared_and_bound():
    declared = glp.exported_symbols()
    L = glp.load_library()
    for name in ("glp_gate_program_circuit_check", "glp_circuit_create_prog"):
        assert name in declared, name + " is not declared in include/glp.h"
        assert getattr(L, name).argtypes is not None, name
    assert glp.GATE_PROGRAM == pg.GATE_PROGRAM == 23 and glp.GATE_PROGRAM_MAX_CONSTRAINTS >= 512
    assert 23 not in glp.GATE_TYPE_NAMES and 19 not in glp.GATE_TYPE_NAMES


def test_counts_and_degree_of_a_small_program():
    asm, F = _asm()
    asm.emit(_body(asm, F))
    asm.emit(F.sub(asm.col(1, 7), asm.param(3)))           # degree 1, the top wire
    asm.emit(asm.imm(5))                                   # degree 0
    asm.end(asm.imm(1))
    assert glp.gate_program_circuit_check(asm.assemble()) == (3, 5, 8, 3)
    asm, F = _asm()
    x = asm.col(0, 0)
    for _ in range(5):                                     # MUL adds, MOV and ADD keep: x^32, then + x
        x = F.mul(x, x)
    y = asm.mov(asm.reg(), x)
    asm.emit(F.add(y, asm.col(0, 0)))
    asm.end(asm.imm(1))
    assert glp.gate_program_circuit_check(asm.assemble()) == (1, 32, 0, 1)


def test_refusals_name_the_instruction_and_the_field():
    check = glp.gate_program_circuit_check

    def prog(build, **kw):
        asm, F = _asm(**kw)
        build(asm, F)
        return asm.assemble()
    ok = prog(lambda a, F: (a.emit(_body(a, F)), a.end(a.imm(1))))
    assert check(ok) == (1, 5, 4, 3)
    _refused(lambda: check(prog(lambda a, F: (a.emit(F.add(a.col_next(1, 0), a.col(1, 1))), a.end(a.imm(1))))), "instruction 0", "field a", "COL_NEXT")
    _refused(lambda: check(prog(lambda a, F: (a.emit(F.mul(a.col(1, 0), a.x)), a.end(a.imm(1))))), "instruction 0", "field b", "X")
    _refused(lambda: check(prog(lambda a, F: (a.emit(a.col(1, 0)), a.end(a.imm(1)), a.emit(a.col(1, 1)), a.end(a.imm(1))))), "instruction 1", "END")
    _refused(lambda: check(prog(lambda a, F: (a.emit(a.col(1, 0)), a.end(a.imm(2))))), "instruction 1", "field a", "END")
    _refused(lambda: check(prog(lambda a, F: (a.emit(a.col(1, 0)), a.end(a.col(0, 0))))), "instruction 1", "field a", "END")
    _refused(lambda: check(prog(lambda a, F: (a.emit(a.col(1, 0)), a.end(a.imm(1))), num_params=5)), "num_params")
    one = gp.Assembler([4], 0)
    one.emit(one.col(0, 0)); one.end(one.imm(1))
    _refused(lambda: check(one.assemble()), "num_oracles")
    _refused(lambda: check(ok, num_regs=0), "num_regs")                     # what glp_gate_program_check refuses is refused here too
    # the constraint bound, both sides
    bound = glp.GATE_PROGRAM_MAX_CONSTRAINTS

    def many(count):
        def build(a, F):
            for _ in range(count):
                a.emit(a.col(1, 0))
            a.end(a.imm(1))
        return build
    assert check(prog(many(bound))) == (bound, 1, 1, 0)
    over = prog(many(bound))
    over.code = np.concatenate([over.code[:1], over.code])                  # one more EMIT than the assembler lets through
    _refused(lambda: check(over), "instruction %d" % bound, "EMIT")
    outs = check(ok)
    with pytest.raises(glp.GlpError):
        check(ok, num_oracles=3)
    assert outs == (1, 5, 4, 3)


# gate_shapes.h restated: (wires, gate constants, constraints, degree or None) of a gate type with its parameters
def _shape(t, p0, p1):
    s = synth
    if t == s.GATE_CONSTANT: return p0, p0, p0, None
    if t == s.GATE_PUBLIC_INPUT: return 4, 0, 4, None
    if t == s.GATE_ARITHMETIC: return 4 * p0, 2, p0, None
    if t == s.GATE_POSEIDON: return 135, 0, 123, None
    if t == s.GATE_U32_INTERLEAVE: return 34 * p0, 0, 34 * p0, None
    if t in (s.GATE_UNINTERLEAVE_U32, s.GATE_UNINTERLEAVE_B32): return 67 * p0, 0, 67 * p0, None
    if t == s.GATE_U32_ARITHMETIC: return 38 * p0, 0, 36 * p0, None
    if t == s.GATE_U32_ADD_MANY: return (p0 + 3 + 18) * p1, 0, 21 * p1, None
    if t == s.GATE_U32_SUBTRACTION: return 21 * p0, 0, 19 * p0, None
    if t == s.GATE_U32_RANGE_CHECK: return 17 * p0, 0, 17 * p0, None
    if t == s.GATE_COMPARISON:
        cb = -(-p0 // p1)
        return 4 + 5 * p1 + cb + 1, 0, 2 + 5 * p1 + 1 + (cb + 1) + 2, None
    if t == s.GATE_BASE_SUM: return 1 + p0, 0, 1 + p0, None
    if t == s.GATE_RANDOM_ACCESS:
        copies, extra = p1 & 0xFFFF, p1 >> 16
        return (2 + (1 << p0)) * copies + extra + p0 * copies, extra, copies * (p0 + 2) + extra, None
    if t == s.GATE_ARITHMETIC_EXTENSION: return 8 * p0, 2, 2 * p0, None
    if t == s.GATE_MUL_EXTENSION: return 6 * p0, 1, 2 * p0, None
    if t == s.GATE_REDUCING: return 3 * p0 + 4, 0, 2 * p0, None
    if t == s.GATE_REDUCING_EXTENSION: return 4 * p0 + 4, 0, 2 * p0, None
    if t == s.GATE_EXPONENTIATION: return 2 * p0 + 2, 0, p0 + 1, 4
    if t == s.GATE_COSET_INTERPOLATION:
        ni = ((1 << p0) - 2) // (p1 - 1)
        return 7 + (2 << p0) + 4 * ni, 0, 2 * (2 + 2 * ni), p1
    if t == s.GATE_POSEIDON_MDS: return 48, 0, 24, 1
    raise AssertionError(t)


def _circuits():
    rec = synth.Config.standard_recursion_config
    return [synth.arith_circuit(4, public_inputs=[1, 2], pi_hash=[5, 6, 7, 8]), synth.zkdsa_circuit(3), synth.u32_circuit(6), synth.ecdsa_shape_circuit(7),
            synth.keccak_shape_circuit(6), synth.ext_gates_circuit(4, rec()), synth.recursion_gates_circuit(4, rec(), mix_ext=True)]


def test_traced_builtin_gates_report_their_shape():
    seen = set()
    for desc in _circuits():
        nsel, qdf = int(desc.num_selectors), int(desc.quotient_degree_factor)
        for g in desc.gates:
            t, p0, p1 = int(g["type"]), int(g["p0"]), int(g["p1"])
            if t == synth.GATE_NOOP:
                continue
            wires, consts, constraints, degree = _shape(t, p0, p1)
            assert constraints == int(g["num_constraints"]), (t, p0, p1)
            got = glp.gate_program_circuit_check(pg.trace_gate(desc, g))
            assert got[0] == constraints and got[2] == wires, ((t, p0, p1), got, wires)
            assert got[3] == (nsel + consts if consts else 0), ((t, p0, p1), got, consts)
            if degree is not None:
                assert got[1] == degree, ((t, p0, p1), got)
            # what glp_circuit_create_prog holds the twin to: plonky2's selector grouping leaves room for the body the tests restate
            filt = int(g["group_end"]) - int(g["group_start"]) - 1 + (1 if nsel > 1 else 0)
            assert got[1] + filt <= qdf + 1, ((t, p0, p1), got, filt)
            seen.add(t)
    assert seen == set(range(1, 19)) | {20, 21, 22}, sorted(seen)
