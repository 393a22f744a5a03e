"""The vanishing identity at zeta for caller-held circuits (glp_gate_program_eval_ext, glp_perm_check_zeta), the part that needs no GPU.
1. the pin: programs traced from the gate bodies of zeta_identity (and zeta_identity_recursion), run by the restated F_p^2
   interpreter on the openings of oracle proofs and then through the restated permutation check (tests/gate_program_ext_restate.py),
   give zeta_identity.check's verdict: accepted on the proof, and the same verdict on copies with one opening word changed, in every
   opening section.  (The oracle proves arith_circuit; for the two circuits whose gates it has no bodies for, see `proved`.)
2. the restated interpreter at a point of the base field is the base-field restatement (gate_program_restate.run).
3. the new functions are declared, exported and bound.
The device side is tests/test_gpu_zeta_check.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
from plonky2_lib_amd import gate_program as gp
import plonky2_lib_amd.gl_numpy as gl
import plonky2_lib_amd.synth as synth
import gate_program_ext_restate as gx
import gate_program_restate as gr
import zeta_identity as zi
import zeta_identity_recursion as zr

NEW = ["glp_gate_program_eval_ext", "glp_perm_check_zeta"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = zi.P
SECTIONS = ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q")


@functools.lru_cache(maxsize=None)
def proved(name):
    """(desc, traced program, the restatement to agree with, an oracle proof)"""
    from oracle import oracle
    oracle.build()
    pi = [5, 1 << 44]
    if name == "arith":
        desc = synth.arith_circuit(4, synth.Config.standard_ecc_config(), seed=23, public_inputs=pi, pi_hash=oracle.hash_no_pad(pi))
        prog, check = gr.trace_circuit(desc)[0], zi.check
    elif name == "ext":
        desc = synth.ext_gates_circuit(4, public_inputs=pi, pi_hash=oracle.hash_no_pad(pi))
        prog, check = gr.trace_circuit(desc)[0], zi.check
    else:
        desc = synth.recursion_gates_circuit(5, synth.Config.standard_recursion_config())
        prog, check = gx.trace_circuit(desc, zr.gate_constraints), zr.check
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0 and oc.verify(proof) == 0
    if name != "arith":
        # The oracle has no bodies for the extension and recursion gates: its quotient leaves their constraints out, and the checker
        # rightly rejects its proof.  Every other opening is a true opening of the circuit's polynomials, so the quotient opening is
        # solved for from the restatement's own left side; `check` shares nothing with it and accepts only if that side is right.
        assert not check(desc, proof, desc.circuit_digest)
        proof = gx.with_solved_quotient(desc, prog, proof, desc.circuit_digest)
    return desc, prog, check, proof


def tampered(desc, proof, seed):
    """(section, word, copy with 1 added to that word): the first, the last and a random word of every opening section"""
    lay = zi.proof_layout(desc)
    rng = np.random.default_rng(seed)
    for name in SECTIONS:
        o, cnt = lay[name]
        for word in sorted({o, o + 2 * cnt - 1, o + int(rng.integers(0, 2 * cnt))}):
            bad = np.array(proof, np.uint64)
            bad[word] = (int(bad[word]) + 1) % P
            yield name, word, bad


@pytest.mark.parametrize("name", ["arith", "ext", "recursion"])
def test_restatements_pinned_to_the_zeta_identity(name):
    desc, prog, check, proof = proved(name)
    assert check(desc, proof, desc.circuit_digest)
    assert gx.check_proof(desc, prog, proof, desc.circuit_digest) == ""
    caught = set()
    for section, word, bad in tampered(desc, proof, 3):
        want = check(desc, bad, desc.circuit_digest)
        why = gx.check_proof(desc, prog, bad, desc.circuit_digest)
        assert (why == "") == want, (section, word, why)
        assert why == "" or why.startswith("Mismatch between evaluation and opening of quotient polynomial (challenge ")
        if why:
            caught.add(section)
    assert caught == set(SECTIONS), "no changed word was rejected in %s" % (set(SECTIONS) - caught,)


def test_a_quotient_word_names_its_challenge():
    desc, prog, _check, proof = proved("arith")
    o, cnt = zi.proof_layout(desc)["q"]
    qdf = int(desc.quotient_degree_factor)
    assert cnt == int(desc.num_challenges) * qdf
    for c in range(int(desc.num_challenges)):
        bad = np.array(proof, np.uint64)
        bad[o + 2 * (c * qdf + 1)] = (int(bad[o + 2 * (c * qdf + 1)]) + 1) % P
        assert gx.check_proof(desc, prog, bad, desc.circuit_digest) == gx.MISMATCH % c


def test_zeta_one_and_the_absent_gate_term():
    desc, prog, _check, proof = proved("arith")
    betas, gammas, alphas, zeta, pih = zi.challenges(desc, proof, desc.circuit_digest)
    op = gx.proof_openings(desc, proof)
    args = (op["sigmas"], op["wires"], op["zs"] + op["pp"], op["zs_next"], op["q"], betas, gammas, alphas)
    qdf = int(desc.quotient_degree_factor)
    assert gx.perm_check(desc, qdf, (1, 0), *args) == gx.ZETA_IS_ONE
    sums = gx.run_ext(prog, [op["constants"] + op["sigmas"], op["wires"]], None, zeta, alphas, pih)
    assert gx.perm_check(desc, qdf, zeta, *args, gate_sums=sums) == ""
    # the gate constraints vanish on H, not at zeta: their share is not zero there, and leaving it out is a mismatch
    assert any(s != (0, 0) for s in sums) and gx.perm_check(desc, qdf, zeta, *args) == gx.MISMATCH % 0


def test_at_a_base_field_point_the_reading_is_the_provers():
    """second component 0 everywhere: run_ext on one row of the coset is gate_program_restate.run on that row"""
    rng = np.random.default_rng(8)
    asm = gp.Assembler([4, 3], num_params=2)
    T = gp.TraceField(asm)
    for gate in range(3):
        vs = [T.mul(T.add(asm.col(0, j), asm.x), T.sub(asm.col_next(1, (j + gate) % 3), asm.param(j % 2))) for j in range(4)]
        for v in vs + [asm.col(1, gate)]:
            asm.emit(v)
        asm.end(T.sub(asm.col(0, gate), T.lift(3)))
    prog = asm.assemble(hoist_emits=True)
    lg, sub_bits = 3, 1
    M, S = 1 << (lg + sub_bits), 1 << sub_bits
    rows = [gl.rand(rng, (M, c)) for c in (4, 3)]
    alphas, params = gl.rand(rng, (3,)), gl.rand(rng, (2,))
    want = gr.run(prog, rows, sub_bits, alphas, params)
    x = gr.coset_points(lg, sub_bits)
    for i in (0, 5, M - 1):
        at = [[(int(v), 0) for v in r[i]] for r in rows]
        nxt = [[(int(v), 0) for v in r[(i + S) % M]] for r in rows]
        got = gx.run_ext(prog, at, nxt, (int(x[i]), 0), alphas, params)
        assert got == [(int(want[c][i]), 0) for c in range(3)], i


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
    assert hasattr(glp.GateProgram, "eval_ext") and hasattr(glp.Context, "perm_check_zeta") and callable(glp.plonk_ext_openings)
    # the C struct: two pointers and a size_t
    assert binding._ExtOpenings.at_next.offset == 8 and binding._ExtOpenings.proof_stride.offset == 16 and C.sizeof(binding._ExtOpenings) == 24
    hdr = open(os.path.join(ROOT, "include", "glp.h")).read()
    assert "} glp_ext_openings;" in hdr
    # null arguments are refused by name, no context needed
    assert L.glp_gate_program_eval_ext(None, None, 1, 1, None, None, 0, None, None, None, 0) == -1 and b"ctx" in L.glp_last_error()
    assert L.glp_perm_check_zeta(None, None, 1, 1, None, None, None, None, None, 0, None, None, None, None, 0, None, None) == -1
    assert b"glp_perm_check_zeta" in L.glp_last_error() and b"ctx" in L.glp_last_error()


def test_the_slicing_helper_follows_the_order_of_glp_fri_open():
    import fri_restate as fr
    desc, _prog, _check, proof = proved("arith")
    lay = zi.proof_layout(desc)
    count = sum(cnt for _o, cnt in (lay[s] for s in SECTIONS))
    start = lay["constants"][0]
    op = fr.plonk_openings_to_points(desc, proof[start:start + 2 * count])
    two = np.stack([op, op[::-1]])                                 # two proofs: the stride is one proof's words
    parts = glp.plonk_ext_openings(desc, two)
    assert parts["count"] == count and op.shape == (count, 2)
    want = gx.proof_openings(desc, proof)
    flat = two.reshape(-1)

    def read(e, polys, next_=False, k=0):
        assert e.proof_stride == 2 * count and not e.on_device
        at = (e.at_next if next_ else e.at) + k * e.proof_stride
        return gx.pairs(flat[at:at + 2 * polys])
    assert read(parts["program"][0], len(want["constants"]) + len(want["sigmas"])) == want["constants"] + want["sigmas"]
    assert read(parts["program"][1], len(want["wires"])) == want["wires"] == read(parts["wires"], len(want["wires"]))
    assert read(parts["sigmas"], len(want["sigmas"])) == want["sigmas"]
    assert read(parts["zs"], len(want["zs"]) + len(want["pp"])) == want["zs"] + want["pp"]
    assert read(parts["zs_next"], len(want["zs_next"])) == want["zs_next"]
    assert read(parts["quotient"], len(want["q"])) == want["q"]
    assert read(parts["wires"], 1, k=1) == gx.pairs(two[1].reshape(-1)[parts["wires"].at:parts["wires"].at + 2])
    c = parts["zs"]._c()
    assert c.at == flat.ctypes.data + 8 * parts["zs"].at or c.at == parts["zs"].array.ctypes.data + 8 * parts["zs"].at
    assert c.at_next is None and c.proof_stride == 2 * count
