"""The edge table of tests/witness_edge_rows.py on the CPU: its coverage (computed from the restated fill, never from the library), the
restated constraints on every row, the oracle's prover, verifier and generators on the circuits of gate types up to 14, and one
demonstration that a single wrong cell on any edge row is caught by the comparisons the GPU module makes.  No GPU."""
import numpy as np
import pytest

import plonky2_lib_amd.synth as synth
import limb_gates_restate as lg
import witness_check_restate as wr
import witness_edge_rows as we
import witness_fill_restate as wf
import zeta_identity_recursion as zr

P = we.P
CIRCUITS = {ec.name: ec for ec in we.circuits()}
# rows the issue's table lists as out of domain that the gates' constraints accept (the gates range-check their outputs, not their
# inputs): they stand in the in-domain circuits
MOVED = [
    ("U32Arithmetic", "operands ('0x100000000', '0x100000000', '0x0')", "in"),                        # 2^64 = 2^32 - 1 in the field
    ("U32Arithmetic", "operands ('0xffffffff00000000', '0xffffffff00000000', '0xffffffff00000000')", "in"),     # (-1)(-1) - 1 = 0
    ("U32Arithmetic", "operands ('0x100000000', '0x1', '0xffffffff00000000')", "in"),                 # 2^32 - 1
    ("U32AddMany", "3 addends and the carry all ('0x100000000',)", "in"),                             # carry 4, result 0
    ("U32Subtraction", "operands ('0xffffffff00000000', '0x0', '0x0')", "in"),                        # -1: a borrow, result 2^32 - 1
    ("U32Subtraction", "operands ('0x0', '0x100000000', '0x0')", "in"),                               # p - 2^32: a borrow, result 0
    ("U32Subtraction", "operands ('0x0', '0xffffffff00000000', '0x0')", "in"),                        # 0 - (-1) = 1
    ("U32Subtraction", "operands ('0x5', '0x2', '0xffffffff00000000')", "in"),                        # 5 - 2 + 1 = 4
    ("Comparison", "10/4 first = 2^bits", "in"),                                                      # 4 chunks of 3 bits hold 12 bits
    ("CosetInterpolation", "16 points, shift 0x0, point 0", "in"),                                    # 0 * 0 = 0
    ("CosetInterpolation", "8 points, shift 0x0, point 0", "in"),
]


def _rows(t, in_domain=True):
    """[(wires after the restated fill, Row)] of type t"""
    return [(we.row_cells(r, we._config(r.kind).num_wires)[0], r) for r in we.classified(t)[0 if in_domain else 1]]


def test_every_generator_type_has_rows():
    assert set(wf.GENERATOR_TYPES) == {1} | set(range(3, 19)) | {20, 21, 22} and len(wf.GENERATOR_TYPES) == 20
    for t in wf.GENERATOR_TYPES:
        assert len(we.classified(t)[0]) >= 1, t
    with_out = {t for t in wf.GENERATOR_TYPES if we.classified(t)[1]}
    # the other gates' generators are total: every input has satisfying outputs (U32Arithmetic by the moves above)
    assert with_out == {4, 5, 9, 10, 11, 12, 13, 14, 21}
    assert {ec.type for ec in CIRCUITS.values() if ec.in_domain} == set(wf.GENERATOR_TYPES)


def test_moves_are_the_documented_ones():
    assert [m for t in wf.GENERATOR_TYPES for m in we.classified(t)[2]] == MOVED


def test_branches_are_reached():
    M32 = we.M32
    inv = {w[6 * i + 5] == 0 for w, r in _rows(8) for i in range(r.kind[1])}
    assert inv == {True, False}
    assert any(w[6 * i + 4] == M32 and w[6 * i + 3] == 0 and w[6 * i + 5] == 0 for w, r in _rows(8) for i in range(r.kind[1]))
    borrow = {w[5 * i + 4] for w, r in _rows(10) for i in range(r.kind[1])}
    assert borrow == {0, 1}
    assert any((w[5 * i] - w[5 * i + 1] - w[5 * i + 2]) % P == P - (1 << 32) for w, r in _rows(10) for i in range(r.kind[1]))
    carries = {(r.kind[1], w[(r.kind[1] + 3) * i + r.kind[1] + 2]) for w, r in _rows(9) for i in range(r.kind[2])}
    assert {(na, 0) for na in range(1, 16)} | {(na, na) for na in range(1, 16)} <= carries and (15, 15) in carries
    for nb, nc in ((32, 16), (10, 4)):
        lay = lg.comparison_layout(nb, nc)
        rows = [w for w, r in _rows(12) if r.kind == (12, nb, nc)]
        assert {w[2] for w in rows} == {0, 1}
        eq = [[w[lay["equal"] + i] for i in range(nc)] for w in rows]
        assert [1] * nc in eq                                                        # all chunks equal
        assert [0] + [1] * (nc - 1) in eq and [1] * (nc - 1) + [0] in eq              # only the bottom / only the top chunk differs
        assert {w[2] for w, e in zip(rows, eq) if e == [0] + [1] * (nc - 1)} == {0, 1}
        assert {w[2] for w, e in zip(rows, eq) if e == [1] * (nc - 1) + [0]} == {0, 1}
    ra = lg.random_access_layout(*we.classified(14)[0][0].kind[1:])
    idx = {w[ra["per_copy"] * c] for w, r in _rows(14) for c in range(ra["copies"])}
    assert {0, ra["size"] - 1} <= idx
    exp = _rows(20)
    nb = exp[0][1].kind[1]
    assert any(w[0] == 0 and not any(w[1:1 + nb]) and w[nb + 1] == 1 for w, r in exp)            # 0^0 = 1
    assert any(w[0] == 0 and any(w[1:1 + nb]) and w[nb + 1] == 0 for w, r in exp)
    for w, r in _rows(21):
        lay = zr.coset_layout(*r.kind[1:])
        x = (w[lay["shifted"]], w[lay["shifted"] + 1])
        xs = zr.subgroup(r.kind[1])
        if x[1] == 0 and x[0] in xs and w[0]:
            j = xs.index(x[0])
            assert (w[lay["value"]], w[lay["value"] + 1]) == (w[1 + 2 * j], w[2 + 2 * j]), r.label      # on the coset: the value there
    on = {(r.kind, xs_j) for w, r in _rows(21) for xs_j in (0, (1 << r.kind[1]) - 1)
          if w[0] and (w[zr.coset_layout(*r.kind[1:])["shifted"]], w[zr.coset_layout(*r.kind[1:])["shifted"] + 1]) == (zr.subgroup(r.kind[1])[xs_j], 0)}
    assert len(on) == 4                                                              # j = 0 and j = n - 1, both parameter sets
    assert any(w[zr.coset_layout(*r.kind[1:])["shifted"] + 1] != 0 for w, r in _rows(21))            # and points off it
    assert {w[0] for w, r in _rows(21)} >= {0, 1, 7, P - 1}
    assert {w[lg.POS_SWAP] for w, r in _rows(4)} == {0, 1} and {w[lg.POS_SWAP] for w, r in _rows(4, False)} == {2}
    assert any(all(v == P - 1 for v in w[:24]) for w, r in _rows(22))


def test_selector_polynomials():
    sel = {ec.name: int(ec.desc.num_selectors) for ec in CIRCUITS.values()}
    assert 1 in sel.values() and max(sel.values()) >= 2, sel
    assert sel["U32AddMany-in"] >= 2 and len(CIRCUITS["U32AddMany-in"].desc.gates) == 16
    for ec in CIRCUITS.values():
        assert ec.desc.degree_bits == max(3, (len(ec.rows) - 1).bit_length())
        assert (np.asarray(ec.desc.sigmas) == synth.gl.mul(np.asarray(ec.desc.k_is)[:, None],
                                                           synth.gl.powers(synth.gl.root_of_unity(ec.desc.degree_bits), 1 << ec.desc.degree_bits)[None, :])).all()


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_restated_constraints_decide(name):
    """in-domain: every constraint of every row is zero after the restated fill, and the fill is a fixed point; out of domain: every
    table row fails"""
    ec = CIRCUITS[name]
    rep, by_gate = wr.check(ec.desc)
    assert rep["failed_copies"] == 0
    if ec.in_domain:
        assert wr.as_tuple(rep) == (0, 0, 0) + (None,) * 10
    else:
        assert rep["failed_rows"] == len(ec.rows) and rep["row"] == 0
    for only_advice in (False, True):
        assert we.first_mismatch(wf.fill(ec.desc, ec.desc.wires, only_advice), ec.desc.wires) is None
    again = wf.fill(ec.desc, we.scramble_outputs(ec, 3))
    if ec.type != lg.RANDOM_ACCESS or ec.in_domain:
        assert we.first_mismatch(again, ec.desc.wires) is None


@pytest.mark.parametrize("name", sorted(n for n, ec in CIRCUITS.items() if ec.type <= 14))
def test_oracle_on_the_early_types(oracle, name):
    """the oracle proves the in-domain circuit and its verifier accepts (the restated identity at zeta too); its generators agree with
    the restated ones cell for cell on every circuit, out of domain included, in both modes"""
    ec = CIRCUITS[name]
    desc = ec.desc
    assert desc.proof_of_work_bits == 0
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0
    assert (oc.verify(proof) == 0) == ec.in_domain
    assert zr.check(desc, proof, desc.circuit_digest, 0) == ec.in_domain
    for only_advice in (False, True):
        w = we.scramble_outputs(ec, 5)
        assert we.first_mismatch(oc.witness_fill(w, only_advice=only_advice), wf.fill(desc, w, only_advice)) is None


def test_one_wrong_cell_on_any_edge_row_is_caught():
    """what the GPU module compares a fill against is the restated fill: with one role-1 cell of it off by one, on any edge row, the
    comparison names that cell, and on an in-domain row the restated checker rejects the witness as well"""
    rng = np.random.default_rng(1)
    for ec in list(CIRCUITS.values()) + [we.subtraction_across_workgroups()]:
        want = wf.fill(ec.desc, we.scramble_outputs(ec, 7))
        mask = we.role_mask(ec.desc)
        for r in ec.row_of:
            cols = np.nonzero(mask[:, r])[0]
            c = int(cols[rng.integers(0, len(cols))])
            wrong = want.copy()
            wrong[c, r] = (int(wrong[c, r]) + 1) % P
            assert we.first_mismatch(wrong, want) == (c, r, int(wrong[c, r]), int(want[c, r]))
            if ec.in_domain and r == ec.row_of[0]:
                rep, _ = wr.check(ec.desc, wrong)
                assert rep["failed_rows"] == 1 and rep["row"] == r, (ec.name, c)


def test_workgroup_circuit():
    ec = we.subtraction_across_workgroups()
    assert ec.desc.degree_bits == 9 and ec.row_of[:4] == [0, 255, 256, 511]
    gi = next(i for i, g in enumerate(ec.desc.gates) if int(g["type"]) == lg.U32_SUBTRACTION)
    assert sorted(int(r) for r in zr.gate_rows(ec.desc, gi)) == sorted(ec.row_of)
    assert wr.as_tuple(wr.check(ec.desc)[0])[:3] == (0, 0, 0)
