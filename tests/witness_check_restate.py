"""glp_witness_check restated on the CPU: every gate's unfiltered constraints on the rows of H and every copy constraint of one witness,
with the report fields of include/glp.h's glp_witness_report and the failing rows per gate.

The gate of a row follows zeta_identity_recursion.gate_rows, the constraints come from zeta_identity_recursion.gate_constraints over
_Fp (every assigned gate type; types 4-12 and 14 from tests/limb_gates_restate.py), sigma is decoded through a dictionary {k_is[j] w^i: (j, i)}.  Nothing here shares code with
csrc/.  For a gate type without a body here (an unassigned one) the rows, gates and copies are still done and the constraint fields are UNKNOWN."""
import numpy as np

import zeta_identity_recursion as zr
from zeta_identity import P, _Fp

HAS_BODY = tuple(range(19)) + (20, 21, 22)        # every assigned gate type; 19 is unassigned
UNKNOWN = "unknown"
FIELDS = ("failed_constraints", "failed_rows", "failed_copies", "row", "gate", "constraint", "value", "copy_row", "copy_col", "to_col",
          "to_row", "copy_value", "to_value")
POW2_GEN = 1753635133440165772           # of order 2^32


def root_of_unity(lg):
    return pow(POW2_GEN, 1 << (32 - lg), P)


def decode_sigmas(desc):
    """{(j, i): (j', i')} with sigmas[j][i] == k_is[j'] w^i'; KeyError-free: a value on no coset raises ValueError naming it."""
    lg, nr = int(desc.degree_bits), int(desc.num_routed_wires)
    n, w = 1 << lg, root_of_unity(lg)
    table = {}
    for j in range(nr):
        x = int(desc.k_is[j])
        for i in range(n):
            table[x] = (j, i)
            x = x * w % P
    assert len(table) == nr * n, "the cosets k_is[j] H are not distinct"
    out = {}
    for j in range(nr):
        for i in range(n):
            s = int(desc.sigmas[j][i])
            if s not in table:
                raise ValueError("sigmas[%d][%d]" % (j, i))
            out[(j, i)] = table[s]
    return out


def public_inputs_hash(public_inputs):
    from plonky2_lib_amd import poseidon_py
    pi = [int(x) for x in public_inputs]
    return poseidon_py.hash_no_pad(pi) if pi else [0, 0, 0, 0]


def check(desc, wires=None, public_inputs=None, sigma_map=None):
    """(report dict with FIELDS, rows_failed_by_gate list).  Fields of a count that is 0 are None.  In a circuit with a gate type that
    has no body here the constraint fields, and that gate's entry of rows_failed_by_gate, are UNKNOWN; the copies are still done."""
    W = np.asarray(desc.wires if wires is None else wires, np.uint64)
    pih = public_inputs_hash(desc.public_inputs if public_inputs is None else public_inputs)
    nsel, ng = int(desc.num_selectors), len(desc.gates)
    by_gate = [0] * ng
    fails = []                                       # (row, gate, constraint, value)
    total = 0
    unknown_types = False
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        if t not in HAS_BODY:
            unknown_types = True
            continue
        for r in zr.gate_rows(desc, gi):
            r = int(r)
            w = [int(x) for x in W[:, r]]
            gc = [int(x) for x in desc.constants[nsel:, r]]
            vals = zr.gate_constraints(_Fp, g, gc, w, pih)
            assert len(vals) == int(g["num_constraints"])
            bad = [(k, v) for k, v in enumerate(vals) if v]
            if bad:
                by_gate[gi] += 1
                total += len(bad)
                fails.append((r, gi, bad[0][0], bad[0][1]))
    rep = dict.fromkeys(FIELDS)
    rep["failed_constraints"], rep["failed_rows"] = total, len(fails)
    if fails:
        rep["row"], rep["gate"], rep["constraint"], rep["value"] = min(fails)
    if unknown_types:                                # some rows cannot be judged here: nothing about the constraints is claimed
        for f in ("failed_constraints", "failed_rows", "row", "gate", "constraint", "value"):
            rep[f] = UNKNOWN
        by_gate = [UNKNOWN if int(g["type"]) not in HAS_BODY else c for g, c in zip(desc.gates, by_gate)]
    sm = decode_sigmas(desc) if sigma_map is None else sigma_map
    broken = sorted((i, j) for (j, i), (j2, i2) in sm.items() if W[j, i] != W[j2, i2])
    rep["failed_copies"] = len(broken)
    if broken:
        i, j = broken[0]
        j2, i2 = sm[(j, i)]
        rep.update(copy_row=i, copy_col=j, to_col=j2, to_row=i2, copy_value=int(W[j, i]), to_value=int(W[j2, i2]))
    return rep, by_gate


def as_tuple(rep):
    return tuple(rep[f] for f in FIELDS)
