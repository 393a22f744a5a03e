"""plonky2's extension-field gates (ArithmeticExtension, MulExtension, Reducing, ReducingExtension) on the host: the zeta
checker (tests/zeta_identity.py) pinned against oracle proofs, the base-field constraints of the synthetic circuits that carry
these gates, their metadata and the circuit file round trip.  No GPU."""
import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
import zeta_identity as zi

PRESETS = {"rec": synth.Config.standard_recursion_config, "ecc": synth.Config.standard_ecc_config}
CATEGORIES = ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q")


# ---------------------------------------------------------------------------------------------------- (a) checker vs oracle
@pytest.mark.parametrize("preset", sorted(PRESETS))
@pytest.mark.parametrize("hasher", [0, 1])
@pytest.mark.parametrize("nch", [2, 3])
def test_checker_pinned_to_oracle(oracle, preset, hasher, nch):
    """The checker accepts oracle proofs of arith_circuit and rejects each of them when one opening word changes."""
    pi = [9, 1 << 50]
    desc = synth.arith_circuit(4, PRESETS[preset](num_challenges=nch), seed=20 + nch, public_inputs=pi,
                               pi_hash=oracle.hash_no_pad(pi))
    desc.hasher = hasher
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0 and oc.verify(proof) == 0
    assert zi.check(desc, proof, desc.circuit_digest, hasher)
    lay = zi.proof_layout(desc)
    rng = np.random.default_rng(nch + 7 * hasher)
    for name in CATEGORIES:
        o, cnt = lay[name]
        if name == "wires":
            cnt = desc.num_routed_wires          # the advice wires above them are in no constraint of this circuit
        for word in (o, o + 2 * cnt - 1, o + int(rng.integers(0, 2 * cnt))):
            bad = proof.copy()
            bad[word] = (int(bad[word]) + 1) % zi.P
            assert not zi.check(desc, bad, desc.circuit_digest, hasher), (name, word)


# ---------------------------------------------------------------------------------------------------- (b) base-field constraints
def _rows_of(desc, gi):
    assert desc.num_selectors == 1
    return np.nonzero(desc.constants[0] == gi)[0]


def _probe_columns(t, p0):
    """Constrained wires to disturb: both components of the first and last op's output (and an input), or of the first and the
    last accumulator (acc_{N-1} = output) and of alpha / old_acc / a coefficient."""
    if t == synth.GATE_ARITHMETIC_EXTENSION:
        return [6, 7, 8 * (p0 - 1) + 6, 8 * (p0 - 1) + 7, 0, 5]
    if t == synth.GATE_MUL_EXTENSION:
        return [4, 5, 6 * (p0 - 1) + 4, 6 * (p0 - 1) + 5, 1, 2]
    cw = 1 if t == synth.GATE_REDUCING else 2
    a0 = 6 + cw * p0
    return [a0, a0 + 1, 0, 1, 2, 5, 6, 6 + cw * (p0 - 1)]


@pytest.mark.parametrize("preset", sorted(PRESETS))
@pytest.mark.parametrize("lg", [3, 6])
def test_ext_rows_satisfy_their_gates(preset, lg):
    desc = synth.ext_gates_circuit(lg, PRESETS[preset]())
    seen = set()
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        if t not in synth.EXT_GATES:
            continue
        rows = _rows_of(desc, gi)
        assert len(rows) >= 1
        seen.add(t)
        for r in rows:
            assert not any(zi.row_constraints(desc, gi, int(r))), (t, int(r))
        r = int(rows[-1])
        for col in _probe_columns(t, int(g["p0"])):
            keep = int(desc.wires[col, r])
            desc.wires[col, r] = (keep + 1) % zi.P
            assert any(zi.row_constraints(desc, gi, r)), (t, col)
            desc.wires[col, r] = keep
    assert seen == set(synth.EXT_GATES)


@pytest.mark.parametrize("t", synth.EXT_GATES)
def test_each_gate_alone_and_copy_constraints(t):
    """A circuit of one extension gate type; the permutation really runs over its routed wires (non-identity sigmas)."""
    for preset in PRESETS:
        desc = synth.ext_gates_circuit(5, PRESETS[preset](), gates=(t,))
        assert sorted(int(g["type"]) for g in desc.gates) == sorted([0, 1, 2, t])
        gi = next(i for i, g in enumerate(desc.gates) if int(g["type"]) == t)
        for r in _rows_of(desc, gi):
            assert not any(zi.row_constraints(desc, gi, int(r)))
        # sigma != identity on some routed cell of a row of this gate
        n = 1 << desc.degree_bits
        ident = synth.gl.mul(np.asarray(desc.k_is)[:, None], synth.gl.powers(synth.gl.root_of_unity(desc.degree_bits), n)[None, :])
        rows = _rows_of(desc, gi)
        assert (desc.sigmas[:, rows] != ident[:, rows]).any()


def test_copy_constraints_hold():
    """Every permutation cycle connects equal wire values."""
    desc = synth.ext_gates_circuit(7, PRESETS["rec"]())
    n, nr = 1 << desc.degree_bits, desc.num_routed_wires
    sub = synth.gl.powers(synth.gl.root_of_unity(desc.degree_bits), n)
    pos = {int(sub[r]): r for r in range(n)}
    kpos = {int(k): j for j, k in enumerate(desc.k_is)}
    for col in range(nr):
        for row in range(n):
            s = int(desc.sigmas[col, row])
            # sigma = k_is[col'] w^row': recover (col', row') by trying each coset
            found = None
            for k, j in kpos.items():
                x = s * pow(k, zi.P - 2, zi.P) % zi.P
                if x in pos:
                    found = (j, pos[x])
                    break
            assert found is not None
            assert desc.wires[found[0], found[1]] == desc.wires[col, row], (col, row, found)


# ---------------------------------------------------------------------------------------------------- (c) metadata
def test_metadata():
    par = {"rec": {15: 10, 16: 13, 17: 43, 18: 32}, "ecc": {15: 10, 16: 13, 17: 44, 18: 33}}
    for preset, want in par.items():
        cfg = PRESETS[preset]()
        got = synth.ext_gate_params(cfg)
        assert {int(k): v for k, v in got.items()} == want
        for t, p0 in got.items():
            assert synth.ext_gate_wires(t, p0) <= cfg.num_wires
            routed = {15: 8 * p0, 16: 6 * p0, 17: 6 + p0, 18: 6 + 2 * p0}[t]
            assert routed <= cfg.num_routed_wires
        assert synth.ext_gate_wires(17, got[17] + 1) > cfg.num_wires or 6 + got[17] + 1 > cfg.num_routed_wires
        assert synth.ext_gate_wires(18, got[18] + 1) > cfg.num_wires or 6 + 2 * (got[18] + 1) > cfg.num_routed_wires
    for t in synth.EXT_GATES:
        assert synth.gate_num_constraints(t, 7) == 14
    assert [synth.gate_degree(t) for t in synth.EXT_GATES] == [3, 3, 2, 2]
    # build() order: (degree, id string)
    desc = synth.ext_gates_circuit(5, PRESETS["rec"]())
    assert [int(g["type"]) for g in desc.gates] == [0, 1, 2, 18, 17, 15, 16]
    assert [int(g["num_constraints"]) for g in desc.gates][3:] == [64, 86, 20, 26]
    assert desc.num_gate_constraints == 86


def test_existing_circuits_unchanged():
    """The circuits that already exist carry none of the new gate types."""
    for d in (synth.ecdsa_shape_circuit(7), synth.keccak_shape_circuit(6), synth.smt_shape_circuit(5), synth.zkdsa_circuit(3)):
        assert all(int(g["type"]) < 15 for g in d.gates)


# ---------------------------------------------------------------------------------------------------- (d) circuit file
def test_circuit_file_round_trip(tmp_path):
    desc = synth.ext_gates_circuit(6, PRESETS["ecc"](), num_challenges=3)
    path = str(tmp_path / "ext.glpc")
    glp.write_circuit_file(path, desc)
    with glp.CircuitFile(path) as cf:
        d = cf.desc
        assert [{k: int(v) for k, v in g.items()} for g in desc.gates] == [{k: int(g[k]) for k in desc.gates[0]} for g in d.gates]
        assert int(d.num_challenges) == 3 and int(d.num_gate_constraints) == int(desc.num_gate_constraints)
        assert (d.constants == desc.constants).all() and (d.sigmas == desc.sigmas).all() and (d.wires == desc.wires).all()
