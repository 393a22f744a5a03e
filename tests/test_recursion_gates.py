"""The recursion gates (ExponentiationGate, CosetInterpolationGate, PoseidonMdsGate) on the host: the zeta checker of
tests/zeta_identity_recursion.py pinned against oracle proofs, the row constraints of synth.recursion_gates_circuit, what the gates
compute (checked without their recurrences), their shapes, the copy constraints and the circuit file round trip.  No GPU."""
import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
import zeta_identity as zi
import zeta_identity_recursion as zr

P = zi.P
EXP, COSET, MDS = synth.GATE_EXPONENTIATION, synth.GATE_COSET_INTERPOLATION, synth.GATE_POSEIDON_MDS
PRESETS = {"rec": synth.Config.standard_recursion_config, "ecc": synth.Config.standard_ecc_config}
CATEGORIES = ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "q")
# what plonky2 picks under standard_recursion_config; N = 2 without intermediates; N = 16 at the largest degree the config carries
# (chunks 8, 7, 1: a short last chunk); N = 8 at degree 3 (chunks 3, 2, 2, 1) with an odd number of power bits
PARAMS = {
    "default": None,
    "n2": {COSET: (1, 2), EXP: (1, 0)},
    "d8": {COSET: (4, 8), EXP: (7, 0)},
    "odd": {COSET: (3, 3), EXP: (63, 0)},
}
# per parameter set: (constraints, degree, wires, routed wires) of Exponentiation and of CosetInterpolation
SHAPES = {
    "default": ((67, 4, 134, 68), (12, 6, 47, 37)),
    "n2": ((2, 4, 4, 3), (4, 2, 11, 9)),
    "d8": ((8, 4, 16, 9), (12, 8, 47, 37)),
    "odd": ((64, 4, 128, 65), (16, 3, 35, 21)),
}


def _circuit(lg, name="default", preset="rec", **kw):
    return synth.recursion_gates_circuit(lg, PRESETS[preset](), params=PARAMS[name], **kw)


def _gate_index(desc, t):
    return next(i for i, g in enumerate(desc.gates) if int(g["type"]) == t)


# ---------------------------------------------------------------------------------------------------- (a) checker vs oracle
@pytest.mark.parametrize("preset,hasher,nch", [("rec", 0, 2), ("ecc", 1, 2), ("rec", 1, 3), ("ecc", 0, 3)])
def test_checker_pinned_to_oracle(oracle, preset, hasher, nch):
    """Pin before use: the restated identity accepts oracle proofs of circuits over the existing gate set and rejects each of them
    when one opening word changes."""
    pi = [3, 1 << 40]
    desc = synth.arith_circuit(4, PRESETS[preset](num_challenges=nch), seed=40 + nch, public_inputs=pi,
                               pi_hash=oracle.hash_no_pad(pi))
    desc.hasher = hasher
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0 and oc.verify(proof) == 0
    assert zr.check(desc, proof, desc.circuit_digest, hasher)
    lay = zi.proof_layout(desc)
    rng = np.random.default_rng(11 * nch + hasher)
    for name in CATEGORIES:
        o, cnt = lay[name]
        if name == "wires":
            cnt = desc.num_routed_wires          # the advice wires above them are in no constraint of this circuit
        for word in (o, o + 2 * cnt - 1, o + int(rng.integers(0, 2 * cnt))):
            bad = proof.copy()
            bad[word] = (int(bad[word]) + 1) % P
            assert not zr.check(desc, bad, desc.circuit_digest, hasher), (name, word)


# ---------------------------------------------------------------------------------------------------- (b) row constraints
def _role_columns(desc, t, g):
    """{role: wire column} to disturb on a row of gate g."""
    p0, p1 = int(g["p0"]), int(g["p1"])
    if t == EXP:
        return {"power bit": 1 + p0 // 2, "intermediate": p0 + 2 + (p0 - 1) // 2, "output": p0 + 1}
    if t == MDS:
        return {"input": 7}
    lay = zr.coset_layout(p0, p1)
    roles = {"value": lay["values"] + 2 * (lay["n"] - 1) + 1, "evaluation point": lay["point"]}
    if lay["ni"]:
        roles["intermediate prod"] = lay["prods"] + 2 * (lay["ni"] - 1)
    return roles


@pytest.mark.parametrize("name", sorted(PARAMS))
@pytest.mark.parametrize("lg,preset", [(3, "rec"), (6, "ecc")])
def test_rows_satisfy_their_gates_and_perturbations_do_not(name, lg, preset):
    desc = _circuit(lg, name, preset)
    seen = set()
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        if t not in synth.RECURSION_GATES:
            continue
        rows = zr.gate_rows(desc, gi)
        assert len(rows) >= 1
        seen.add(t)
        for r in rows:
            vals = zr.row_constraints(desc, gi, int(r))
            assert len(vals) == int(g["num_constraints"]) and not any(vals), (t, int(r))
        r = int(rows[-1])
        for role, col in _role_columns(desc, t, g).items():
            keep = int(desc.wires[col, r])
            desc.wires[col, r] = (keep + 1) % P
            assert any(zr.row_constraints(desc, gi, r)), (t, role)
            desc.wires[col, r] = keep
    assert seen == set(synth.RECURSION_GATES)


def test_helper_rows_satisfy_their_gates():
    """The BaseSum / ArithmeticExtension rows that feed the new gates, and the ext rows of a mixed circuit."""
    desc = _circuit(5, mix_ext=True)
    types = sorted(int(g["type"]) for g in desc.gates)
    assert types == sorted([0, 1, 2, 13, 15, 16, 17, 18, 20, 21, 22])
    for gi, g in enumerate(desc.gates):
        t = int(g["type"])
        rows = zr.gate_rows(desc, gi)
        for r in rows:                              # every gate of the circuit has a body in the checker
            vals = zr.row_constraints(desc, gi, int(r))
            assert len(vals) == int(g["num_constraints"]) and (t == synth.GATE_PUBLIC_INPUT or not any(vals)), (t, int(r))
        if t == synth.GATE_BASE_SUM:
            r = int(rows[0])
            keep = int(desc.wires[2, r])
            desc.wires[2, r] = 2                    # not a bit
            assert any(zr.row_constraints(desc, gi, r))
            desc.wires[2, r] = keep
            for r in rows:
                limbs = [int(x) for x in desc.wires[1:1 + int(g["p0"]), r]]
                assert set(limbs) <= {0, 1} and sum(b << j for j, b in enumerate(limbs)) == int(desc.wires[0, r])


# ---------------------------------------------------------------------------------------------------- (c) semantics
def _f2mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_exponentiation_is_a_power(name):
    desc = _circuit(5, name)
    gi = _gate_index(desc, EXP)
    n = int(desc.gates[gi]["p0"])
    for r in zr.gate_rows(desc, gi):
        w = [int(x) for x in desc.wires[:, r]]
        assert set(w[1:1 + n]) <= {0, 1}
        assert w[n + 1] == pow(w[0], sum(b << i for i, b in enumerate(w[1:1 + n])), P)


def test_poseidon_mds_is_the_mds_layer():
    from plonky2_lib_amd import poseidon_py as pp
    desc = _circuit(5)
    gi = _gate_index(desc, MDS)
    for r in zr.gate_rows(desc, gi):
        w = [int(x) for x in desc.wires[:, r]]
        for k in range(2):
            assert [w[24 + 2 * i + k] for i in range(12)] == pp._mds([w[2 * i + k] for i in range(12)])


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_coset_interpolation_is_lagrange_interpolation(name):
    """evaluation value = sum_i v_i prod_{j != i} (z - s x_j) / (s x_i - s x_j): the polynomial through (s x_i, v_i) at z, in F_p^2."""
    desc = _circuit(5, name)
    gi = _gate_index(desc, COSET)
    lay = zr.coset_layout(int(desc.gates[gi]["p0"]), int(desc.gates[gi]["p1"]))
    n, xs = lay["n"], zr.subgroup(int(desc.gates[gi]["p0"]))
    for r in zr.gate_rows(desc, gi)[:3]:
        w = [int(x) for x in desc.wires[:, r]]
        s = w[0]
        pts = [s * x % P for x in xs]
        z = (w[lay["point"]], w[lay["point"] + 1])
        total = (0, 0)
        for i in range(n):
            term, den = (w[1 + 2 * i], w[2 + 2 * i]), 1
            for j in range(n):
                if j != i:
                    term = _f2mul(term, ((z[0] - pts[j]) % P, z[1]))
                    den = den * (pts[i] - pts[j]) % P
            di = pow(den, P - 2, P)
            total = ((total[0] + term[0] * di) % P, (total[1] + term[1] * di) % P)
        assert total == (w[lay["value"]], w[lay["value"] + 1]), int(r)


# ---------------------------------------------------------------------------------------------------- (d) shapes
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_shapes(name):
    desc = _circuit(4, name)
    for t, want in zip((EXP, COSET), SHAPES[name]):
        g = desc.gates[_gate_index(desc, t)]
        p0, p1 = int(g["p0"]), int(g["p1"])
        wires, routed = synth.recursion_gate_wires(t, p0, p1)
        assert (int(g["num_constraints"]), synth.gate_degree(t, p0, p1), wires, routed) == want
        assert synth.gate_num_constraints(t, p0, p1) == want[0]
    g = desc.gates[_gate_index(desc, MDS)]
    assert (int(g["num_constraints"]), synth.gate_degree(MDS), synth.recursion_gate_wires(MDS)) == (24, 1, (48, 48))
    lay = zr.coset_layout(*[int(desc.gates[_gate_index(desc, COSET)][k]) for k in ("p0", "p1")])
    assert (lay["wires"], lay["routed"]) == SHAPES[name][1][2:]
    assert int(desc.num_gate_constraints) == max(int(g["num_constraints"]) for g in desc.gates) <= 512


def test_default_parameters():
    assert (EXP, COSET, MDS) == (20, 21, 22) and synth.RECURSION_GATES == (20, 21, 22)
    for preset, cfg in PRESETS.items():
        par = synth.recursion_gate_params(cfg())
        assert par == {EXP: (66 if preset == "rec" else 67, 0), COSET: (4, 6), MDS: (0, 0)}
    assert [synth.coset_degree(b, 8) for b in (1, 2, 3, 4, 5)] == [2, 4, 8, 6, 8]
    # build() order, (degree, id): Noop, Constant, PoseidonMds, PublicInput, BaseSum<2>, ArithmeticExtension, Exponentiation, Coset
    desc = _circuit(5)
    assert [int(g["type"]) for g in desc.gates] == [0, 1, 22, 2, 13, 15, 20, 21]
    assert desc.num_selectors == 2
    synth.recursion_gates_circuit(5, params={COSET: (5, 8)})          # 32 points: 87 wires, 69 routed inputs
    with pytest.raises(ValueError):
        synth.recursion_gates_circuit(5, params={COSET: (6, 8)})      # 64 points: 133 routed inputs


def test_existing_circuits_unchanged():
    for d in (synth.ecdsa_shape_circuit(7), synth.keccak_shape_circuit(6), synth.smt_shape_circuit(5), synth.zkdsa_circuit(3),
              synth.ext_gates_circuit(5)):
        assert all(int(g["type"]) < 19 for g in d.gates)


# ---------------------------------------------------------------------------------------------------- (e) copy constraints
@pytest.mark.parametrize("name,zk", [("default", False), ("odd", False), ("n2", True)])
def test_copy_constraints_hold_and_connect_the_gates(name, zk):
    cfg = synth.Config.standard_recursion_zk_config() if zk else PRESETS["rec"]()
    desc = synth.recursion_gates_circuit(6, cfg, params=PARAMS[name], mix_ext=True, blinding_seed=5 if zk else None)
    n, nr = 1 << desc.degree_bits, desc.num_routed_wires
    ident = synth.gl.mul(np.asarray(desc.k_is)[:, None], synth.gl.powers(synth.gl.root_of_unity(desc.degree_bits), n)[None, :])
    cell = {int(v): (c, r) for c in range(nr) for r, v in enumerate(ident[c])}
    assert len(cell) == nr * n
    target = {}
    for c in range(nr):
        for r in range(n):
            tc, tr = cell[int(desc.sigmas[c, r])]
            assert desc.wires[tc, tr] == desc.wires[c, r], (c, r, tc, tr)
            target[(c, r)] = (tc, tr)
    gi = {t: _gate_index(desc, t) for t in (13, 15, EXP, COSET, MDS)}
    rows = {t: [int(r) for r in zr.gate_rows(desc, i)] for t, i in gi.items()}
    nb = int(desc.gates[gi[EXP]]["p0"])
    lay = zr.coset_layout(int(desc.gates[gi[COSET]]["p0"]), int(desc.gates[gi[COSET]]["p1"]))
    for u in range(len(rows[EXP])):
        bs, ex, ae, co, md = (rows[t][u] for t in (13, EXP, 15, COSET, MDS))
        assert target[(1, ex)] == (1, bs) and target[(min(nb, 63), ex)] == (min(nb, 63), bs)     # power bits <- BaseSum limbs
        assert target[(0, co)] == (nb + 1, ex)                                                   # shift <- Exponentiation output
        assert target[(lay["point"], co)] == (6, ae) and target[(lay["values"] + 1, co)] == (15, ae)   # point, value 0 <- outputs
        assert target[(0, md)] == (lay["value"], co) and target[(1, md)] == (lay["value"] + 1, co)     # MDS input 0 <- result


# ---------------------------------------------------------------------------------------------------- (f) sizes, zk, circuit file
@pytest.mark.parametrize("lg", [3, 4, 10])
def test_sizes_and_zero_knowledge(lg):
    desc = _circuit(lg)
    assert desc.degree_bits == lg and not desc.zero_knowledge
    zk = synth.recursion_gates_circuit(lg, synth.Config.standard_recursion_zk_config(), blinding_seed=3)
    assert zk.zero_knowledge and zk.degree_bits == synth.blinding_counts(synth.Config.standard_recursion_zk_config(), 1 << lg)[2]
    for gi, g in enumerate(zk.gates):
        if int(g["type"]) in synth.RECURSION_GATES:
            rows = zr.gate_rows(zk, gi)
            assert len(rows) and rows.max() < (1 << lg)
            assert not any(zr.row_constraints(zk, gi, int(rows[-1])))


def test_circuit_file_round_trip(tmp_path):
    desc = _circuit(6, "odd", "ecc", mix_ext=True, num_challenges=3)
    path = str(tmp_path / "rec.glpc")
    glp.write_circuit_file(path, desc)
    with glp.CircuitFile(path) as cf:
        d = cf.desc
        assert [{k: int(v) for k, v in g.items()} for g in desc.gates] == [{k: int(g[k]) for k in desc.gates[0]} for g in d.gates]
        assert int(d.num_challenges) == 3 and int(d.num_gate_constraints) == int(desc.num_gate_constraints)
        assert (d.constants == desc.constants).all() and (d.sigmas == desc.sigmas).all() and (d.wires == desc.wires).all()
