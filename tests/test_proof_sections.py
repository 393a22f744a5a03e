"""tests/proof_sections.py held against the oracle on the CPU, so that the GPU sweeps (test_gpu_verify_sweep.py,
test_gpu_fri_verify_sweep.py) do not trust their own table.

The oracle proves a circuit without reductions and one with three; its verifier must accept the proof, and reject it with the first
word, the last word and a stride sample of every section of every query round (and of the head) damaged in turn: a section whose
range were off by one would put one of those words into a neighbouring section or past the proof.  The ranges must tile the proof.
The oracle has no salted layout (it proves a blinded circuit as an ordinary one, tests/test_zk.py), so the zk map is held to the plain
one through tests/zk_restate.py::strip_salts: without its salt sections it is the plain map, word for word."""
import numpy as np
import pytest

import plonky2_lib_amd.synth as synth
import fri_restate as fr
import proof_sections as ps
import zk_restate as zr

RC = synth.Config.standard_recursion_config
CIRCUITS = {
    "no reduction": lambda: synth.zkdsa_circuit(3),                                                      # 2^3 rows, 28 rounds
    "three reductions": lambda: synth.smt_shape_circuit(5, config=RC(arity_bits=1, final_poly_bits=2, num_query_rounds=5), seed=9),
    "path-free layer": lambda: synth.smt_shape_circuit(5, config=RC(arity_bits=4, final_poly_bits=1, num_query_rounds=3), seed=9),
}
STRIDE = 37


@pytest.fixture(scope="module", params=sorted(CIRCUITS))
def proved(request, oracle):
    desc = CIRCUITS[request.param]()
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0
    return desc, oc, proof


def test_ranges_tile_the_proof(proved):
    desc, oc, proof = proved
    secs = ps.sections(desc)
    assert ps.tiles(secs, proof.size) and proof.size == oc.proof_words
    assert len(ps.section_of(secs)) == proof.size
    nq, nred = int(desc.num_query_rounds), len(desc.reduction_arity_bits)
    for q in range(nq):
        mine = [s for s in secs if s.q == q]
        assert [s.kind for s in mine if s.kind == "leaf"] == ["leaf"] * 4
        assert sum(s.kind == "evals" for s in mine) == nred
    assert sorted(ps.legacy_ranges(desc).values())[-1][1] == proof.size


def test_oracle_rejects_the_ends_of_every_section(proved):
    desc, oc, proof = proved
    assert oc.verify(proof) == 0
    words = ps.sample(ps.sections(desc), STRIDE)
    assert words[0] == 0 and words[-1] == proof.size - 1
    accepted = []
    for at in words:
        bad = proof.copy()
        bad[at] = np.uint64(ps.bumped(bad[at]))
        if oc.verify(bad) == 0:
            accepted.append(at)
    assert accepted == []
    assert oc.verify(proof) == 0


def test_circuits_reach_what_they_claim():
    d = CIRCUITS["no reduction"]()
    assert d.degree_bits == 3 and list(d.reduction_arity_bits) == []
    d = CIRCUITS["three reductions"]()
    assert d.degree_bits == 5 and list(d.reduction_arity_bits) == [1, 1, 1]
    d = CIRCUITS["path-free layer"]()                   # 2^8 points fold to 2^4 = the cap: the layer's path is empty
    assert list(d.reduction_arity_bits) == [4] and not any(s.kind == "layer_path" for s in ps.sections(d))


@pytest.mark.parametrize("which", sorted(CIRCUITS))
def test_zk_map_is_the_plain_map_plus_salts(which):
    desc = CIRCUITS[which]()
    plain, zk = ps.sections(desc, zk=False), ps.sections(desc, zk=True)
    total = ps.total_words(zk)
    nq = int(desc.num_query_rounds)
    assert ps.tiles(zk, total) and total == zr.proof_words(desc, True) == ps.total_words(plain) + 3 * ps.SALT_SIZE * nq
    salts = [s for s in zk if s.kind == "salt"]
    assert [(s.q, s.index) for s in salts] == [(q, k) for q in range(nq) for k in (1, 2, 3)] and all(s.hi - s.lo == 4 for s in salts)
    kept = zr.strip_salts(desc, np.arange(total, dtype=np.uint64))          # kept[i] = the zk word that lands at plain word i
    by = {s.name: s for s in plain}
    for s in zk:
        if s.kind == "salt":
            assert not np.isin(np.arange(s.lo, s.hi), kept).any(), s
        else:
            t = by[s.name]
            assert (kept[t.lo:t.hi] == np.arange(s.lo, s.hi)).all(), s
    # a leaf and its salts are one Merkle leaf: same oracle, same reason
    for s in salts:
        leaf = next(t for t in zk if t.kind == "leaf" and (t.q, t.index) == (s.q, s.index))
        assert leaf.hi == s.lo and ps.reasons(leaf) == ps.reasons(s)


def test_zk_map_of_a_blinded_circuit(oracle):
    """a circuit that carries its blinding rows (2^10 rows at two query rounds): the zk map has the documented length"""
    desc = synth.zkdsa_circuit(config=synth.Config.standard_recursion_zk_config(num_query_rounds=2), blinding_seed=7)
    assert desc.zero_knowledge and desc.degree_bits == 10
    secs = ps.sections(desc)
    assert ps.tiles(secs, zr.proof_words(desc, True)) and sum(s.kind == "salt" for s in secs) == 6
    assert ps.total_words(ps.sections(desc, zk=False)) == oracle.OracleCircuit(desc).proof_words


def test_reasons_follow_the_check_order():
    desc = CIRCUITS["three reductions"]()
    for s in ps.sections(desc):
        r = ps.reasons(s)
        if s.q is None:
            assert r is None and s.kind not in ps.QUERY_KINDS
        elif s.kind == "evals":
            assert r == ("FRI consistency check failed (query %d, reduction %d)" % (s.q, s.index), "Invalid Merkle proof (query %d, reduction %d)" % (s.q, s.index))
        elif s.kind == "layer_path":
            assert r == ("Invalid Merkle proof (query %d, reduction %d)" % (s.q, s.index),)
        else:
            assert r == ("Invalid Merkle proof (query %d, initial tree %d)" % (s.q, s.index),)


def test_fri_sections_equal_the_restated_layout():
    """the bare FriProof of the seam: same offsets as tests/fri_restate.py::Instance.layout, written separately"""
    for ncols, salted, log_n, ab, ch, nq in [([4, 16, 17, 9], [False, True, False, False], 3, [1, 2], 0, 3), ([5, 3, 41], [False, True, False], 5, [4], 2, 3),
                                             ([5, 3, 41], [False, True, False], 5, [], 1, 2)]:
        inst = fr.Instance(log_n, 3, ch, 0, ncols, salted, [((1, 2), [(0, 0, 1)])], ab, 6, nq)
        o_q, stride, o_f, final_len, o_pow, total = inst.layout()
        secs = ps.fri_sections(ncols, salted, log_n, 3, ch, ab, nq)
        assert ps.tiles(secs, total)
        by = {s.name: s for s in secs}
        assert by["q0_leaf0"].lo == o_q and by["final_poly"] == ps.Section("final_poly", "final_poly", o_f, o_f + 2 * final_len, None, None)
        assert by["pow"].lo == o_pow and (nq < 2 or by["q1_leaf0"].lo == o_q + stride)
        assert [by["q0_leaf%d" % k].hi - by["q0_leaf%d" % k].lo + (4 if s else 0) for k, s in enumerate(salted)] == inst.leaf_len
