"""CPU checks of tests/fri_restate.py, the Python restatement of plonky2's FRI prover and verifier for a general instance that
test_gpu_fri_openings.py holds glp_fri_* to.  The verifier is pinned first, on the FRI slice of the oracle prover's proofs under
the plonk instance (accepts; rejects one changed word per section).  Then the restated prover is pinned against that verifier on
an instance the plonk prover never builds, and its openings against a direct Horner evaluation."""
import numpy as np
import pytest

import plonky2_lib_amd.synth as synth
import fri_restate as fr


def _plonk_fri_slice(oracle, desc):
    """(instance, caps, openings in point order, FriProof words, transcript after the openings) of the oracle prover's proof"""
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0 and oc.verify(proof) == 0
    capw, nch = 4 << desc.cap_height, desc.num_challenges
    caps = [oc.cs_cap] + [proof[k * capw:(k + 1) * capw].reshape(-1, 4) for k in range(3)]
    nopen = (desc.num_constants + desc.num_routed_wires + desc.num_wires + 2 * nch + nch * desc.num_partial_products +
             nch * desc.quotient_degree_factor)
    op = proof[3 * capw:3 * capw + 2 * nopen].reshape(-1, 2)
    ch = oracle.Challenger(oc.hasher)
    ch.observe_hashes(np.asarray(desc.circuit_digest, np.uint64))
    ch.observe(oracle.hash_no_pad(np.asarray(desc.public_inputs, np.uint64)))
    ch.observe_hashes(caps[1])
    ch.get_n(2 * nch)                                        # betas, gammas
    ch.observe_hashes(caps[2])
    ch.get_n(nch)                                            # alphas
    ch.observe_hashes(caps[3])
    zeta = ch.get_ext()
    pts = fr.plonk_openings_to_points(desc, op)
    ch.observe(pts)                                          # to_fri_openings order: the zeta batch, then zs_next
    inst = fr.plonk_instance(desc, zeta)
    start = 3 * capw + 2 * nopen
    words = proof[start:start + inst.layout()[5]].copy()
    assert start + words.size + len(desc.public_inputs) == proof.size
    return inst, caps, pts, words, ch


def _keccak_desc():
    d = synth.arith_circuit(7, synth.Config.standard_recursion_config(), seed=12)
    d.hasher, d.circuit_digest = 1, None
    return d


@pytest.mark.parametrize("which", ["poseidon", "keccak"])
def test_restated_verifier_on_the_oracle_provers_fri(oracle, which):
    desc = synth.arith_circuit(6, synth.Config.standard_recursion_config(), seed=106) if which == "poseidon" else _keccak_desc()
    inst, caps, pts, words, ch = _plonk_fri_slice(oracle, desc)
    assert fr.verify_fri_proof(oracle, inst, caps, pts, words, fr.challenger_clone(oracle, ch)) == 0
    o_q, stride, o_f, final_len, o_pow, total = inst.layout()
    ll0, depth0 = inst.leaf_len[0], inst.lgN - inst.cap_height
    rec = o_q + stride                                       # the second query round
    layer0 = rec + sum(ll + 4 * depth0 for ll in inst.leaf_len)
    places = {"commit cap": 5, "leaf": rec + 3, "path": rec + ll0 + 6, "eval": layer0 + 1,
              "layer path": layer0 + (2 << inst.arity_bits[0]) + 2, "final polynomial": o_f + 1, "witness": o_pow}
    for name, at in places.items():
        bad = words.copy()
        bad[at] = (int(bad[at]) + 1) % fr.P
        assert fr.verify_fri_proof(oracle, inst, caps, pts, bad, fr.challenger_clone(oracle, ch)) != 0, name
    wrong = pts.copy()
    wrong[7, 0] = (int(wrong[7, 0]) + 1) % fr.P              # a claimed opening the proof does not support
    assert fr.verify_fri_proof(oracle, inst, caps, wrong, words, fr.challenger_clone(oracle, ch)) != 0


def shape_b(rng, oracle, log_n, arity_bits, cap_height, rate_bits=3, hasher=0, pow_bits=6, nq=3):
    """The instance of three oracles (5, 3 salted, 41 columns) and three points that the plonk prover never builds; shared with
    test_gpu_fri_openings.py.  -> (instance, coefficient arrays, salts of oracle 1 [N][4])"""
    ncols = [5, 3, 41]
    coeffs = [oracle.rand_field(rng, (c, 1 << log_n)) for c in ncols]
    salts = oracle.rand_field(rng, (1 << (log_n + rate_bits), 4))
    z = [tuple(int(v) for v in oracle.rand_field(rng, 2)) for _ in range(3)]
    points = [(z[0], [(0, 0, 5), (2, 7, 34), (1, 0, 3)]), (z[1], [(2, 0, 3), (2, 20, 2)]), (z[2], [(1, 1, 1)])]
    inst = fr.Instance(log_n, rate_bits, cap_height, hasher, ncols, [False, True, False], points, arity_bits, pow_bits, nq)
    return inst, coeffs, salts


def test_restated_prover_against_the_restated_verifier(oracle):
    rng = np.random.default_rng(505)
    inst, coeffs, salts = shape_b(rng, oracle, 5, [1, 2], 2)
    obs = [fr.commit(oracle, co, inst.rate_bits, inst.cap_height, inst.hasher, salts if s else None) for co, s in zip(coeffs, inst.salted)]
    assert [o.leaves.shape[1] for o in obs] == [5, 7, 41]
    ch = oracle.Challenger(0)
    ch.observe(oracle.rand_field(rng, 11))
    openings, words = fr.prove_openings(oracle, inst, obs, fr.challenger_clone(oracle, ch))
    assert len(openings) == inst.num_openings == 5 + 34 + 3 + 3 + 2 + 1
    k = 0
    for b, (z, _) in enumerate(inst.points):
        for o, c in inst.columns(b):
            acc = (0, 0)
            for cf in coeffs[o][c][::-1]:
                acc = fr.e_add(fr.e_mul(acc, z), (int(cf), 0))
            assert openings[k] == acc, (b, o, c)
            k += 1
    caps = [o.cap for o in obs]
    assert fr.verify_fri_proof(oracle, inst, caps, openings, words, fr.challenger_clone(oracle, ch)) == 0
    o_q, stride, o_f, final_len, o_pow, total = inst.layout()
    assert final_len == 4 and words.size == total
    salted_leaf_end = o_q + 5 + 4 * (inst.lgN - inst.cap_height) + 7 - 1      # the last salt of oracle 1 in the first round
    for at in (0, salted_leaf_end, o_f, o_pow):
        bad = words.copy()
        bad[at] = (int(bad[at]) + 1) % fr.P
        assert fr.verify_fri_proof(oracle, inst, caps, openings, bad, fr.challenger_clone(oracle, ch)) != 0, at
    wrong = list(openings)
    wrong[40] = fr.e_add(wrong[40], (1, 0))
    assert fr.verify_fri_proof(oracle, inst, caps, wrong, words, fr.challenger_clone(oracle, ch)) != 0
    # the witness is the smallest: no candidate below it passes
    wit = int(words[o_pow])
    replay = fr.challenger_clone(oracle, ch)
    replay.get_ext()
    capw = 4 << inst.cap_height
    for r in range(len(inst.arity_bits)):
        replay.observe_hashes(words[r * capw:(r + 1) * capw].reshape(-1, 4))
        replay.get_ext()
    replay.observe(words[o_f:o_f + 2 * final_len])
    for cand in range(wit + 1):
        c2 = fr.challenger_clone(oracle, replay)
        c2.observe([cand])
        assert (c2.get() >> (64 - inst.pow_bits) == 0) == (cand == wit)


def test_periodic_opening_closed_form():
    """fri_restate.periodic_opening, the reference test_gpu_wide_shapes.py opens 2^24 coefficients against, equals Horner over all
    coefficients at sizes Python walks in no time: both coefficient sets of that test and a random one, periods 4 and 2"""
    P = fr.P
    z = (0x0123456789ABCDEF, 0xFEDCBA9876543210 % P)
    rng = np.random.default_rng(14)
    sets = [[P - 2, P - 1, 1, 0x9E3779B97F4A7C15 % P], [P - 2, P - 1, P - 3, P - 4], [int(v) % P for v in rng.integers(0, 1 << 63, 4)], [5, P - 7]]
    for C in sets:
        for log_n in (2, 3, 10):
            coeffs = np.tile(np.array(C, np.uint64), (1 << log_n) // len(C))
            assert fr.periodic_opening(C, log_n, z) == fr.eval_ext(coeffs, z)
            assert fr.periodic_opening(C, log_n, (3, 0)) == fr.eval_ext(coeffs, (3, 0))
