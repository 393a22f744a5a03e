"""The CPU restatement of the proof-of-work search (tests/pow_restate.py) held to the oracle's Challenger, the fixtures of
tests/golden/pow_states.npz derived again from it in full, and the edge-state set of the GPU tests checked for what it claims to
contain.  No GPU: tests/test_gpu_pow_search.py compares the device searches with the same restatement."""
import os

import numpy as np
import pytest

import fri_restate as fr
import pow_restate as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pow_states.npz")
P = pr.P


@pytest.mark.parametrize("hasher", [pr.POSEIDON, pr.KECCAK])
@pytest.mark.parametrize("num_pending", range(8))
def test_restated_witness_is_the_smallest_the_challenger_accepts(oracle, hasher, num_pending):
    """A Challenger that has observed 8 j + num_pending words (num_pending = 0: the rate just filled, the sponge permuted) observes
    the witness and squeezes: `bits` leading zeros for the restated witness, and for no candidate below it."""
    bits = 6
    rng = np.random.default_rng(100 + 8 * hasher + num_pending)
    ch = oracle.Challenger(hasher)
    ch.observe(oracle.rand_field(rng, 8 * (1 + num_pending % 2) + num_pending))
    st, pend = fr.challenger_state(ch)
    assert pend.size == num_pending
    w = pr.smallest_witness(oracle, hasher, st, pend, bits, 1 << 12)

    def squeezed(cand):
        c2 = fr.challenger_clone(oracle, ch)
        c2.observe([cand])
        return c2.get()
    assert squeezed(w) >> (64 - bits) == 0
    assert all(squeezed(c) >> (64 - bits) != 0 for c in range(w))
    assert squeezed(w) == pr.response(oracle, hasher, st, pend, w)
    assert pr.smallest_witness(oracle, hasher, st, pend, 0, 1) == 0
    with pytest.raises(ValueError):
        pr.smallest_witness(oracle, hasher, st, pend, bits, w)           # the limit is exclusive, and nothing lies below w


def test_restatement_refuses_what_is_not_a_sponge(oracle):
    st = np.zeros(12, np.uint64)
    for bad in ([P], [2 ** 64 - 1]):
        with pytest.raises(AssertionError):
            pr.response(oracle, pr.POSEIDON, st, bad, 0)
    with pytest.raises(AssertionError):
        pr.response(oracle, pr.POSEIDON, st, [0] * 8, 0)


@pytest.mark.parametrize("name,hasher", [("poseidon", pr.POSEIDON), ("keccak", pr.KECCAK)])
def test_fixture_witnesses_derive_again(oracle, name, hasher):
    """every stored witness, searched for from candidate 0 (a stale or edited file fails here, without a GPU)"""
    z = np.load(GOLDEN)
    kinds = [str(k) for k in z[name + "_kind"]]
    assert sorted(kinds) == ["a", "a", "b", "c0", "c255", "c256"]
    for k, kind in enumerate(kinds):
        st, pend, bits, w = z[name + "_state"][k], z[name + "_pending"][k], int(z[name + "_bits"][k]), int(z[name + "_witness"][k])
        assert pend.size == 3 and all(int(v) < P for v in st) and all(int(v) < P for v in pend)
        assert pr.smallest_witness(oracle, hasher, st, pend, bits, w + 1) == w, (name, kind)
        if kind == "a":
            assert bits == 8 and w >= 2048        # 8 chunks of 256: what one workgroup that leaves covers
        elif kind == "b":
            assert bits == 12 and w >= 1 << 14    # the first launch of the single search: 2^max(14, bits + 2) candidates
        else:
            assert bits == 8 and w == int(kind[1:])
    assert len({int(w) for w, kind in zip(z[name + "_witness"], kinds) if kind == "a"}) == 2


def test_edge_sponges_hold_what_they_claim():
    """for every slot 0..11: a sum with the round-0 constant that wraps 64 bits, one that is exactly p, and S-box inputs 0, 1, p - 1;
    every word canonical, every one of EDGE_WORDS present; split() hands the first words over as pending inputs and hides them"""
    sp = pr.edge_sponges()
    rc = pr.round0_constants()
    assert sp.shape == (64, 12) and len(rc) == 12 and all(0 < c < P for c in rc)
    words = {int(v) for v in sp.reshape(-1)}
    assert all(v < P for v in words) and set(pr.EDGE_WORDS) <= words
    assert (1 << 63) % P == 1 << 63
    for i in range(12):
        sums = [int(v) + rc[i] for v in sp[:, i]]
        assert any(s >= 1 << 64 for s in sums), i
        assert P in sums, i
        assert {0, 1, P - 1} <= {s % P for s in sums}, i
    for num_pending in range(8):
        st, pend = pr.split(sp, num_pending)
        assert pend.shape == (64, num_pending) and (pend == sp[:, :num_pending]).all() and (st[:, num_pending:] == sp[:, num_pending:]).all()
        assert num_pending == 0 or (st[:, :num_pending] != sp[:, :num_pending]).any()
