"""The proof-of-work search (plonky2 `fri_proof_of_work`, smallest witness) restated on the CPU, as plainly as it can be said: one
sponge state per call, Python integers, the oracle's full permutation once per candidate.  Nothing of the device kernels' shortcuts
is repeated here (no collapsed first round, no single output row, no batching), so that a mistake in one of them cannot hide in
its own reference.  Test infrastructure: tests/test_pow_search.py pins it to the oracle's Challenger, tests/test_gpu_pow_search.py
takes every expected witness from it, tests/golden/make_golden.py finds the fixtures of pow_states.npz with it."""
import numpy as np

P = 0xFFFFFFFF00000001
POSEIDON, KECCAK = 0, 1

# permutations evaluated since the module was loaded (the budget of the GPU test file is counted in these)
permutations = 0


def response(oracle, hasher, state12, pending, witness):
    """output word 7 of the permuted sponge: `pending` over slots 0.., `witness` in the slot after them.  This is the challenge a
    duplex Challenger squeezes first after observing the witness (it pops its output buffer from the back of the rate)."""
    global permutations
    pending = [int(v) for v in pending]
    assert len(pending) < 8
    st = [int(v) for v in np.asarray(state12, dtype=np.uint64).reshape(12)]
    st[:len(pending)] = pending
    st[len(pending)] = int(witness)
    assert all(0 <= v < P for v in st), "not canonical"
    permute = oracle.keccak_permute if int(hasher) == KECCAK else oracle.poseidon_permute
    permutations += 1
    return int(permute(np.array(st, dtype=np.uint64))[7])


def smallest_witness(oracle, hasher, state12, pending, bits, limit):
    """the smallest w in [0, limit) whose response has `bits` leading zero bits; ValueError if there is none below `limit`"""
    bits = int(bits)
    assert 0 <= bits <= 64
    for w in range(int(limit)):
        if bits == 0 or response(oracle, hasher, state12, pending, w) >> (64 - bits) == 0:
            return w
    raise ValueError("no witness with %d leading zero bits below %d" % (bits, limit))


# ---------------------------------------------------------------- sponge words at the edges of the field
EDGE_WORDS = (0, 1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 0xFFFFFFFF00000000, (1 << 63) % P)


def round0_constants():
    """the twelve round-0 constants of Poseidon from the oracle's generator (oracle/gen_poseidon_constants.py writes the table the
    oracle is compiled from, oracle/poseidon_constants.h; tests/test_oracle_poseidon.py holds the two together)"""
    from oracle.gen_poseidon_constants import all_round_constants
    words = all_round_constants()
    assert len(words) == 360
    return [int(w) for w in words[:12]]


def edge_sponges(count=64, seed=64):
    """[count][12] sponges (pending inputs and state in one: split() takes them apart), every word one of EDGE_WORDS, except that
    row 3 i + d carries p - RC[i] + d - 1 in slot i (d = 0, 1, 2): Poseidon's first S-box of that slot then sees p - 1, 0 and 1, and
    the sum of the word and its round constant is p - 1, p and p + 1 before reduction.  The rows from 36 on are EDGE_WORDS only."""
    assert count >= 36
    rng = np.random.default_rng(seed)
    rc = round0_constants()
    out = np.array(EDGE_WORDS, dtype=np.uint64)[rng.integers(0, len(EDGE_WORDS), size=(count, 12))]
    for i in range(12):
        for d in range(3):
            out[3 * i + d, i] = P - rc[i] + d - 1
    assert all(int(v) < P for v in out.reshape(-1))
    return out


def split(sponges, num_pending):
    """(states [K][12], pending [K][num_pending]) that describe `sponges`: the first num_pending words of each are handed over as
    pending inputs, and the state carries other words in their slots (the search must write the pending inputs over them)"""
    sp = np.ascontiguousarray(sponges, dtype=np.uint64).reshape(-1, 12)
    states = sp.copy()
    states[:, :num_pending] = sp[:, 11:11 - num_pending:-1] if num_pending else sp[:, :0]
    return states, sp[:, :num_pending].copy()
