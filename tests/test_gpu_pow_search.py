"""The proof-of-work searches on the device against the CPU restatement tests/pow_restate.py: k_pow (glp_pow_search, glp_pow_search_h,
stepped by the host), k_pow_batch<Keccak> and k_pow_prepare + k_pow_batch2 (glp_pow_search_many).  Every expected witness is the
restatement's -- one state at a time, the oracle's whole permutation per candidate -- never another device path's, and the
comparison is equality of the witness word.  The shapes are the smallest that reach each mechanism (csrc/fri_kernels.inc):
  positions   the candidate in each of the eight rate slots: mds_entry(r, pos) and RC[pos] of the collapsed round 0
  ownership   K around 256 and far past it: thread t owns proofs t, t + 256, ..., a scan over four waves ranks the open ones
  depth       witnesses many chunks deep, where give_up fires, and beyond what the workgroups that leave can cover (tail_from)
  chunk edges witnesses 0, 255, 256; the second launch of the single search's host loop
  field edges sponge words at 0, p - 1, 2^32 +- 1, ... and words that make Poseidon's first S-box input 0, 1, p - 1
The reference costs about 20 us per candidate, so the references shared by several tests are computed once (module fixtures) and
`bits` is kept low; the whole file evaluates about 0.6 M permutations on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
import pow_restate as pr

pytestmark = pytest.mark.gpu

P = pr.P
POW_MAX_BITS = 32
HASHERS = [pr.POSEIDON, pr.KECCAK]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pow_states.npz")
NP_POOL = 3                   # pending inputs of the pooled sponges (and of the fixtures)


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def single(ctx, hasher, st, pend, bits, plain=False):
    """glp_pow_search_h (plain: glp_pow_search, Poseidon only) on one sponge"""
    st, pend = np.ascontiguousarray(st, np.uint64), np.ascontiguousarray(pend, np.uint64)
    L, w = glp.load_library(), C.c_uint64(2 ** 64 - 1)
    pp = binding._p(pend) if pend.size else None
    if plain:
        binding._chk(L.glp_pow_search(ctx._h, binding._p(st), pp, pend.size, bits, C.byref(w)))
    else:
        binding._chk(L.glp_pow_search_h(ctx._h, hasher, binding._p(st), pp, pend.size, bits, C.byref(w)))
    return int(w.value)


def many(ctx, hasher, states, pending, bits):
    return [int(w) for w in ctx.pow_search_many(hasher, states, pending, bits)]


def restated(oracle, hasher, states, pending, bits):
    return [pr.smallest_witness(oracle, hasher, s, p, bits, 1 << 22) for s, p in zip(states, pending)]


def _mismatch(got, want):
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    return "%d of %d differ, first at proof %d: got %d, restated %d" % (len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]) if bad else ""


class Pool:
    """4096 random sponges per hasher with NP_POOL pending inputs, and their restated witnesses at the `bits` asked for (kept)"""

    def __init__(self, oracle):
        self.oracle = oracle
        rng = np.random.default_rng(4096)
        self.states = {h: oracle.rand_field(rng, (4096, 12)) for h in HASHERS}
        self.pending = {h: oracle.rand_field(rng, (4096, NP_POOL)) for h in HASHERS}
        self._want = {}

    def want(self, hasher, bits, K):
        have = self._want.setdefault((hasher, bits), [])
        if len(have) < K:
            have += restated(self.oracle, hasher, self.states[hasher][len(have):K], self.pending[hasher][len(have):K], bits)
        return have[:K]


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


@pytest.fixture(scope="module")
def fixtures(oracle):
    """{hasher: {kind: [(state, pending, bits, witness)]}} of pow_states.npz, every witness restated here once more"""
    z, out = np.load(GOLDEN), {}
    for hasher, name in ((pr.POSEIDON, "poseidon"), (pr.KECCAK, "keccak")):
        by = out.setdefault(hasher, {})
        for k, kind in enumerate(z[name + "_kind"]):
            st, pend, bits = z[name + "_state"][k].copy(), z[name + "_pending"][k].copy(), int(z[name + "_bits"][k])
            assert pend.size == NP_POOL
            w = pr.smallest_witness(oracle, hasher, st, pend, bits, 1 << 22)
            assert w == int(z[name + "_witness"][k])
            by.setdefault(str(kind), []).append((st, pend, bits, w))
    return out


# ------------------------------------------------------------------ positions
@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("num_pending", range(8))
def test_every_candidate_position(ctx, oracle, hasher, num_pending):
    """the candidate in rate slot num_pending, through the single search and through the batch search (K = 3)"""
    bits, K = 7, 3
    rng = np.random.default_rng(700 + 8 * hasher + num_pending)
    states, pending = oracle.rand_field(rng, (K, 12)), oracle.rand_field(rng, (K, num_pending))
    want = restated(oracle, hasher, states, pending, bits)
    assert [single(ctx, hasher, states[k], pending[k], bits) for k in range(K)] == want
    assert many(ctx, hasher, states, pending, bits) == want
    if hasher == pr.POSEIDON:
        assert single(ctx, hasher, states[0], pending[0], bits, plain=True) == want[0]


# ------------------------------------------------------------------ ownership and ranking
@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("K", [1, 2, 255, 256, 257, 600, 4096])
def test_many_proofs_bits4(ctx, pool, hasher, K):
    got = many(ctx, hasher, pool.states[hasher][:K], pool.pending[hasher][:K], 4)
    assert not _mismatch(got, pool.want(hasher, 4, K))


@pytest.mark.parametrize("hasher", HASHERS)
def test_4096_proofs_bits0(ctx, pool, hasher):
    """no condition: every witness is 0 (the restatement says so without hashing)"""
    want = pool.want(hasher, 0, 4096)
    assert want == [0] * 4096
    assert not _mismatch(many(ctx, hasher, pool.states[hasher], pool.pending[hasher], 0), want)


@pytest.mark.parametrize("hasher", HASHERS)
def test_reversed_order_gives_reversed_witnesses(ctx, pool, hasher):
    """300 sponges dealt in the opposite order: a proof's witness does not depend on its index or on its neighbours"""
    K = 300
    got = many(ctx, hasher, pool.states[hasher][:K][::-1], pool.pending[hasher][:K][::-1], 4)
    assert not _mismatch(got, pool.want(hasher, 4, K)[::-1])


# ------------------------------------------------------------------ depth
@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("K,bits", [(24, 12), (2, 15)])
def test_deep_witnesses(ctx, pool, hasher, K, bits):
    """witnesses spread over many chunks of 256 candidates: proofs close at different times, chunks in flight are given up"""
    want = pool.want(hasher, bits, K)
    assert max(want) >= 256 * 8
    assert not _mismatch(many(ctx, hasher, pool.states[hasher][:K], pool.pending[hasher][:K], bits), want)


# ------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("hasher", HASHERS)
def test_witness_past_the_workgroups_that_leave(ctx, fixtures, hasher):
    """K = 1, witness >= 2048: the body of the launch is one workgroup that leaves after 8 chunks of 256 candidates, so the witness is
    reached by the tail workgroups (tail_from ..) alone; without them the search ends with GLP_ERR_PROVE.  That they STAY is held by
    test_more_chunks_wanted_than_leaving_workgroups_grant, not here (profiles/r18_pow_search_tests.txt)"""
    for st, pend, bits, w in fixtures[hasher]["a"]:
        assert w >= 2048 and many(ctx, hasher, st[None], pend[None], bits) == [w]
        assert single(ctx, hasher, st, pend, bits) == w


@pytest.mark.parametrize("hasher", HASHERS)
def test_more_chunks_wanted_than_leaving_workgroups_grant(ctx, fixtures, hasher):
    """4096 copies of a deep state (witness w >= 2048 at bits = 8): every proof needs its chunks 0 .. w / 256, 4096 * 12 = 49 152
    chunks for w = 2826.  The Poseidon launch is 4 * 4096 / 8 + 1 = 2049 workgroups that leave after 8 chunks and 4 per CU that
    stay: if none stayed, all of them together would grant (2049 + 4 * CUs) * 8 chunks -- 24 584 at 256 CUs, fewer than wanted
    up to 750 CUs -- and proofs would end open (GLP_ERR_PROVE).  The searches finish only because the tail workgroups stay; the
    restated witness is the one of the fixture.  (Keccak's k_pow_batch has only workgroups that stay: the same demand, for symmetry.)"""
    K = 4096
    st, pend, bits, w = fixtures[hasher]["a"][0]
    assert bits == 8 and K * (w // 256 + 1) > (4 * K // 8 + 1 + 4 * 750) * 8
    got = many(ctx, hasher, np.repeat(st[None], K, axis=0), np.repeat(pend[None], K, axis=0), bits)
    assert not _mismatch(got, [w] * K)


@pytest.mark.parametrize("hasher", HASHERS)
def test_fixtures_in_a_crowd(ctx, pool, fixtures, hasher):
    """the deep states at indices 0, 256 and 299 and the chunk-edge states at 1, 255 and 257 of 300 sponges at bits = 8"""
    K, bits = 300, 8
    states, pending, want = pool.states[hasher][:K].copy(), pool.pending[hasher][:K].copy(), list(pool.want(hasher, bits, K))
    a, c = fixtures[hasher]["a"], [fixtures[hasher][k][0] for k in ("c0", "c255", "c256")]
    for idx, (st, pend, b, w) in zip((0, 256, 299, 1, 255, 257), (a[0], a[1], a[0], c[0], c[1], c[2])):
        assert b == bits
        states[idx], pending[idx], want[idx] = st, pend, w
    assert [want[i] for i in (1, 255, 257)] == [0, 255, 256] and min(want[0], want[256]) >= 2048
    assert not _mismatch(many(ctx, hasher, states, pending, bits), want)


@pytest.mark.parametrize("hasher", HASHERS)
def test_chunk_edges(ctx, fixtures, hasher):
    """witnesses 0, 255 and 256: the last candidate of chunk 0 and the first of chunk 1, alone, together and through the single search"""
    rows = [fixtures[hasher][k][0] for k in ("c0", "c255", "c256")]
    assert [r[3] for r in rows] == [0, 255, 256]
    for st, pend, bits, w in rows:
        assert many(ctx, hasher, st[None], pend[None], bits) == [w]
        assert single(ctx, hasher, st, pend, bits) == w
    assert many(ctx, hasher, np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), 8) == [0, 255, 256]


@pytest.mark.parametrize("hasher", HASHERS)
def test_single_search_second_launch(ctx, fixtures, hasher):
    """bits = 12: the host steps k_pow in launches of 2^14 candidates; this witness lies in the second"""
    (st, pend, bits, w), = fixtures[hasher]["b"]
    assert bits == 12 and w >= 1 << 14
    assert single(ctx, hasher, st, pend, bits) == w
    if hasher == pr.POSEIDON:
        assert single(ctx, hasher, st, pend, bits, plain=True) == w
    assert many(ctx, hasher, st[None], pend[None], bits) == [w]


# ------------------------------------------------------------------ identical sponges
@pytest.mark.parametrize("hasher", HASHERS)
def test_identical_sponges(ctx, pool, hasher):
    K = 300
    w = pool.want(hasher, 8, 1)[0]
    got = many(ctx, hasher, np.repeat(pool.states[hasher][:1], K, axis=0), np.repeat(pool.pending[hasher][:1], K, axis=0), 8)
    assert not _mismatch(got, [w] * K)


# ------------------------------------------------------------------ field edges
@pytest.mark.parametrize("hasher", HASHERS)
@pytest.mark.parametrize("num_pending", [0, 5])
def test_edge_sponges(ctx, oracle, hasher, num_pending):
    """64 sponges of edge words (pow_restate.edge_sponges; tests/test_pow_search.py checks what the set contains).  With nothing
    pending the candidate takes slot 0 and slots 1..11 count; with five pending it takes slot 5 and slots 0..4 arrive as pending
    inputs: between the two runs every slot's edge words reach the permutation."""
    bits = 6
    states, pending = pr.split(pr.edge_sponges(), num_pending)
    want = restated(oracle, hasher, states, pending, bits)
    assert not _mismatch(many(ctx, hasher, states, pending, bits), want)
    assert not _mismatch([single(ctx, hasher, states[k], pending[k], bits) for k in range(len(want))], want)


# ------------------------------------------------------------------ refusals
def _refused(fn):
    with pytest.raises(glp.GlpError) as e:
        fn()
    return e.value.code, str(e.value)


def test_refusals(ctx, oracle):
    """a sponge word that is no field element is GLP_ERR_ARG at each of the five entries, named; what was refused before still is"""
    rng = np.random.default_rng(5)
    L = glp.load_library()
    co = oracle.rand_field(rng, (3, 3, 32))
    shared, m3 = ctx.batch_from_coeffs(co[0], 3, 2), ctx.batch_many_from_coeffs(co, 3, 2)
    ranges = [((5, 9), [(0, 0, 3)]), ((11, 13), [(0, 1, 2)])]
    zs = oracle.rand_field(rng, (3, 2, 2))
    st3, pend3 = oracle.rand_field(rng, (3, 12)), oracle.rand_field(rng, (3, 2))
    w3 = np.zeros(3, np.uint64)

    def search_many(st, pend, K=3, npend=2, bits=4, hasher=0):
        binding._chk(L.glp_pow_search_many(ctx._h, hasher, K, binding._p(st), binding._p(pend), npend, bits, binding._p(w3)))

    entries = {
        "glp_pow_search": lambda st, pend: single(ctx, 0, st[0], pend[0], 4, plain=True),
        "glp_pow_search_h": lambda st, pend: single(ctx, 1, st[0], pend[0], 4),
        "glp_pow_search_many": search_many,
        "glp_fri_prove": lambda st, pend: glp.fri_prove(ctx, [shared], ranges, [2], 4, 2, st[0], pend[0]),
        "glp_fri_prove_many": lambda st, pend: glp.fri_prove_many(ctx, [m3], ranges, zs, [2], 4, 2, st, pend),
    }
    for name, call in entries.items():
        call(st3, pend3)                                         # the call itself is a good one
        is_many = name.endswith("many")
        for bad in (P, 2 ** 64 - 1):
            k = 2 if is_many else 0
            st = st3.copy()
            st[k, 11] = bad
            code, msg = _refused(lambda: call(st, pend3))
            assert code == -1 and "canonical" in msg and ("sponge_states[2][11]" if is_many else "sponge_state[11]") in msg, (name, msg)
            pend = pend3.copy()
            pend[k, 1] = bad
            code, msg = _refused(lambda: call(st3, pend))
            assert code == -1 and "canonical" in msg and ("pending_inputs[2][1]" if is_many else "pending_inputs[1]") in msg, (name, msg)
        st = st3.copy()
        st[:, 4] = P - 1                                         # the largest field element is one
        call(st, pend3)
    # as before: 8 pending inputs, too many bits, no proofs or too many, an unknown hasher
    st8, pend8, w = oracle.rand_field(rng, (4097, 12)), oracle.rand_field(rng, (4097, 8)), C.c_uint64()
    for rc in (L.glp_pow_search(ctx._h, binding._p(st8), binding._p(pend8), 8, 4, C.byref(w)),
               L.glp_pow_search_h(ctx._h, 0, binding._p(st8), binding._p(pend8), 8, 4, C.byref(w)),
               L.glp_pow_search_many(ctx._h, 0, 3, binding._p(st8), binding._p(pend8), 8, 4, binding._p(w3))):
        assert rc == -1 and b"pending" in L.glp_last_error()
    for rc in (L.glp_pow_search(ctx._h, binding._p(st8), binding._p(pend8), 2, POW_MAX_BITS + 1, C.byref(w)),
               L.glp_pow_search_h(ctx._h, 1, binding._p(st8), binding._p(pend8), 2, POW_MAX_BITS + 1, C.byref(w)),
               L.glp_pow_search_many(ctx._h, 1, 3, binding._p(st8), binding._p(pend8), 2, POW_MAX_BITS + 1, binding._p(w3))):
        assert rc == -1 and b"proof_of_work_bits" in L.glp_last_error()
    big = np.zeros(4097, np.uint64)
    for K in (0, 4097):
        assert L.glp_pow_search_many(ctx._h, 0, K, binding._p(st8), binding._p(pend8), 2, 4, binding._p(big)) == -1
        assert b"num_proofs" in L.glp_last_error()
    assert L.glp_pow_search_h(ctx._h, 2, binding._p(st8), binding._p(pend8), 2, 4, C.byref(w)) == -3 and b"hasher" in L.glp_last_error()
    assert L.glp_pow_search_many(ctx._h, 2, 3, binding._p(st8), binding._p(pend8), 2, 4, binding._p(w3)) == -3 and b"hasher" in L.glp_last_error()
    d, keep = binding._fri_desc_to_c([shared], ranges, [2], 4, 2)
    op, proof = np.zeros((5, 2), np.uint64), np.zeros(glp.fri_proof_words([shared], [2], 2), np.uint64)
    assert L.glp_fri_prove(ctx._h, C.byref(d), binding._p(st8), binding._p(pend8), 8, binding._p(op), binding._p(proof)) == -1
    assert b"pending" in L.glp_last_error()
    del keep
    d, keep = binding._fri_desc_to_c([m3], ranges, [2], 4, 2)
    op, proof = np.zeros((3, 5, 2), np.uint64), np.zeros((3, glp.fri_proof_words([m3], [2], 2)), np.uint64)
    assert L.glp_fri_prove_many(ctx._h, C.byref(d), 3, binding._p(zs), binding._p(st8), binding._p(pend8), 8, binding._p(op), binding._p(proof)) == -1
    assert b"pending" in L.glp_last_error()
    del keep
    for b in (shared, m3):
        b.free()
