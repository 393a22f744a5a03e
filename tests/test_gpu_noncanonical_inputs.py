"""Words >= p at every field input of the library (include/glp.h, conventions paragraph).

A HOST array with such a word is refused by name before anything is launched: code -1, a message with the parameter, the position and
"canonical", in-place arrays untouched, and the context serves the next canonical call correctly.  A DEVICE array is reduced mod p as
it is loaded: every result is word for word the CPU oracle's result for `input % p`, every word handed back is < p, and the caller's
buffer is not written to.  Seeds are taken mod p.

The arrays come from tests/noncanonical_inputs.py: `single` (one word of NC at the first, the last and a seeded middle position),
`pairs` (the partners of the first butterfly and an adjacent pair hold (0, 2^64 - 1), (2^64 - 1, 2^64 - 1), (p, 0): glf::sub and
glf::add are wrong on them unreduced) and `twin` (at least a quarter of the words lifted by p).  Shapes: the smallest that reaches each
first reader of raw words in the inverse transform (ntt.hip intt_values_to_coeffs), and the largest log_n that reader serves."""
import ctypes as C

import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
from plonky2_lib_amd import binding

import coset_quotient as cq
import noncanonical_inputs as nc
import perm_restate as pr
import witness_edge_rows as we
import witness_fill_restate as wf

pytestmark = pytest.mark.gpu

P = nc.P
U = np.uint64


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


class Dev:
    """an array in a device buffer of the context; on exit the buffer must still hold exactly what was uploaded"""

    def __init__(self, ctx, arr, check_unchanged=True):
        self.ctx, self.arr, self.check = ctx, np.ascontiguousarray(arr, U), check_unchanged

    def __enter__(self):
        self.ptr = self.ctx.dev_alloc(self.arr.nbytes)
        self.ctx.dev_upload(self.ptr, self.arr)
        return self.ptr

    def __exit__(self, et, ev, tb):
        back = np.empty_like(self.arr)
        try:
            if et is None and self.check:
                self.ctx.dev_download(self.ptr, back)
        finally:
            self.ctx.dev_free(self.ptr)
        if et is None and self.check:
            assert (back == self.arr).all(), "the caller's device input was written to"


def _variants(seed, shape, singles=True):
    """name -> (array, A = array % p): twin, pairs, and a single word of NC at the first, the last and a seeded middle position"""
    out = {"twin": nc.twin(seed, shape)}
    nc.check_twin(*out["twin"])
    if shape[-1] >= 2:
        out["pairs"] = nc.pairs(seed, shape)
    if singles:
        size = int(np.prod(shape))
        for pos in nc.single_positions(seed, size):
            for k, word in enumerate(nc.NC):
                out["single 0x%x @%d" % (word, pos)] = nc.single(seed + k, shape, word, pos)
    for arr, A in out.values():
        assert (nc.reduced(arr) == A).all() and (A < U(P)).all()
    assert all((arr >= U(P)).any() for arr, _ in out.values())
    return out


def _combined(seed, shape):
    """one array for a shape whose oracle reference takes seconds: the twin, with the three kinds of pairs at fixed butterfly partners
    and adjacent places and the five words of NC at the first places, the last places and around the middle on top; A = array % p"""
    arr, _ = nc.twin(seed, shape)
    cols = arr.reshape(-1, shape[-1])
    n = shape[-1]
    for k, (a, b) in enumerate(nc.PAIRS):
        c, i, j = k % len(cols), 1000 + 77 * k, 2 * (3000 + 91 * k)
        cols[c, i], cols[c, i + n // 2], cols[c, j], cols[c, j + 1] = U(a), U(b), U(a), U(b)
    flat = arr.reshape(-1)
    for k, word in enumerate(nc.NC):
        flat[k], flat[flat.size - 1 - k], flat[flat.size // 2 + 3 * k] = U(word), U(word), U(word)
    A = nc.reduced(arr)
    nc.check_twin(arr, A)
    return {"twin + pairs + singles": (arr, A)}


def _check_batch(oracle, b, ref, lg, rb, full):
    """coefficients, cap, (digests and the whole LDE | sampled leaves and paths) against the oracle's batch; every word < p"""
    N = 1 << (lg + rb)
    co = b.coeffs()
    assert (co < U(P)).all(), "a stored coefficient is >= p"
    assert (co == ref.coeffs).all(), "coefficients: first mismatch at %s" % (tuple(np.argwhere(co != ref.coeffs)[0]),)
    cap = b.cap()
    assert (cap == ref.cap).all() and (cap < U(P)).all()
    if full:
        assert (b.digests() == ref.digests).all()
        rows = b.lde_values(0, b.ncols, rb)                                  # row i = leaf bitrev(i)
        assert (rows < U(P)).all(), "an LDE value is >= p"
        assert (rows == ref.leaves[oracle.bitrev_perm(lg + rb)]).all()
    elif N * b.ncols <= 1 << 23:                                             # too many digests to bring back: the whole LDE still is
        rows = b.lde_values(0, b.ncols, rb)
        assert (rows < U(P)).all(), "an LDE value is >= p"
        assert (rows == ref.leaves[oracle.bitrev_perm(lg + rb)]).all()
    for j in sorted({0, N - 1, (N // 3) | 1 if N > 2 else 0}):
        leaf = b.leaf(j)
        assert (leaf == ref.leaves[j]).all() and (leaf < U(P)).all(), j
        assert (b.prove(j) == ref.prove(j)).all()


def _cap_h(lg, rb):
    return min(4, lg + rb)


# ------------------------------------------------------------------------------------------ commitments from device words
# (log_n, columns, rate_bits): the first reader of the raw words in intt_values_to_coeffs / intt_chunk
FROM_VALUES = [
    (0, 3, 3), (1, 3, 3), (2, 3, 3), (4, 3, 3),        # k_intt_small<L>: loads straight into dft_reg_dif
    (5, 3, 3), (8, 3, 3),                              # k_intt_contig, B < 4096: the first reader is a mul
    (9, 3, 3), (12, 3, 3),                             # k_intt_contig (2^9 .. 2^11), k_intt_contig16 (2^12): a mul again
    (13, 3, 3), (16, 3, 1),                            # strided first: k_outer<true, 1, false> .. k_outer<true, 4, false>
    (17, 3, 1), (19, 3, 1),                            # k_strided16e<true, 1> .. <true, 3>
    (20, 3, 1),                                        # k_strided16<true>
    (21, 1, 1),                                        # k_strided32<true, 4, LW>
]


@pytest.mark.parametrize("lg,ncols,rb", FROM_VALUES, ids=["2^%d x %d" % (s[0], s[1]) for s in FROM_VALUES])
def test_from_values_device(ctx, oracle, lg, ncols, rb):
    small = lg <= 13
    cases = _variants(100 + lg, (ncols, 1 << lg)) if small else _combined(100 + lg, (ncols, 1 << lg))
    for name, (arr, A) in cases.items():
        ref = oracle.batch_from_values(A, rb, _cap_h(lg, rb))
        with Dev(ctx, arr) as d:
            b = ctx.batch_from_values_device(d, ncols, lg, rb, _cap_h(lg, rb))
            try:
                _check_batch(oracle, b, ref, lg, rb, full=small)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))
            finally:
                b.free()


def test_from_values_device_three_passes(ctx, oracle):
    """2^23 points, one column: k_outer<true, 3, true> reads the raw words.  The coefficients against the oracle's inverse transform and
    two leaves against its coset evaluation; the tree of 2^23 leaves is left to the smaller shapes."""
    lg = 23
    (t_arr, t_A), = _combined(124, (1, 1 << lg)).values()
    want = oracle.ifft(t_A[0])
    with Dev(ctx, t_arr) as d:
        b = ctx.batch_from_values_device(d, 1, lg, 0, 4)
        co = b.coeffs()
        leaves = [(j, b.leaf(j)) for j in (0, (1 << lg) - 1)]
        b.free()
    assert (co < U(P)).all() and (co[0] == want).all()
    lde = oracle.lde(want, 0, 7)
    br = oracle.bitrev_perm(lg)
    for j, leaf in leaves:
        assert int(leaf[0]) == int(lde[br[j]]) and int(leaf[0]) < P


@pytest.mark.parametrize("lg", [2, 6, 9, 13])
def test_from_coeffs_device(ctx, oracle, lg):
    """the coefficient copy a from_coeffs batch keeps (glp_batch_coeffs hands it back) is canonical too"""
    ncols, rb = 3, 3
    for name, (arr, A) in _variants(200 + lg, (ncols, 1 << lg)).items():
        ref = oracle.batch_from_coeffs(A, rb, _cap_h(lg, rb))
        with Dev(ctx, arr) as d:
            b = ctx.batch_from_coeffs_device(d, ncols, lg, rb, _cap_h(lg, rb))
            try:
                _check_batch(oracle, b, ref, lg, rb, full=True)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))
            finally:
                b.free()


def _many_on_device(ctx, fn, dptr, K, ncols, lg, rb, ch, hasher=0, seed=None):
    sd = None if seed is None else np.ascontiguousarray(seed, U)
    h = C.c_void_p()
    binding._chk(getattr(binding.load_library(), fn)(ctx._h, C.c_void_p(dptr), 1, K, ncols, lg, rb, ch, hasher, None if sd is None else binding._p(sd),
                                                     C.byref(h)))
    b = glp.Batch(ctx, h, ncols, lg, rb, ch)
    b.hasher = hasher
    return b


def _salted(oracle, ref, seed, k, ch):
    import zk_restate as zr
    N = ref.leaves.shape[0]
    leaves = np.concatenate([ref.leaves, zr.salt_columns(oracle, list(seed[:3]) + [(int(seed[3]) + k) % P], zr.TAG_BATCH, N)], axis=1)
    return leaves, oracle.merkle_build(leaves, ch)[1]


@pytest.mark.parametrize("lg", [3, 7])
@pytest.mark.parametrize("seed", [None, (5, 6, 7, 8)], ids=["plain", "salted"])
def test_many_from_values_on_device(ctx, oracle, lg, seed):
    K, ncols, rb = 3, 3, 2
    ch = _cap_h(lg, rb)
    for name, (arr, A) in _variants(300 + lg, (K, ncols, 1 << lg), singles=False).items():
        with Dev(ctx, arr) as d:
            b = _many_on_device(ctx, "glp_batch_many_from_values", d, K, ncols, lg, rb, ch, seed=seed)
            caps = b.caps()
            for k in range(K):
                ref = oracle.batch_from_values(A[k], rb, ch)
                m = b.member(k)
                assert (m.coeffs() == ref.coeffs).all(), (name, k)
                if seed is None:
                    _check_batch(oracle, m, ref, lg, rb, full=True)
                else:
                    leaves, cap = _salted(oracle, ref, seed, k, ch)
                    assert (caps[k] == cap).all(), (name, k)
                    for j in (0, leaves.shape[0] - 1):
                        assert (m.leaf(j) == leaves[j]).all()
                assert (caps[k] < U(P)).all()
            b.free()


def test_many_from_coeffs_on_device(ctx, oracle):
    K, ncols, lg, rb = 3, 3, 3, 2
    for name, (arr, A) in _variants(350, (K, ncols, 1 << lg), singles=False).items():
        with Dev(ctx, arr) as d:
            b = _many_on_device(ctx, "glp_batch_many_from_coeffs", d, K, ncols, lg, rb, 2)
            for k in range(K):
                _check_batch(oracle, b.member(k), oracle.batch_from_coeffs(A[k], rb, 2), lg, rb, full=True)
            b.free()


def test_from_coset_values_on_device(ctx, oracle):
    """values on g <W_M>: coset_ifft(g) per polynomial on the CPU, chunks of n, from_coeffs"""
    lg, sb, rb, npoly = 5, 2, 3, 3
    n, M = 1 << lg, 1 << (lg + sb)
    for name, (arr, A) in _variants(400, (npoly, M), singles=True).items():
        chunks = np.stack([oracle.coset_ifft(A[p], 7) for p in range(npoly)]).reshape(npoly << sb, n)
        ref = oracle.batch_from_coeffs(chunks, rb, 4)
        with Dev(ctx, arr) as d:
            b = ctx.batch_from_coset_values(None, sb, rb, 4, dev_ptr=d, shape=(npoly, M))
            try:
                _check_batch(oracle, b, ref, lg, rb, full=True)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))
            finally:
                b.free()


def test_from_coset_values_on_device_one_plane(ctx, oracle):
    """sub_bits = 0: no k_coset_to_planes in front, the inverse transform reads the caller's words itself (k_intt_small here)"""
    lg, rb, npoly = 3, 2, 3
    for name, (arr, A) in _variants(410, (npoly, 1 << lg), singles=False).items():
        ref = oracle.batch_from_coeffs(np.stack([oracle.coset_ifft(A[p], 7) for p in range(npoly)]), rb, 2)
        with Dev(ctx, arr) as d:
            b = ctx.batch_from_coset_values(None, 0, rb, 2, dev_ptr=d, shape=(npoly, 1 << lg))
            try:
                _check_batch(oracle, b, ref, lg, rb, full=True)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))
            finally:
                b.free()


# ------------------------------------------------------------------------------------------ proving from device wires
CIRCUITS = {
    "zkdsa 2^3": lambda: synth.zkdsa_circuit(3),                                   # wires through k_intt_small, k_pp_rows_small
    "keccak shape 2^6": lambda: synth.keccak_shape_circuit(6, seed=9),
    "ecdsa shape 2^7": lambda: synth.ecdsa_shape_circuit(7, seed=9),
    "arith 2^13": lambda: synth.arith_circuit(13, synth.Config.standard_ecc_config(), seed=113),   # strided first reader, k_pp_rows
}


def _proof_words_canonical(proof, desc):
    if int(getattr(desc, "hasher", 0)) == 0:            # KeccakHash<25> digests are bytes, not field elements
        assert (proof < U(P)).all(), "proof word %d is >= p" % int(np.argmax(proof >= U(P)))


def _same_proof(got, ref, what):
    assert (got == ref).all(), "%s: first mismatch at word %d" % (what, int(np.argmax(got != ref)))


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_prove_device(ctx, oracle, name):
    """an (unsatisfying) twin witness in HBM: the proof is OracleCircuit.prove(witness % p) in every word"""
    desc = CIRCUITS[name]()
    arr, A = nc.twin(500, desc.wires.shape)
    nc.check_twin(arr, A)
    oc, gc = oracle.OracleCircuit(desc), glp.Circuit(ctx, desc)
    rc, ref = oc.prove(wires=A)
    with Dev(ctx, arr) as d:
        got = gc.prove_device(d)
    _same_proof(got, ref, name)
    _proof_words_canonical(got, desc)
    gc.free()


def test_prove_device_pairs_at_2_3(ctx, oracle):
    """the zkdsa wires are committed through k_intt_small: the butterfly pairs in three wire columns"""
    desc = synth.zkdsa_circuit(3)
    arr, A = nc.pairs(510, desc.wires.shape)
    oc, gc = oracle.OracleCircuit(desc), glp.Circuit(ctx, desc)
    rc, ref = oc.prove(wires=A)
    with Dev(ctx, arr) as d:
        got = gc.prove_device(d)
    _same_proof(got, ref, "pairs")
    gc.free()


def test_prove_device_keccak_config(ctx, oracle):
    desc = synth.zkdsa_circuit(3)
    desc.hasher, desc.circuit_digest = 1, None
    gc = glp.Circuit(ctx, desc)
    desc.circuit_digest = gc.digest()
    oc = oracle.OracleCircuit(desc, cs_cap=gc.constants_sigmas_cap())
    arr, A = nc.twin(520, desc.wires.shape)
    rc, ref = oc.prove(wires=A)
    with Dev(ctx, arr) as d:
        got = gc.prove_device(d)
    _same_proof(got, ref, "KeccakGoldilocksConfig")
    gc.free()


def test_prove_device_zero_knowledge(oracle):
    """a blinded circuit: the salted wires tree is the oracle's LDE of witness % p under the restated salts, at every query"""
    from test_gpu_zk import SEED, _check_zk_proof, _zkdsa
    desc = _zkdsa(4)
    arr, A = nc.twin(530, desc.wires.shape)
    with glp.Context(0) as c2:
        c2.set_salt_seed([SEED[0] + P, SEED[1], SEED[2], SEED[3] + P])          # seed words are taken mod p
        gc = glp.Circuit(c2, desc)
        with Dev(c2, arr) as d:
            got = gc.prove_device(d)
        c2.set_salt_seed(SEED)
        with Dev(c2, A) as d:
            canonical = gc.prove_device(d)
        desc.wires = A
        _check_zk_proof(oracle, desc, gc, got)
        _same_proof(got, canonical, "zk, lifted witness and lifted seed against the reduced ones")
        _proof_words_canonical(got, desc)
        gc.free()


@pytest.mark.parametrize("name,members", [("zkdsa 2^3", (0, 1, 2)), ("keccak shape 2^6", (0, 1, 2)), ("ecdsa shape 2^7", (0, 1, 2)),
                                          ("arith 2^13", (0,)), ("arith 2^13", (1,)), ("arith 2^13", (2,))])
def test_prove_batch_on_device(ctx, oracle, name, members):
    """K = 3 twin witnesses in one device array; `members`: the ones whose proof this case holds against the oracle prover (the 2^13
    circuit one per case: an oracle proof of it takes two seconds)"""
    desc = CIRCUITS[name]()
    K = 3
    arr, A = nc.twin(540, (K,) + desc.wires.shape)
    oc, gc = oracle.OracleCircuit(desc), glp.Circuit(ctx, desc)
    pis = np.stack([np.asarray(desc.public_inputs, U)] * K) if len(desc.public_inputs) else None
    with Dev(ctx, arr) as d:
        got = gc.prove_batch_device(d, K, pis)
    for k in members:
        rc, ref = oc.prove(wires=A[k])
        _same_proof(got[k], ref, "%s, member %d" % (name, k))
        _proof_words_canonical(got[k], desc)
    gc.free()


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_session_on_device(ctx, oracle, name):
    """glp_session_begin on device wires, stepped by the oracle's transcript to the whole proof"""
    from test_gpu_prove import _stepped_proof
    desc = CIRCUITS[name]()
    arr, A = nc.twin(550, desc.wires.shape)
    oc, gc = oracle.OracleCircuit(desc), glp.Circuit(ctx, desc)
    rc, ref = oc.prove(wires=A)
    with Dev(ctx, arr) as d:
        real = glp.Session
        try:
            glp.Session = lambda circuit: real(circuit, dev_wires_ptr=d)            # _stepped_proof opens glp.Session(gc): here on the device wires
            got = _stepped_proof(gc, oracle, desc)
        finally:
            glp.Session = real
    _same_proof(got, ref, name)
    gc.free()


# ------------------------------------------------------------------------------------------ the permutation seam, witness fill
def _satisfying_twin(desc, seed):
    """(array, A) for the wires of a perm_restate description: A still satisfies the copy constraints (one value per cycle), the
    largest cycles hold words of SMALL until at least half of the routed cells do, and half of all small cells are lifted by p"""
    rng = np.random.default_rng(seed)
    nr = desc.num_routed_wires
    A = np.ascontiguousarray(desc.wires, U).copy()
    vals, counts = np.unique(A[:nr], return_counts=True)
    covered = 0
    for k in np.argsort(-counts, kind="stable"):
        if 2 * covered >= A[:nr].size:
            break
        A[A == vals[k]] = U(nc.SMALL[int(rng.integers(0, len(nc.SMALL)))])
        covered += int(counts[k])
    adv_arr, adv_A = nc.twin(seed + 1, A[nr:].shape)
    A[nr:] = adv_A
    low = np.flatnonzero(A[:nr].reshape(-1) < U((1 << 32) - 1))
    arr = A.copy()
    arr[:nr].reshape(-1)[rng.permutation(low)[:(low.size + 1) // 2]] += U(P)
    arr[nr:] = adv_arr
    nc.check_twin(arr, A)
    return arr, A


def test_perm_zs_commit_on_device(ctx, oracle):
    """device wires and sigmas at the 2^4 shape of test_gpu_perm_seam.py: the commitment of the restated Z and partial products of the
    reduced arrays, built by the CPU oracle"""
    lg, nw, nr, chunk, nch, rb = 4, 20, 13, 5, 3, 3
    desc = pr.synthetic(lg, nw, nr, chunk, nch, seed=1000 * lg + 10 * nr + chunk)
    chal = nc.base(77, (2, nch))
    w_arr, w_A = _satisfying_twin(desc, 600)
    s_A = np.ascontiguousarray(desc.sigmas, U)
    s_arr = s_A.copy()
    s_arr[s_A < U((1 << 32) - 1)] += U(P)               # the few sigmas that fit: 1 = the image (column of k = 1, row 0) and the small powers of two
    assert (nc.reduced(s_arr) == s_A).all() and (s_arr >= U(P)).any()
    desc.wires = w_A
    zp = cq.zs_partial_products(desc, w_A, chal[0], chal[1])
    ref = oracle.batch_from_values(zp, rb, 4)
    with Dev(ctx, w_arr) as dw, Dev(ctx, s_arr) as ds:
        b = ctx.perm_zs_commit(desc, None, None, chal[0], chal[1], rb, 4, wires_dev_ptr=dw, sigmas_dev_ptr=ds)
        _check_batch(oracle, b, ref, lg, rb, full=True)
        b.free()


def test_perm_quotient_gate_sums(ctx):
    """host gate sums with a word >= p are refused by name; device gate sums enter through acc_fma, which takes any u64: the
    quotient values equal the restatement on the reduced sums"""
    lg, nw, nr, chunk, nch, rb = 4, 20, 13, 5, 3, 3
    desc = pr.synthetic(lg, nw, nr, chunk, nch, seed=1000 * lg + 10 * nr + chunk)
    chal = nc.base(78, (3, nch))
    M = 1 << (lg + rb)
    zp = cq.zs_partial_products(desc, desc.wires, chal[0], chal[1])
    sb_ = ctx.batch_from_values(np.concatenate([np.asarray(desc.wires[:2], U), desc.sigmas]), rb, 4)
    wb, zb = ctx.batch_from_values(desc.wires, rb, 4), ctx.batch_from_values(zp, rb, 4)
    arr, A = nc.twin(610, (nch, M))
    rows = lambda b, c0=0, k=None: b.lde_values(c0, b.ncols - c0 if k is None else k, rb)
    want = pr.perm_quotient(desc, rows(sb_, 2), rows(wb), rows(zb), rb, chal[0], chal[1], chal[2], gate_sums=A)
    with Dev(ctx, arr) as d:
        got = ctx.perm_quotient_values(desc, sb_, 2, wb, zb, rb, chal[0], chal[1], chal[2], gate_sums_dev_ptr=d)
    assert (got == want).all() and (got < U(P)).all()
    bad, _ = nc.single(611, (nch, M), nc.NC[1], M + 5)
    with pytest.raises(glp.GlpError) as e:
        ctx.perm_quotient_values(desc, sb_, 2, wb, zb, rb, chal[0], chal[1], chal[2], gate_sums=bad)
    msg = str(e.value)
    assert e.value.code == -1 and "gate_sums" in msg and "column 1, index 5" in msg and "canonical" in msg
    assert (ctx.perm_quotient_values(desc, sb_, 2, wb, zb, rb, chal[0], chal[1], chal[2], gate_sums=A) == want).all()
    for b in (sb_, wb, zb):
        b.free()


EDGE = {ec.name: ec for ec in we.circuits()}


@pytest.mark.parametrize("name", sorted(EDGE))
def test_witness_fill(ctx, name):
    """a twin of the routed columns of each edge-row family: the generator inputs are reduced as they are loaded, the written cells are
    those for the reduced witness, every other cell stays as it is (lifted words included)"""
    ec = EDGE[name]
    desc = ec.desc
    gc = glp.Circuit(ctx, desc)
    nr = desc.num_routed_wires
    w = np.ascontiguousarray(we.scramble_outputs(ec, 41), U)       # every cell a generator writes starts wrong
    written = we.role_mask(desc)
    # the cells no generator writes (inputs and untouched ones): a generator that declines an out-of-domain row leaves its cells as they are
    low = np.flatnonzero(((w < U((1 << 32) - 1)) & ~written)[:nr].reshape(-1))
    lift = np.random.default_rng(7).permutation(low)[:(low.size + 1) // 2]
    arr = w.copy()
    arr[:nr].reshape(-1)[lift] += U(P)
    assert (nc.reduced(arr) == w).all() and (arr >= U(P)).any(), "no routed word of this family can be lifted"
    for only_advice in (False, True):
        want = wf.fill(desc, w, only_advice)
        with Dev(ctx, arr, check_unchanged=False) as d:
            gc.witness_fill(d, only_advice=only_advice)
            got = np.empty_like(arr)
            ctx.dev_download(d, got)
        changed = got != arr
        assert not (changed & ~written).any(), "a cell outside the written roles changed"
        if only_advice:
            assert not changed[:nr].any()
        bad = we.first_mismatch(np.where(written, got, 0), np.where(written, want, 0))
        assert bad is None, "only_advice %d: (column %d, row %d) = 0x%x, restated 0x%x" % ((only_advice,) + bad)
        assert (got[written] < U(P)).all(), "a written cell is >= p"
    gc.free()


# ------------------------------------------------------------------------------------------ seeds
def test_seed_words_are_taken_mod_p(ctx, oracle):
    """a seed word + p gives the batch of the reduced seed at every entry that takes a seed; the salts are the restated PRF's"""
    lg, ncols, rb, ch = 4, 3, 2, 2
    seed = (3, (1 << 32) - 2, 0, 9)
    lifted = tuple(s + P for s in seed)
    vals = nc.base(700, (2, ncols, 1 << lg))
    ref = oracle.batch_from_values(vals[0], rb, ch)
    leaves, cap = _salted(oracle, ref, seed, 0, ch)
    b = ctx.batch_from_values_salted(vals[0], lifted, rb, ch)
    assert (b.cap() == cap).all() and (b.leaf(5) == leaves[5]).all()
    b.free()
    for fn, arg in ((ctx.batch_many_from_values, vals), (ctx.batch_many_from_coeffs, vals)):
        a, c = fn(arg, rb, ch, seed=seed), fn(arg, rb, ch, seed=lifted)
        assert (a.caps() == c.caps()).all()
        a.free(); c.free()
    m = ctx.batch_many_from_values(vals, rb, ch, seed=lifted)
    assert (m.caps()[0] == cap).all()
    m.free()
    cv = nc.base(701, (ncols, 1 << (lg + 1)))
    a, c = ctx.batch_from_coset_values(cv, 1, rb, ch, seed=seed), ctx.batch_from_coset_values(cv, 1, rb, ch, seed=lifted)
    assert (a.cap() == c.cap()).all() and (a.leaf(3) == c.leaf(3)).all()
    a.free(); c.free()
    desc = pr.synthetic(4, 20, 13, 5, 3, seed=4135)
    chal = nc.base(702, (2, 3))
    a = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, chal[0], chal[1], rb, ch, seed=seed)
    c = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, chal[0], chal[1], rb, ch, seed=lifted)
    assert (a.caps() == c.caps()).all() and (a.leaf(3) == c.leaf(3)).all()
    a.free(); c.free()
    # glp_ctx_set_salt_seed: test_prove_device_zero_knowledge proves under a lifted seed


# ------------------------------------------------------------------------------------------ refusals of host arrays
def _refused(call, param, where):
    with pytest.raises(glp.GlpError) as e:
        call()
    msg = str(e.value)
    assert e.value.code == -1, msg
    assert param in msg and where in msg and "canonical" in msg, msg


def _where(shape, pos, proofs):
    """the position a refusal names for flat position `pos` of an array of `shape`"""
    idx = np.unravel_index(pos, shape)
    names = {1: ("index",), 2: ("proof", "index") if proofs else ("column", "index"), 3: ("proof", "column", "index")}[len(shape)]
    return ", ".join("%s %d" % (n, i) for n, i in zip(names, idx))


def _sweep(shape, call, param, proofs=False, label=None):
    """every word of NC at the first, the last and a seeded middle position of a canonical array of `shape`"""
    size = int(np.prod(shape))
    for k, word in enumerate(nc.NC):
        for pos in nc.single_positions(k, size):
            arr, _ = nc.single(800 + k, shape, word, pos)
            where = label(pos) if label else _where(shape, pos, proofs)
            _refused(lambda: call(arr), param, where + " = 0x%016x" % word)


def test_in_place_primitives_refuse(ctx, oracle):
    """glp_fft, glp_ifft, glp_coset_ifft, glp_poseidon_permute, glp_lde: refused, the caller's array left as it was, the next call right"""
    L = binding.load_library()
    for fn, shape, extra in (("glp_fft", (3, 16), ()), ("glp_ifft", (3, 2), ()), ("glp_ifft", (2, 1 << 13), ()), ("glp_coset_ifft", (3, 16), (7,))):
        def raw(arr, fn=fn, shape=shape, extra=extra):
            keep = arr.copy()
            rc = getattr(L, fn)(ctx._h, binding._p(arr), shape[0], shape[1].bit_length() - 1, *extra)
            assert (arr == keep).all(), "%s wrote to a refused array" % fn
            binding._chk(rc)
        _sweep(shape, raw, "%s: cols" % fn)

    def permute(arr):
        keep = arr.copy()
        rc = L.glp_poseidon_permute(ctx._h, binding._p(arr), arr.shape[0])
        assert (arr == keep).all()
        binding._chk(rc)
    _sweep((5, 12), permute, "glp_poseidon_permute: states", label=lambda pos: "state %d, index %d" % divmod(pos, 12))
    a = nc.base(1, (3, 16))
    assert all((ctx.ifft(a)[k] == oracle.ifft(a[k])).all() and (ctx.fft(a)[k] == oracle.fft(a[k])).all() for k in range(3)), "the context after a refusal"
    assert (ctx.coset_ifft(a)[2] == oracle.coset_ifft(a[2], 7)).all()
    st = nc.base(2, (2, 12))
    assert (ctx.poseidon_permute(st)[1] == oracle.poseidon_permute(st[1])).all()
    # glp_ifft of [0, 2^64 - 1]: the case that returned a wrong second coefficient before the scan
    _refused(lambda: ctx.ifft(np.array([[0, 2 ** 64 - 1]], U)), "glp_ifft: cols", "column 0, index 1")
    _sweep((3, 16), lambda arr: ctx.lde(arr, 2, 7), "glp_lde: coeffs")
    for word in nc.NC:                                  # the coset shift of glp_lde is a field element too
        with pytest.raises(glp.GlpError) as e:
            ctx.lde(a, 2, word)
        assert e.value.code == -1 and "shift" in str(e.value) and "canonical" in str(e.value)
    assert (ctx.lde(a[:1], 2, 7)[0] == oracle.lde(a[0], 2, 7)).all()


def test_commitments_refuse_host_words(ctx, oracle):
    """every glp_batch_* entry that reads host memory: refused by name, and no handle comes back"""
    L = binding.load_library()

    def no_handle(fn, *args):
        def call(arr):
            h = C.c_void_p(0xDEAD)
            rc = getattr(L, fn)(ctx._h, binding._p(arr), *args, C.byref(h))
            assert rc != 0 and not h.value, "%s: a refused call returned a handle" % fn
            binding._chk(rc)
        return call
    sd = np.array([1, 2, 3, 4], U)
    for fn, args, param in (("glp_batch_from_values", (3, 4, 2, 2), "values"), ("glp_batch_from_values_h", (3, 4, 2, 2, 1), "values"),
                            ("glp_batch_from_values_salted", (3, 4, 2, 2, 0, binding._p(sd)), "values"),
                            ("glp_batch_from_coeffs", (3, 4, 2, 2), "coeffs"), ("glp_batch_from_coeffs_h", (3, 4, 2, 2, 0), "coeffs")):
        _sweep((3, 16), no_handle(fn, *args), "%s: %s" % (fn, param))
    for fn, param in (("glp_batch_many_from_values", "values"), ("glp_batch_many_from_coeffs", "coeffs")):
        _sweep((2, 3, 16), no_handle(fn, 0, 2, 3, 4, 2, 2, 0, None), "%s: %s" % (fn, param), proofs=True)
    _sweep((2, 3, 64), no_handle("glp_batch_from_coset_values", 0, 2, 3, 4, 2, 2, 2, 0, None), "glp_batch_from_coset_values: values", proofs=True)
    a = nc.base(1, (3, 16))
    for make, ref in ((ctx.batch_from_values, oracle.batch_from_values), (ctx.batch_from_coeffs, oracle.batch_from_coeffs)):
        b, want = make(a, 2, 2), ref(a, 2, 2)
        assert (b.cap() == want.cap).all() and (b.coeffs() == want.coeffs).all()
        b.free()


def test_large_host_array_is_scanned_in_pieces(ctx, oracle):
    """3 x 2^20 words: the scan runs in pieces on the context's host threads; the first bad word in array order is the one named"""
    L = binding.load_library()
    shape = (3, 1 << 20)
    arr = nc.base(5, shape)
    h = C.c_void_p()
    for k, pos in enumerate(nc.single_positions(5, arr.size)):
        bad = arr.copy()
        bad.reshape(-1)[pos] = U(nc.NC[k])
        bad.reshape(-1)[-1] = U(nc.NC[4])               # a later one as well: the earlier is reported
        rc = L.glp_batch_from_values(ctx._h, binding._p(bad), 3, 20, 0, 4, C.byref(h))
        msg = L.glp_last_error().decode()
        word = nc.NC[k] if pos < arr.size - 1 else nc.NC[4]
        assert rc == -1 and not h.value and "values: %s = 0x%016x" % (_where(shape, pos, False), word) in msg and "canonical" in msg, msg


def test_perm_seam_refuses_host_words(ctx, oracle):
    desc = pr.synthetic(4, 20, 13, 5, 3, seed=4135)
    chal = nc.base(3, (2, 3))
    _sweep(desc.wires.shape, lambda arr: ctx.perm_zs_commit(desc, arr, desc.sigmas, chal[0], chal[1], 3, 4), "glp_perm_zs_commit: wires", proofs=False,
           label=lambda pos: "proof 0, column %d, index %d" % divmod(pos, 16))
    _sweep(desc.sigmas.shape, lambda arr: ctx.perm_zs_commit(desc, desc.wires, arr, chal[0], chal[1], 3, 4), "glp_perm_zs_commit: sigmas")
    b = ctx.perm_zs_commit(desc, desc.wires, desc.sigmas, chal[0], chal[1], 3, 4)      # the next canonical call
    _check_batch(oracle, b, oracle.batch_from_values(cq.zs_partial_products(desc, desc.wires, chal[0], chal[1]), 3, 4), 4, 3, full=True)
    b.free()


def test_prover_refuses_host_words(ctx, oracle):
    """glp_prove, glp_prove_batch, glp_session_begin, glp_witness_stage, and the public inputs of glp_prove_device and glp_prove_staged"""
    cd = synth.zkdsa_circuit(3)
    oc, gc = oracle.OracleCircuit(cd), glp.Circuit(ctx, cd)
    rc, ref = oc.prove()
    wshape, npi = cd.wires.shape, len(cd.public_inputs)
    assert npi > 0
    pis = np.asarray(cd.public_inputs, U)
    _sweep(wshape, lambda arr: gc.prove(wires=arr), "glp_prove: wires")
    _sweep((npi,), lambda arr: gc.prove(public_inputs=arr), "glp_prove: public_inputs")
    _sweep((2,) + wshape, lambda arr: gc.prove_batch(arr, np.stack([pis, pis])), "glp_prove_batch: wires", proofs=True)
    _sweep((2, npi), lambda arr: gc.prove_batch(np.stack([cd.wires, cd.wires]), arr), "glp_prove_batch: public_inputs", proofs=True)
    _sweep(wshape, lambda arr: glp.Session(gc, wires=arr), "glp_session_begin: wires")
    _sweep((npi,), lambda arr: glp.Session(gc, public_inputs=arr), "glp_session_begin: public_inputs")
    _sweep(wshape, lambda arr: gc.stage_witness(arr), "glp_witness_stage: host_wires")
    nr = cd.num_routed_wires
    _sweep((nr, wshape[1]), lambda arr: gc.stage_witness(np.concatenate([arr, cd.wires[nr:]]), routed_only=True), "glp_witness_stage: host_wires")
    lifted_advice = np.ascontiguousarray(cd.wires, U).copy()
    lifted_advice[nr:] = U(2 ** 64 - 1)                                           # ROUTED_ONLY never reads the advice columns
    st = gc.stage_witness(lifted_advice, routed_only=True)
    with Dev(ctx, cd.wires) as d:
        _sweep((npi,), lambda arr: gc.prove_device(d, public_inputs=arr), "glp_prove_device: public_inputs")
        _sweep((npi,), lambda arr: gc.prove_staged(st, public_inputs=arr), "glp_prove_staged: public_inputs")
        assert (gc.prove_device(d) == ref).all()
    w0 = np.ascontiguousarray(cd.wires, U).copy()
    w0[nr:] = 0
    rc, want = oc.prove(wires=oc.witness_fill(w0, only_advice=True))
    assert (gc.prove_staged(st) == want).all()
    st.free()
    assert (gc.prove() == ref).all() and (gc.prove_batch(np.stack([cd.wires, cd.wires]), np.stack([pis, pis]))[1] == ref).all()
    gc.free()


def test_pow_witness_is_refused(ctx, oracle):
    """the proof-of-work witness is a field element that lands in the proof: glp_session_queries, glp_fri_queries, glp_fri_queries_many"""
    from test_gpu_prove import _stepped_proof
    desc = synth.zkdsa_circuit(3)
    oc = oracle.OracleCircuit(desc)                     # derives the circuit digest the transcript starts from
    gc = glp.Circuit(ctx, desc)
    real = glp.Session
    seen = []

    class Probe(real):
        def queries(self, w, idx):
            for word in nc.NC:
                _refused(lambda: real.queries(self, word, idx), "glp_session_queries: pow_witness", "0x%016x" % word)
            seen.append(1)
            return real.queries(self, w, idx)
    try:
        glp.Session = Probe                             # _stepped_proof opens glp.Session(gc)
        got = _stepped_proof(gc, oracle, desc)
    finally:
        glp.Session = real
    rc, ref = oc.prove()
    assert seen and (got == ref).all()
    gc.free()
    vals = nc.base(900, (3, 16))
    b = ctx.batch_from_values(vals, 3, 2)
    for many in (False, True):
        if many:
            f = glp.FriOpeningsMany(ctx, [b], [((5, 6), [(0, 0, 3)])], [[[5, 6]]], [2], 4, 3)
        else:
            f = glp.FriOpenings(ctx, [b], [((5, 6), [(0, 0, 3)])], [2], 4, 3)
        f.open()
        f.combine([3, 4] if not many else [[3, 4]])
        f.commit()
        f.fold([7, 8] if not many else [[7, 8]])
        f.final_poly()
        for word in nc.NC:
            _refused(lambda: f.queries(word if not many else [word], [1, 2, 3] if not many else [[1, 2, 3]]), "pow_witness", "0x%016x" % word)
        f.queries(5 if not many else [5], [1, 2, 3] if not many else [[1, 2, 3]])
        assert 5 in f.proof().reshape(-1)
        f.end()
    b.free()


def test_session_challenges_are_refused(ctx):
    """the stepped session's challenges after the betas and gammas (test_gpu_prove.py pins those): alphas, zeta, the FRI alpha and beta"""
    desc = synth.arith_circuit(6, synth.Config.standard_recursion_config(), seed=77)
    assert len(desc.reduction_arity_bits) > 0
    gc = glp.Circuit(ctx, desc)
    nch = desc.num_challenges
    s = glp.Session(gc)
    s.partial_products([5] * nch, [7] * nch)
    for word in nc.NC:
        _refused(lambda: s.quotient([9] * (nch - 1) + [word]), "challenge %d" % (nch - 1), "")
    s.quotient([9] * nch)
    for word in nc.NC:
        _refused(lambda: s.open([3, word]), "zeta", "")
    s.open([3, 4])
    for word in nc.NC:
        _refused(lambda: s.fri_combine([word, 1]), "alpha", "")
    s.fri_combine([11, 1])
    s.fri_commit()
    for word in nc.NC:
        _refused(lambda: s.fri_fold([2, word]), "beta", "")
    s.end()
    gc.free()
