"""Zero-knowledge proving on the GPU: salted commitments (glp_batch_from_values_salted) against the oracle's Merkle tree over its own
LDE leaves with the restated salts appended, and zk proofs (GLP_CIRCUIT_ZERO_KNOWLEDGE) through every proving path and both
verifiers, checked against the restated salt rule, the oracle's Merkle verifier and LDE, and the vanishing identity at zeta."""
import ctypes as C
import os

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
from plonky2_lib_amd import gadgets as G
import plonky2_lib_amd.synth as synth
import zeta_identity
import zk_restate as zr

pytestmark = pytest.mark.gpu

SEED = [11, 22, 33, 44]
FORMS = {"coop": (1 << 30, 1 << 30), "quad": (0, 1 << 30), "plain": (0, 0)}


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    c.set_salt_seed(SEED)
    yield c
    c.close()


def _ctx_with_form(form):
    keys = ("GLP_MERKLE_COOP_MAX", "GLP_MERKLE_QUAD_MAX")
    old = {k: os.environ.get(k) for k in keys}
    os.environ.update(dict(zip(keys, (str(v) for v in FORMS[form]))))
    try:
        return glp.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("form", sorted(FORMS))
def test_salted_batch_tree(oracle, form):
    c2 = _ctx_with_form(form)
    try:
        rng = np.random.default_rng(3)
        for hasher in (0, 1):
            for ncols in (4, 5, 12):
                lg, rb, ch = 6, 2, 2
                vals = oracle.rand_field(rng, (ncols, 1 << lg))
                ref = oracle.batch_from_values(vals, rb, ch, hasher)
                N = 1 << (lg + rb)
                leaves = np.concatenate([ref.leaves, zr.salt_columns(oracle, SEED, zr.TAG_BATCH, N)], axis=1)
                with oracle._Hasher(hasher):
                    dig, cap = oracle.merkle_build(leaves, ch)
                b = c2.batch_from_values_salted(vals, SEED, rb, ch, hasher)
                assert b.leaf_len == ncols + 4 and b.ncols == ncols
                assert (b.cap() == cap).all(), (form, hasher, ncols)
                assert (b.digests() == dig).all()
                assert (b.coeffs() == ref.coeffs).all()
                for j in (0, 1, N // 2 + 3, N - 1):
                    assert (b.leaf(j) == leaves[j]).all()
                    assert (b.prove(j) == oracle.merkle_prove(dig, N, ch, j)).all()
                    assert oracle.merkle_verify(b.leaf(j), j, cap, b.prove(j), hasher)
                b.free()
    finally:
        c2.close()


def _zkdsa(q=28, hasher=0):
    c = synth.zkdsa_circuit(config=synth.Config.standard_recursion_zk_config(num_query_rounds=q))
    c.hasher = hasher
    return c


def _smt():
    t = G.SparseMerkleTree()
    for k, v in ((1, 2), (12, 1), (5, 51)):
        t.insert(G.hash_out_from_u128(k), G.hash_out_from_u128(v))
    return G.smt_inclusion_circuit(t, G.hash_out_from_u128(5), config=synth.Config.standard_recursion_zk_config())


def _ext():
    """64 rows of extension-field gates followed by the blinding rows: 2^10 rows"""
    return synth.ext_gates_circuit(6, config=synth.Config.standard_recursion_zk_config(num_query_rounds=2))


def _plain_twin(desc):
    """the same blinded circuit as a non-zk description (shares every array)"""
    class D:
        pass
    d = D()
    d.__dict__.update(desc.__dict__)
    d.zero_knowledge = False
    return d


def _check_zk_proof(oracle, desc, gc, proof, seed=SEED, k=0):
    """salts = the restated PRF, salted leaves verify against the proof's caps, stripped wires / constants leaves = the oracle's LDE
    values at the query index, stripped proof passes the identity at zeta"""
    hasher = int(getattr(desc, "hasher", 0))
    assert proof.size == zr.proof_words(desc, True) == gc.proof_words
    cap = 4 << int(desc.cap_height)
    caps = [gc.constants_sigmas_cap()] + [proof[i * cap:(i + 1) * cap].reshape(-1, 4) for i in range(3)]
    N = 1 << (desc.degree_bits + desc.rate_bits)
    with oracle._Hasher(hasher):
        wb = oracle.batch_from_values(desc.wires, desc.rate_bits, desc.cap_height)
        csb = oracle.batch_from_values(np.concatenate([desc.constants, desc.sigmas]), desc.rate_bits, desc.cap_height)
    nw = int(desc.num_wires)
    for rnd in zr.query_leaves(desc, proof, True):
        wl = rnd[1][0]
        hits = np.nonzero((wb.leaves[:, 0] == wl[0]) & (wb.leaves[:, 1] == wl[1]))[0]
        assert hits.size == 1
        x = int(hits[0])
        assert (wl[:nw] == wb.leaves[x]).all()
        assert (rnd[0][0] == csb.leaves[x]).all()
        for o in range(4):
            leaf, path = rnd[o]
            assert oracle.merkle_verify(leaf, x, caps[o], path, hasher), o
            if o > 0:
                assert (leaf[-4:] == zr.salt(oracle, seed, o - 1, x, k)).all(), o
    if all(int(g["type"]) in IDENTITY_GATES for g in desc.gates):      # the gate types tests/zeta_identity.py restates
        assert zeta_identity.check(desc, zr.strip_salts(desc, proof), gc.digest(), hasher)


IDENTITY_GATES = {synth.GATE_NOOP, synth.GATE_CONSTANT, synth.GATE_PUBLIC_INPUT, synth.GATE_ARITHMETIC} | set(synth.EXT_GATES)
CASES = {"zkdsa": lambda: _zkdsa(), "smt": _smt, "ext": _ext, "q2": lambda: _zkdsa(2), "q2_keccak": lambda: _zkdsa(2, 1)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_zk_proof(ctx, oracle, case):
    desc = CASES[case]()
    gc = glp.Circuit(ctx, desc)
    if desc.circuit_digest is None:
        desc.circuit_digest = gc.digest()
    assert gc.zero_knowledge and binding.load_library().glp_circuit_zero_knowledge(gc._h) == 1
    proof = gc.prove()
    _check_zk_proof(oracle, desc, gc, proof)
    assert gc.verify(proof)
    assert list(gc.verify_batch(np.stack([proof, proof]))) == [True, True]
    # bytes round trip
    data = gc.proof_to_bytes(proof)
    assert len(data) == binding.load_library().glp_proof_bytes_len(gc._h)
    assert (gc.proof_from_bytes(data) == proof).all()
    # the same blinded circuit without zk: 12 * num_query_rounds fewer words, and a zk proof is refused by length
    pc = glp.Circuit(ctx, _plain_twin(desc))
    assert pc.proof_words + 12 * desc.num_query_rounds == gc.proof_words
    rc = binding.load_library().glp_verify_n(pc._h, binding._p(proof), proof.size)
    assert rc == -1
    gc.free(); pc.free()


def test_zk_paths_agree(ctx, oracle):
    """glp_prove, device, staged and stepped session agree word for word; ROUTED_ONLY staging is refused"""
    desc = _zkdsa(2)
    gc = glp.Circuit(ctx, desc)
    ref = gc.prove()
    w = np.ascontiguousarray(desc.wires)
    dp = ctx.dev_alloc(w.nbytes)
    try:
        ctx.dev_upload(dp, w)
        assert (gc.prove_device(dp) == ref).all()
    finally:
        ctx.dev_free(dp)
    st = gc.stage_witness(w)
    assert (gc.prove_staged(st) == ref).all()
    st.free()
    with pytest.raises(glp.GlpError):
        gc.stage_witness(w, routed_only=True)
    from test_gpu_prove import _stepped_proof
    desc.circuit_digest = gc.digest()
    assert (_stepped_proof(gc, oracle, desc) == ref).all()
    gc.free()


def test_zk_and_plain_sessions_open_alike(ctx):
    """driven by one challenge sequence, a zk and a non-zk session of the same witness give identical openings, FRI layer caps and
    final polynomial: salts never enter the opened polynomials"""
    desc = _zkdsa(2)
    gz, gp = glp.Circuit(ctx, desc), glp.Circuit(ctx, _plain_twin(desc))
    rng = np.random.default_rng(9)
    chal = [int(x) for x in rng.integers(1, 1 << 62, 32, dtype=np.int64)]
    outs = []
    for gc in (gz, gp):
        s = glp.Session(gc)
        s.partial_products(chal[0:2], chal[2:4])
        s.quotient(chal[4:6])
        op = s.open(chal[6:8])
        s.fri_combine(chal[8:10])
        caps = []
        for r in range(len(desc.reduction_arity_bits)):
            caps.append(s.fri_commit())
            s.fri_fold(chal[10 + 2 * r:12 + 2 * r])
        outs.append((s.wires_cap, op, caps, s.fri_final_poly()))
        s.end()
    (wz, oz, cz, fz), (wp, opl, cp, fp) = outs
    assert not (wz == wp).all()
    assert (oz == opl).all() and all((a == b).all() for a, b in zip(cz, cp)) and (fz == fp).all()
    gz.free(); gp.free()


@pytest.mark.parametrize("host_transcript", [False, True])
def test_zk_prove_batch(ctx, oracle, host_transcript):
    """member k of glp_prove_batch = glp_prove with seed3 + k (K = 9 crosses the leaf-hash threshold); glp_verify_batch agrees"""
    desc = _zkdsa(2)
    gc = glp.Circuit(ctx, desc)
    K = 9
    if host_transcript:
        os.environ["GLP_BATCH_HOST_TRANSCRIPT"] = "1"
    try:
        proofs = gc.prove_batch(np.stack([desc.wires] * K), np.stack([desc.public_inputs] * K))
    finally:
        os.environ.pop("GLP_BATCH_HOST_TRANSCRIPT", None)
    desc.circuit_digest = gc.digest()
    for k in (0, 1, K - 1):
        ctx.set_salt_seed(SEED[:3] + [SEED[3] + k])
        try:
            assert (proofs[k] == gc.prove()).all(), k
        finally:
            ctx.set_salt_seed(SEED)
    _check_zk_proof(oracle, desc, gc, proofs[K - 1], k=K - 1)
    assert all(gc.verify_batch(proofs))
    gc.free()


def test_zk_verdicts(ctx):
    """glp_verify and glp_verify_batch reject a flipped salt, a flipped stripped-leaf word and a non-canonical salt, for one reason"""
    desc = _zkdsa(2)
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    q0, stride, oracles, _ = zr.layout(desc, True)
    lo, ll, _ = oracles[1]
    salt_at, leaf_at = q0 + lo + ll - 1, q0 + lo + 3
    bad = []
    for at, val in ((salt_at, int(proof[salt_at]) ^ 1), (leaf_at, int(proof[leaf_at]) ^ 1), (salt_at, zr.P + 5)):
        p = proof.copy()
        p[at] = np.uint64(val)
        bad.append(p)
    L = binding.load_library()
    ok, reasons = gc.verify_batch(np.stack([proof] + bad), reasons=True)
    assert list(ok) == [True, False, False, False]
    for p, why in zip(bad, reasons[1:]):
        assert not gc.verify(p)
        assert L.glp_verify(gc._h, binding._p(p)) == -5
        assert L.glp_last_error().decode() == why
    gc.free()


def test_zk_os_seed(oracle):
    """with the OS seed two proofs of one witness differ in all three caps and both verify"""
    c2 = glp.Context(0)
    try:
        desc = _zkdsa(2)
        gc = glp.Circuit(c2, desc)
        a, b = gc.prove(), gc.prove()
        cap = 4 << desc.cap_height
        for i in range(3):
            assert not (a[i * cap:(i + 1) * cap] == b[i * cap:(i + 1) * cap]).all(), i
        assert gc.verify(a) and gc.verify(b)
        assert all(gc.verify_batch(np.stack([a, b])))
        gc.free()
    finally:
        c2.close()


def test_create_ex_without_flag_is_create(ctx):
    desc = synth.zkdsa_circuit()
    gc = glp.Circuit(ctx, desc)
    L = binding.load_library()
    d, keep = binding._desc_to_c(desc)
    h = C.c_void_p()
    assert L.glp_circuit_create_ex(ctx._h, C.byref(d), 0, C.byref(h)) == 0
    assert L.glp_circuit_zero_knowledge(h) == 0 and L.glp_proof_words(h) == gc.proof_words
    out = np.zeros(gc.proof_words, np.uint64)
    pi = np.ascontiguousarray(desc.public_inputs, np.uint64)
    assert L.glp_prove(ctx._h, h, binding._p(np.ascontiguousarray(desc.wires)), binding._p(pi), binding._p(out)) == 0
    assert (out == gc.prove()).all()
    L.glp_circuit_free(h)
    assert L.glp_circuit_create_ex(ctx._h, C.byref(d), 2, C.byref(h)) == -1
    del keep
    gc.free()


def test_zk_ecdsa_one_signature(ctx):
    from plonky2_lib_amd import gadgets_ecdsa as E
    (msg, sig, pk), = E.random_signatures(1, seed=3)
    desc = E.ecdsa_circuit([(msg, sig, pk)], config=synth.Config.standard_ecc_config(zero_knowledge=True))
    assert desc.degree_bits == 17
    gc = glp.Circuit(ctx, desc)
    proof = gc.prove()
    assert gc.verify(proof) and proof.size == zr.proof_words(desc, True)
    assert list(gc.verify_batch(proof[None])) == [True]
    gc.free()
