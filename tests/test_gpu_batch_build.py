"""glp::batch_build is one pipeline for every K >= 1 (csrc/api.hip): every public commit goes through it.
1. every input kind (values, natural coefficients, coset values = the BATCH_COEFFS_BITREV kind) at K = 1 and K = 3, salted and not,
   both hashers, against the oracle's tree member by member; host and device input forms word for word.
2. the stage records a K = 1 call leaves (bench.py's stage_table assigns records to oracles by counting them), and a K = 3 call
   leaving the same names.
3. the shape refusals of the entry points that allocate or upload before batch_build: code by code, none reaching a stage record.
Shapes: log_n = 3, 3 and 6 columns (an unsalted leaf of at most four words is copied, not hashed), rate_bits 0 and 3, cap_height 0
and log_n + rate_bits (the cap is the leaves: empty paths)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
import plonky2_lib_amd.synth as synth
import perm_restate as pr
import zk_restate as zr

pytestmark = pytest.mark.gpu

SEED = [11, 22, 33, 44]
LG = 3
ARG, UNSUPPORTED = -1, -3              # GLP_ERR_ARG, GLP_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _on_device(ctx, arr):
    a = np.ascontiguousarray(arr, np.uint64)
    d = ctx.dev_alloc(a.nbytes)
    ctx.dev_upload(d, a)
    return d


# ------------------------------------------------------------------ 1. every input kind through the one body
@functools.lru_cache(maxsize=None)
def _salts(oracle, N, k):
    return zr.salt_columns(oracle, SEED, zr.TAG_BATCH, N, k)


def _oracle_tree(oracle, kind, member, rb, ch, hasher, salted, k):
    """(coeffs, leaves, digests, cap) of member k: the oracle's batch, with the member's salts (seed3 + k) appended when salted"""
    ref = oracle.batch_from_values(member, rb, ch, hasher) if kind == "values" else oracle.batch_from_coeffs(member, rb, ch, hasher)
    if not salted:
        return ref.coeffs, ref.leaves, ref.digests, ref.cap
    leaves = np.concatenate([ref.leaves, _salts(oracle, 1 << (LG + rb), k)], axis=1)
    with oracle._Hasher(hasher):
        dig, cap = oracle.merkle_build(leaves, ch)
    return ref.coeffs, leaves, dig, cap


def _commit(ctx, kind, data, K, rb, ch, hasher, seed, dev_ptr=None):
    """the public call of `kind` on data [K][cols][len] (K = 1: the single-batch entry points where there is one), host or device input"""
    L = glp.load_library()
    if kind.startswith("coset"):
        sub_bits = int(kind[-1])
        v = data if K > 1 else data[0]
        return ctx.batch_from_coset_values(None if dev_ptr else v, sub_bits, rb, ch, hasher, seed, dev_ptr=dev_ptr, shape=v.shape)
    if K == 1 and dev_ptr is None and kind == "values" and seed is not None:
        return ctx.batch_from_values_salted(data[0], seed, rb, ch, hasher)
    if K == 1 and dev_ptr is None and seed is None:
        return ctx.batch_from_values(data[0], rb, ch, hasher) if kind == "values" else ctx.batch_from_coeffs(data[0], rb, ch, hasher)
    if K == 1 and dev_ptr is not None and seed is None and hasher == 0:
        fn = ctx.batch_from_values_device if kind == "values" else ctx.batch_from_coeffs_device
        return fn(dev_ptr, data.shape[1], LG, rb, ch)
    h, sd = C.c_void_p(), None if seed is None else np.array(seed, np.uint64)
    fn = L.glp_batch_many_from_values if kind == "values" else L.glp_batch_many_from_coeffs
    a = np.ascontiguousarray(data)
    binding._chk(fn(ctx._h, C.c_void_p(dev_ptr) if dev_ptr else binding._p(a), 1 if dev_ptr else 0, K, a.shape[1], LG, rb, ch, hasher,
                    None if sd is None else binding._p(sd), C.byref(h)))
    b = glp.Batch(ctx, h, a.shape[1], LG, rb, ch)
    b.hasher = hasher
    return b


def _words(b, K, js):
    """everything the accessors serve, member by member"""
    out = []
    for k in range(K):
        m = b.member(k) if K > 1 else b
        out.append([m.coeffs(), m.digests(), m.cap()] + [m.leaf(j) for j in js] + [m.prove(j) for j in js])
    return out


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kind", ["values", "coeffs", "coset sub_bits 0", "coset sub_bits 1"])
def test_every_input_kind_against_the_oracle(ctx, oracle, kind, K):
    rng = np.random.default_rng(7 * K + len(kind))
    n = 1 << LG
    for ncols in (3, 6):
        if kind.startswith("coset"):
            # num_polys << sub_bits columns: 3 is odd, so sub_bits = 1 takes 2 (one polynomial; still a copied leaf) and 6
            sub_bits = int(kind[-1])
            ncols = max(ncols >> sub_bits, 1) << sub_bits
            coeffs = oracle.rand_field(rng, (K, ncols >> sub_bits, n << sub_bits))
            data = np.stack([np.stack([oracle.coset_fft(p, 7) for p in member]) for member in coeffs])
            members, okind = coeffs.reshape(K, ncols, n), "coeffs"
        else:
            data = members = oracle.rand_field(rng, (K, ncols, n))
            okind = kind
        dev = _on_device(ctx, data)
        try:
            for rb, hasher, seed in itertools.product((0, 3), (0, 1), (None, SEED)):
                if kind == "coset sub_bits 1" and rb == 0:
                    continue                                    # sub_bits <= rate_bits is a rule of the entry point: not a case
                N = n << rb
                js = (0, N // 2 + 1, N - 1)
                for ch in (0, LG + rb):
                    tag = (kind, K, ncols, rb, ch, hasher, seed is not None)
                    b = _commit(ctx, kind, data, K, rb, ch, hasher, seed)
                    assert b.num_proofs == K and b.ncols == ncols and b.leaf_len == ncols + (4 if seed else 0), tag
                    got = _words(b, K, js)
                    for k in range(K):
                        co, leaves, dig, cap = _oracle_tree(oracle, okind, members[k], rb, ch, hasher, seed is not None, k)
                        want = [co, dig, cap] + [leaves[j] for j in js] + [oracle.merkle_prove(dig, N, ch, j) for j in js]
                        for g, w in zip(got[k], want):
                            assert np.asarray(g).shape == np.asarray(w).shape and (np.asarray(g) == np.asarray(w)).all(), tag + (k,)
                    if K > 1:
                        assert (b.caps() == np.stack([g[2] for g in got])).all(), tag
                    b.free()
                    bd = _commit(ctx, kind, data, K, rb, ch, hasher, seed, dev_ptr=dev)
                    for gk, dk in zip(got, _words(bd, K, js)):
                        for g, d in zip(gk, dk):
                            assert (np.asarray(g) == np.asarray(d)).all(), ("device input",) + tag
                    bd.free()
            back = np.empty_like(data)
            ctx.dev_download(dev, back)
            assert (back == data).all(), "the caller's device input was written to"
        finally:
            ctx.dev_free(dev)


# ------------------------------------------------------------------ 2. stage records
TREE = ["merkle_leaves", "merkle_levels"]
# Recorded from a run of the commit before batch_build became one body, at these shapes -- not from the code under test.
STAGES_K1 = {
    "batch_from_values": ["intt", "lde"] + TREE,
    "batch_from_values_device": ["intt", "lde"] + TREE,
    "batch_from_coeffs": ["bitrev_coeffs", "lde"] + TREE,
    "batch_from_values_salted": ["intt", "lde", "salt"] + TREE,
    "batch_from_coset_values": ["copy_coeffs", "lde"] + TREE,
}
# glp_prove of synth.zkdsa_circuit(3): the wires, Z / partial-products and quotient commits, then the FRI stages (no reduction at 2^3 rows)
STAGES_PROVE = (["intt", "lde"] + TREE + ["partial_products", "intt", "lde"] + TREE + ["quotient_eval", "quotient_intt", "copy_coeffs", "lde"] + TREE
                + ["openings", "fri_combine", "fri_pow", "fri_queries"])


def _names(ctx):
    return [s[0] for s in ctx.stages()]


@pytest.fixture()
def prof(ctx):
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.stage_reset()
    yield ctx
    ctx.set_profiling(False)
    ctx.stage_reset()


def test_stage_records_of_a_single_batch(prof, oracle):
    """The literal lists are what the parent commit (three bodies in batch_build) recorded at these shapes; bench.py's stage_table
    counts on them.  A K = 3 call, which recorded only the salt and tree stages before, now leaves the names of its K = 1 form."""
    ctx = prof
    rng = np.random.default_rng(5)
    vals = oracle.rand_field(rng, (6, 1 << LG))
    dev = _on_device(ctx, vals)
    calls = {
        "batch_from_values": lambda: ctx.batch_from_values(vals, 3, 2),
        "batch_from_values_device": lambda: ctx.batch_from_values_device(dev, 6, LG, 3, 2),
        "batch_from_coeffs": lambda: ctx.batch_from_coeffs(vals, 3, 2),
        "batch_from_values_salted": lambda: ctx.batch_from_values_salted(vals, SEED, 3, 2),
        "batch_from_coset_values": lambda: ctx.batch_from_coset_values(vals[:3].reshape(3, 1 << LG), 0, 3, 2),
    }
    try:
        for name, call in calls.items():
            ctx.stage_reset()
            b = call()
            got = _names(ctx)
            print(name, got)
            assert got == STAGES_K1[name], name
            b.free()
        many = np.stack([vals, vals, vals])
        for seed, want in ((None, STAGES_K1["batch_from_values"]), (SEED, STAGES_K1["batch_from_values_salted"])):
            ctx.stage_reset()
            b1 = ctx.batch_many_from_values(many[:1], 3, 2, 0, seed)
            one, bytes1 = _names(ctx), [s[2] for s in ctx.stages()]
            ctx.stage_reset()
            b3 = ctx.batch_many_from_values(many, 3, 2, 0, seed)
            three = _names(ctx)
            print("batch_many_from_values", seed, one, three)
            assert one == want and three == one, (seed, one, three)
            assert [s[2] for s in ctx.stages()] == [3 * x for x in bytes1], "the bytes of a record scale by K"
            b1.free(); b3.free()
    finally:
        ctx.dev_free(dev)


def test_stage_records_of_one_proof(prof):
    """One Circuit.prove of the suite's smallest synthetic circuit: the list is the parent commit's, record for record."""
    ctx = prof
    gc = glp.Circuit(ctx, synth.zkdsa_circuit(3))
    ctx.stage_reset()
    gc.prove()
    got = _names(ctx)
    print("Circuit.prove", got)
    assert got == STAGES_PROVE
    gc.free()


# ------------------------------------------------------------------ 3. refusals
def _code(fn):
    with pytest.raises(glp.GlpError) as e:
        fn()
    return e.value.code, str(e.value)


# (rate_bits 5, cap_height log_n + rate_bits + 1, log_n 25, num_proofs 0, num_proofs 4097, hasher 2): the codes of the parent commit
REFUSALS = {
    "batch_many_from_values": dict(rate_bits=ARG, cap_height=ARG, log_n=UNSUPPORTED, none=ARG, many=ARG, hasher=UNSUPPORTED),
    "batch_from_coset_values": dict(rate_bits=ARG, cap_height=ARG, log_n=UNSUPPORTED, none=ARG, many=ARG, hasher=UNSUPPORTED),
    "perm_zs_commit": dict(rate_bits=ARG, cap_height=ARG, log_n=ARG, none=ARG, many=ARG, hasher=ARG),
}


@pytest.mark.parametrize("entry", list(REFUSALS))
def test_shape_refusals_keep_their_codes_and_reach_no_launch(prof, oracle, entry):
    """Every refusal is an argument check that returns before any allocation or launch.  The codes are the parent commit's."""
    ctx = prof
    L = glp.load_library()
    h = C.c_void_p()
    RB = 3
    vals = oracle.rand_field(np.random.default_rng(9), (2, 3, 1 << LG))
    desc = pr.synthetic(LG, 4, 3, 2, 1, seed=3)
    ch = oracle.rand_field(np.random.default_rng(10), (2, 2, 1))
    wires2 = np.stack([desc.wires, desc.wires])

    def call(K=2, log_n=LG, rb=RB, cap_height=2, hasher=0):
        if entry == "batch_many_from_values":
            rc = L.glp_batch_many_from_values(ctx._h, binding._p(vals), 0, K, 3, log_n, rb, cap_height, hasher, None, C.byref(h))
        elif entry == "batch_from_coset_values":
            rc = L.glp_batch_from_coset_values(ctx._h, binding._p(vals), 0, K, 3, log_n, 0, rb, cap_height, hasher, None, C.byref(h))
        else:
            d, keep = glp.perm_desc(desc)
            d.log_n = log_n
            rc = L.glp_perm_zs_commit(ctx._h, C.byref(d), K, binding._p(wires2), 0, binding._p(desc.sigmas), 0, binding._p(ch[0]), binding._p(ch[1]),
                                      rb, cap_height, hasher, None, C.byref(h))
        binding._chk(rc)
        glp.Batch(ctx, h, 0, log_n, rb, cap_height).free()

    cases = dict(rate_bits=lambda: call(rb=5), cap_height=lambda: call(cap_height=LG + RB + 1), log_n=lambda: call(log_n=25),
                 none=lambda: call(K=0), many=lambda: call(K=4097), hasher=lambda: call(hasher=2))
    for name, fn in cases.items():
        code, text = _code(fn)
        print(entry, name, code, text)
        assert code == REFUSALS[entry][name], (entry, name, code, text)
        assert not h.value, (entry, name)
        assert ctx.stages() == [], "a refused call reached a launch: %s" % (ctx.stages(),)
    call()                                  # the shape the refusals vary is served
    assert _names(ctx) != []
