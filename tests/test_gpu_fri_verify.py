"""glp_fri_verify_many / glp_fri_verify_queries_many / glp_fri_verify on the GPU (include/glp.h).  Every expected verdict is that of the
Python restatement tests/fri_restate.py::verify_fri_proof, never the library's alone: accepted where it returns 0, else rejected with
its number in the reason's "[check N]".  Fixtures (shape_c, Case, tampers) are pinned on the CPU in tests/test_fri_verify.py.
A. accepts what the restatement accepts   B. rejects with the restatement's check number   C. stepped equals one-call
D. the plonk instance from the CPU prover   E. group geometry   F. refusals"""
import ctypes as C
import re

import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import binding
import fri_restate as fr
from test_fri_openings import shape_b, _plonk_fri_slice
from test_fri_verify import Case, shape_c, tampers, plonk_desc

pytestmark = pytest.mark.gpu

K3 = 3                        # odd: 9 groups leave 7 idle in the one workgroup
SEED = [11, 22, 33, 44]
SHAPES = {"b": shape_b, "c": shape_c}


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _check(reason):
    m = re.search(r"\[check (\d)\]$", reason)
    assert m, "the reason %r does not end in [check N]" % reason
    return int(m.group(1))


def _verify(ctx, c, data):
    words, openings, caps, zs = data
    return glp.fri_verify_many(ctx, c.shapes, c.ranges, zs, *c.params, openings, words, c.states, c.pend, caps=caps, **c.geometry)


def _hold_to_restatement(oracle, c, data, status, reasons, members=None, what=""):
    """-> the restatement's codes of the members looked at"""
    codes = {}
    for k in range(c.K) if members is None else members:
        code = codes[k] = c.restated(oracle, k, data)
        if code == 0:
            assert status[k] == 0 and reasons[k] == "", (what, k, status[k], reasons[k])
        else:
            assert status[k] == -5 and _check(reasons[k]) == code, (what, k, code, status[k], reasons[k])
    return codes


# ------------------------------------------------------------------ A. accepts what the restatement accepts
# 2^2, 2^3, 2^5 points x the arities that fit x caps of 1 and 4 digests; the pending count walks 0 (output buffer refilled), 3, 7
_GEO = [(lg, ab, ch) for lg in (2, 3, 5) for ab in ([1, 2], [4], [2]) for ch in (0, 2) if sum(ab) <= lg]
CASES_A = [(s, lg, ab, ch, (0, 3, 7)[(i + j) % 3]) for j, s in enumerate("bc") for i, (lg, ab, ch) in enumerate(_GEO)]


@pytest.mark.parametrize("shape,log_n,arity_bits,cap_height,pending", CASES_A)
def test_accepts_the_restated_provers_proofs(ctx, oracle, shape, log_n, arity_bits, cap_height, pending):
    rng = np.random.default_rng(9000 + 100 * log_n + 10 * len(arity_bits) + cap_height + (shape == "c"))
    c = Case(oracle, rng, SHAPES[shape], K3, log_n, arity_bits, cap_height, pending=pending)
    data = c.data()
    status, reasons = _verify(ctx, c, data)
    codes = _hold_to_restatement(oracle, c, data, status, reasons)
    assert set(codes.values()) == {0} and list(status) == [0] * K3


@pytest.mark.parametrize("shape,hasher,arity_bits", [("c", 1, [1, 2]), ("b", 1, [2]), ("c", 0, []), ("b", 0, [])])
def test_accepts_under_keccak_and_without_reductions(ctx, oracle, shape, hasher, arity_bits):
    c = Case(oracle, np.random.default_rng(40 + hasher + len(arity_bits)), SHAPES[shape], K3, 3, arity_bits, 1, hasher=hasher)
    data = c.data()
    status, reasons = _verify(ctx, c, data)
    assert set(_hold_to_restatement(oracle, c, data, status, reasons).values()) == {0}


def _gpu_batches(ctx, c):
    """the case's polynomials committed on the GPU: oracle 0 a batch of one (shared), the rest many-proof batches (salted where the
    shape says so, with the library's own salts)"""
    i = c.inst0
    out = [ctx.batch_from_coeffs(c.co[0], i.rate_bits, i.cap_height, i.hasher)]
    for o in range(1, len(i.ncols)):
        out.append(ctx.batch_many_from_coeffs(c.co[o], i.rate_bits, i.cap_height, i.hasher, seed=SEED if i.salted[o] else None))
    return out


@pytest.mark.parametrize("shape,log_n,arity_bits,cap_height", [("b", 3, [1, 2], 0), ("c", 3, [2], 2), ("b", 5, [4], 2), ("c", 5, [1, 2], 0)])
def test_accepts_the_gpu_provers_proofs(ctx, oracle, shape, log_n, arity_bits, cap_height):
    """proofs of glp_fri_prove_many, the oracles handed over as live Batch objects (shape and caps taken from them)"""
    c = Case(oracle, np.random.default_rng(77 + log_n), SHAPES[shape], K3, log_n, arity_bits, cap_height, pending=0, prove=False)
    batches = _gpu_batches(ctx, c)
    ops, proofs = glp.fri_prove_many(ctx, batches, c.ranges, c.zs, *c.params, c.states, c.pend)
    status, reasons = glp.fri_verify_many(ctx, batches, c.ranges, c.zs, *c.params, ops, proofs, c.states, c.pend)
    data = (proofs, ops, [batches[0].cap()] + [b.caps() for b in batches[1:]], c.zs)
    assert set(_hold_to_restatement(oracle, c, data, status, reasons).values()) == {0}
    for b in batches:
        b.free()


# ------------------------------------------------------------------ B. rejects, with the restatement's check number
@pytest.fixture(scope="module")
def case_b5(oracle):
    return Case(oracle, np.random.default_rng(5151), shape_b, K3, 5, [1, 2], 2)


@pytest.fixture(scope="module")
def case_c3(oracle):
    return Case(oracle, np.random.default_rng(909), shape_c, K3, 3, [1, 2], 0)


@pytest.mark.parametrize("which", ["b5", "c3"])
def test_rejects_with_the_restatements_check_number(ctx, oracle, case_b5, case_c3, which):
    c = case_b5 if which == "b5" else case_c3
    seen = set()
    for name, member, expect, everyone, fn in tampers(c):
        data = c.data()
        fn(*data)
        status, reasons = _verify(ctx, c, data)
        codes = _hold_to_restatement(oracle, c, data, status, reasons, what=name)
        for k, code in codes.items():
            assert (code != 0) == (everyone or k == member), (name, k, code)
        seen |= set(codes.values())
    assert {0, 1, 2, 4, 6} <= seen and (5 in seen or 7 in seen)


# ------------------------------------------------------------------ C. stepped equals one-call
def _challenges(oracle, c, data):
    """alpha, the betas and the indices of every member from the oracle's Challenger on cloned transcripts, over the proofs in `data`"""
    words, i = data[0], c.inst0
    o_q, stride, o_f, final_len, o_pow, total = i.layout()
    capw = 4 << i.cap_height
    alphas, betas, idx = [], [], []
    for k in range(c.K):
        ch = fr.challenger_clone(oracle, c.chs[k])
        alphas.append(ch.get_ext())
        bk = []
        for r in range(len(i.arity_bits)):
            ch.observe_hashes(words[k][r * capw:(r + 1) * capw].reshape(-1, 4))
            bk.append(ch.get_ext())
        betas.append(bk)
        ch.observe(words[k][o_f:o_f + 2 * final_len])
        ch.observe(words[k][o_pow:o_pow + 1])
        ch.get()
        idx.append([ch.get() % (1 << i.lgN) for _ in range(i.nq)])
    return np.array(alphas, np.uint64), np.array(betas, np.uint64).reshape(c.K, len(i.arity_bits), 2), np.array(idx, np.uint64)


def _verify_stepped(ctx, oracle, c, data):
    words, openings, caps, zs = data
    al, be, ix = _challenges(oracle, c, data)
    return glp.fri_verify_queries_many(ctx, c.shapes, c.ranges, zs, *c.params, openings, words, al, be, ix, caps=caps, **c.geometry)


@pytest.mark.parametrize("hasher", [0, 1])
def test_stepped_equals_one_call(ctx, oracle, hasher):
    c = Case(oracle, np.random.default_rng(300 + hasher), shape_c, K3, 3, [1, 2], 1, hasher=hasher)
    picked = [t for t in tampers(c) if t[0] in ("a leaf word of oracle 2", "a fold evaluation in the second query round", "one claimed opening")]
    assert len(picked) == 3                                   # none of them enters the transcript: the caller checks the proof of work itself
    for name, fn in [("untouched", None)] + [(t[0], t[4]) for t in picked]:
        data = c.data()
        if fn:
            fn(*data)
        one = _verify(ctx, c, data)
        stepped = _verify_stepped(ctx, oracle, c, data)
        assert list(one[0]) == list(stepped[0]) and one[1] == stepped[1], (name, one, stepped)
        codes = _hold_to_restatement(oracle, c, data, *stepped, what=name)
        assert (sum(v != 0 for v in codes.values()) == 1) == (fn is not None), (name, codes)


# ------------------------------------------------------------------ D. the plonk instance, from the CPU prover
@pytest.mark.parametrize("which", ["poseidon", "keccak"])
def test_plonk_instance_from_the_cpu_prover(ctx, oracle, which):
    """a proof the GPU never touched: four oracles, two points; the seven tampers of test_restated_verifier_on_the_oracle_provers_fri"""
    inst, caps, pts, words, ch = _plonk_fri_slice(oracle, plonk_desc(which))
    shapes = [(c, 0, 0) for c in inst.ncols]
    state, pend = fr.challenger_state(ch)
    L = glp.load_library()

    def verdict(w, op):
        ok = glp.fri_verify(ctx, shapes, inst.points, inst.arity_bits, inst.pow_bits, inst.nq, op, w, state, pend, caps=caps, log_n=inst.log_n,
                            rate_bits=inst.rate_bits, cap_height=inst.cap_height, hasher=inst.hasher)
        want = fr.verify_fri_proof(oracle, inst, caps, op, w, fr.challenger_clone(oracle, ch))
        assert ok == (want == 0)
        if want:
            assert _check(L.glp_last_error().decode()) == want
        return want

    assert verdict(words, pts) == 0
    o_q, stride, o_f, final_len, o_pow, total = inst.layout()
    ll0, depth0 = inst.leaf_len[0], inst.lgN - inst.cap_height
    rec = o_q + stride
    layer0 = rec + sum(ll + 4 * depth0 for ll in inst.leaf_len)
    places = {"commit cap": 5, "leaf": rec + 3, "path": rec + ll0 + 6, "eval": layer0 + 1, "layer path": layer0 + (2 << inst.arity_bits[0]) + 2,
              "final polynomial": o_f + 1, "witness": o_pow}
    for name, at in places.items():
        bad = words.copy()
        bad[at] = (int(bad[at]) + 1) % fr.P
        assert verdict(bad, pts) != 0, name
    wrong = pts.copy()
    wrong[7, 0] = (int(wrong[7, 0]) + 1) % fr.P
    assert verdict(words, wrong) != 0


# ------------------------------------------------------------------ E. group geometry
def test_second_workgroup_partly_idle(ctx, oracle):
    """K = 7, three query rounds: 21 groups, 16 in the first workgroup and 5 in the second"""
    c = Case(oracle, np.random.default_rng(21), shape_c, 7, 2, [2], 0)
    data = c.data()
    data[0][6][c.inst0.layout()[0] + 1] ^= np.uint64(1)       # member 6 lives in the second workgroup
    status, reasons = _verify(ctx, c, data)
    codes = _hold_to_restatement(oracle, c, data, status, reasons)
    assert [k for k, v in codes.items() if v] == [6]


def test_256_proofs_two_damaged(ctx, oracle):
    K = 256
    c = Case(oracle, np.random.default_rng(256), shape_b, K, 3, [1, 2], 1, pending=0, prove=False)
    batches = _gpu_batches(ctx, c)
    ops, proofs = glp.fri_prove_many(ctx, batches, c.ranges, c.zs, *c.params, c.states, c.pend)
    o_q, stride, o_f = c.inst0.layout()[:3]
    proofs[5][o_q + stride + 2] = (int(proofs[5][o_q + stride + 2]) + 1) % fr.P        # a leaf word of the second query round
    proofs[250][o_f - 1] = (int(proofs[250][o_f - 1]) + 1) % fr.P                      # the last layer path word of the last round
    status, reasons = glp.fri_verify_many(ctx, batches, c.ranges, c.zs, *c.params, ops, proofs, c.states, c.pend)
    assert [k for k in range(K) if status[k] != 0] == [5, 250] and all(r == "" for k, r in enumerate(reasons) if k not in (5, 250))
    data = (proofs, ops, [batches[0].cap()] + [b.caps() for b in batches[1:]], c.zs)
    codes = _hold_to_restatement(oracle, c, data, status, reasons, members=[0, 5, 128, 250, 255])
    assert codes == {0: 0, 5: 4, 128: 0, 250: 6, 255: 0}
    for b in batches:
        b.free()


# ------------------------------------------------------------------ F. refusals (all decided on the host, before any launch)
def _refused(fn):
    with pytest.raises(glp.GlpError) as e:
        fn()
    return e.value.code, str(e.value)


def test_refusals(ctx, oracle, case_c3):
    c = case_c3
    words, openings, caps, zs = c.data()
    ab, pw, nq = c.params
    geo = c.geometry

    def call(shapes=c.shapes, ranges=c.ranges, zs=zs, ab=ab, pw=pw, nq=nq, caps=caps, pend=c.pend, **over):
        return _refused(lambda: glp.fri_verify_many(ctx, shapes, ranges, zs, ab, pw, nq, openings, words, c.states, pend, caps=caps, **dict(geo, **over)))

    def with_point(b, ranges):
        return [((0, 0), ranges if i == b else r) for i, (_, r) in enumerate(c.ranges)]

    for args, fragment in [
            (dict(shapes=[], caps=[]), "num_oracles"), (dict(shapes=[c.shapes[0]] * 9, caps=[caps[0]] * 9), "num_oracles"),
            (dict(ranges=c.ranges + [c.ranges[0]], zs=np.zeros((K3, 5, 2), np.uint64)), "num_points"),
            (dict(ranges=with_point(3, [(3, 0, 1)] * 17)), "num_ranges"),
            (dict(ranges=with_point(1, [(1, 7, 10)])), "ncols"), (dict(ranges=with_point(1, [(1, 17, 0)])), "ncols"),
            (dict(ranges=with_point(2, [(4, 0, 1)])), "oracle"),
            (dict(ranges=with_point(2, [])), "points[2] names no polynomial"), (dict(ranges=with_point(0, [(0, 1, 0)])), "points[0] names no polynomial"),
            (dict(ab=[1, 0]), "reduction_arity_bits[1]"), (dict(ab=[5]), "reduction_arity_bits[0]"), (dict(ab=[2, 2]), "sum"),
            (dict(ab=[1] * 17), "reductions"),
            (dict(nq=0), "num_query_rounds"), (dict(hasher=2), "hasher"), (dict(pw=33), "proof_of_work_bits"),
            (dict(pend=np.zeros((K3, 8), np.uint64)), "num_pending")]:
        code, msg = call(**args)
        assert code == -1 and fragment in msg, (fragment, msg)
    # what the binding cannot express: a proof count out of range and null pointers, on the C ABI itself
    L = glp.load_library()
    d, keep = binding._fri_verify_desc_to_c(c.shapes, c.ranges, geo["log_n"], geo["rate_bits"], geo["cap_height"], 0, ab, pw, nq, num_proofs=K3)
    cs = [binding._a(x) for x in caps]
    ptrs = (C.c_void_p * 4)(*[x.ctypes.data for x in cs])
    status = np.zeros(K3, np.int32)
    good = dict(K=K3, points=binding._p(zs), caps=ptrs, openings=binding._p(openings), proofs=binding._p(words), states=binding._p(c.states),
                pending=binding._p(c.pend), npend=c.pend.shape[1], status=status.ctypes.data_as(C.c_void_p))

    def raw(**over):
        a = dict(good, **over)
        rc = L.glp_fri_verify_many(ctx._h, C.byref(d), a["K"], a["points"], a["caps"], a["openings"], a["proofs"], a["states"], a["pending"], a["npend"],
                                   a["status"], None)
        return rc, L.glp_last_error().decode()

    assert raw()[0] == 0 and list(status) == [0] * K3
    one_null = (C.c_void_p * 4)(ptrs[0], ptrs[1], None, ptrs[3])
    for over, fragment in [(dict(K=0), "num_proofs"), (dict(K=65537), "num_proofs"), (dict(points=None), "points"), (dict(caps=None), "caps"),
                           (dict(caps=one_null), "caps[2]"), (dict(openings=None), "openings"), (dict(proofs=None), "proofs"),
                           (dict(states=None), "sponge_states"), (dict(pending=None), "pending_inputs"), (dict(status=None), "status_out")]:
        rc, msg = raw(**over)
        assert rc == -1 and fragment in msg, (fragment, rc, msg)
    assert L.glp_fri_verify_many(ctx._h, None, K3, good["points"], ptrs, good["openings"], good["proofs"], good["states"], good["pending"], good["npend"],
                                 good["status"], None) == -1 and "desc" in L.glp_last_error().decode()
    del keep
    # the stepped form: an index outside the LDE domain, a challenge that is not canonical
    data = c.data()
    al, be, ix = _challenges(oracle, c, data)

    def stepped(al=al, be=be, ix=ix):
        return _refused(lambda: glp.fri_verify_queries_many(ctx, c.shapes, c.ranges, zs, ab, pw, nq, openings, words, al, be, ix, caps=caps, **geo))

    bad = ix.copy()
    bad[1, 2] = 1 << c.inst0.lgN
    code, msg = stepped(ix=bad)
    assert code == -1 and "indices[1]" in msg
    bad = al.copy()
    bad[2, 1] = glp.P
    code, msg = stepped(al=bad)
    assert code == -1 and "alphas[2]" in msg
    for word in (glp.P, 2 ** 64 - 1):
        bad = be.copy()
        bad[1, be.shape[1] - 1, 1] = word
        code, msg = stepped(be=bad)
        assert code == -1 and "betas[1]" in msg and "canonical" in msg
    # one proof: a damaged proof is GLP_ERR_PROVE with the check in glp_last_error, not an exception
    one = dict(caps=[caps[0]] + [x[0] for x in caps[1:]], **geo)
    assert glp.fri_verify(ctx, c.shapes, c.inst(0).points, ab, pw, nq, openings[0], words[0], c.states[0], c.pend[0], **one) is True
    hurt = words[0].copy()
    hurt[c.inst0.layout()[0]] ^= np.uint64(1)
    assert glp.fri_verify(ctx, c.shapes, c.inst(0).points, ab, pw, nq, openings[0], hurt, c.states[0], c.pend[0], **one) is False
    assert _check(L.glp_last_error().decode()) == 4
    d1, keep1 = binding._fri_verify_desc_to_c(c.shapes, c.inst(0).points, geo["log_n"], geo["rate_bits"], geo["cap_height"], 0, ab, pw, nq)
    one_ptrs = (C.c_void_p * 4)(*[binding._a(x).ctypes.data for x in one["caps"]])
    assert L.glp_fri_verify(ctx._h, C.byref(d1), one_ptrs, binding._p(openings[0]), binding._p(hurt), binding._p(c.states[0]), binding._p(c.pend[0]),
                            c.pend.shape[1]) == -5
    del keep1
