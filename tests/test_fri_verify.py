"""glp_fri_verify*: the part that needs no GPU, and the fixtures tests/test_gpu_fri_verify.py shares.

`shape_c` is an instance at the verifier's limits (four oracles with leaves of 4, 20, 17 and 9 words, four points, 17-column and
mid-oracle ranges, an oracle split across two points, a column no point names).  `Case` builds K proofs of an instance with
tests/fri_restate.py alone (no GPU prover involved); `tampers` lists the one-word damages of section B with the check numbers the
restatement can answer for each.  Here, on the CPU: the restated verifier accepts the restated prover's proofs of shape_c and answers
every tamper with one of the expected numbers; the sizes the library computes equal the restatement's; the entry points are
declared, exported, bound and documented; without a GPU the bindings raise GlpError."""
import os
import subprocess

import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
import fri_restate as fr
from test_fri_openings import shape_b

NEW = ["glp_fri_verify_proof_words", "glp_fri_verify_num_openings", "glp_fri_verify_many", "glp_fri_verify_queries_many", "glp_fri_verify"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = fr.P


def shape_c(rng, oracle, log_n, arity_bits, cap_height, rate_bits=3, hasher=0, pow_bits=6, nq=3):
    """Four oracles (4, 16 salted, 17, 9 columns: leaves of 4 words -- hash_or_noop copies them --, 20, 17 and 9 words -- one past the
    8-word sponge chunk) and four points (GLP_FRI_MAX_POINTS).  Oracle 1 is split across points 0 and 1, the second half starting
    mid-oracle; point 0 names a 17-column range (more than one 16-lane stride); no point names column 8 of oracle 3.
    -> (instance, coefficient arrays, salts of oracle 1 [N][4]), the signature of shape_b"""
    ncols = [4, 16, 17, 9]
    coeffs = [oracle.rand_field(rng, (c, 1 << log_n)) for c in ncols]
    salts = oracle.rand_field(rng, (1 << (log_n + rate_bits), 4))
    z = [tuple(int(v) for v in oracle.rand_field(rng, 2)) for _ in range(4)]
    points = [(z[0], [(0, 0, 4), (1, 0, 7), (2, 0, 17)]), (z[1], [(1, 7, 9), (3, 2, 3)]), (z[2], [(3, 0, 2), (0, 1, 2)]), (z[3], [(3, 5, 3)])]
    inst = fr.Instance(log_n, rate_bits, cap_height, hasher, ncols, [False, True, False, False], points, arity_bits, pow_bits, nq)
    return inst, coeffs, salts


class Case:
    """K proofs of one instance (shape_b or shape_c): oracle 0 shared by all proofs, every other oracle per proof, every proof at its
    own points and on its own transcript (left with `pending` buffered inputs).  Everything comes from tests/fri_restate.py."""

    def __init__(self, oracle, rng, shape, K, log_n, arity_bits, cap_height, hasher=0, pending=3, nq=3, prove=True):
        inst0, co, _ = shape(rng, oracle, log_n, arity_bits, cap_height, hasher=hasher, nq=nq)
        self.K, self.inst0, self.hasher = K, inst0, hasher
        self.ranges = [((0, 0), r) for _, r in inst0.points]
        n, N, nor = 1 << log_n, 1 << inst0.lgN, len(inst0.ncols)
        self.co = [co[0]] + [oracle.rand_field(rng, (K, c, n)) for c in inst0.ncols[1:]]
        self.salts = [oracle.rand_field(rng, (K, N, 4)) if s else None for s in inst0.salted]
        self.zs = oracle.rand_field(rng, (K, len(inst0.points), 2))
        self.shapes = [(c, int(s), int(o == 0)) for o, (c, s) in enumerate(zip(inst0.ncols, inst0.salted))]
        self.params = (inst0.arity_bits, inst0.pow_bits, inst0.nq)
        self.geometry = dict(log_n=log_n, rate_bits=inst0.rate_bits, cap_height=cap_height, hasher=hasher)
        self.ref = self.caps = None                           # the restated commitments: not built for a case the GPU commits and proves
        if prove or pending:
            shared = fr.commit(oracle, self.co[0], inst0.rate_bits, cap_height, hasher)
            self.ref = [[shared] + [fr.commit(oracle, self.co[o][k], inst0.rate_bits, cap_height, hasher, None if self.salts[o] is None else self.salts[o][k])
                                    for o in range(1, nor)] for k in range(K)]
            self.caps = [shared.cap.copy()] + [np.stack([self.ref[k][o].cap for k in range(K)]) for o in range(1, nor)]
        self.chs = []
        for k in range(K):
            ch = oracle.Challenger(hasher)
            if pending:
                for ob in self.ref[k]:
                    ch.observe_hashes(ob.cap)
                have = fr.challenger_state(ch)[1].size
                ch.observe(oracle.rand_field(rng, (pending - have) % 8 or 8))
            else:
                ch.observe(oracle.rand_field(rng, 16))       # fills the rate twice: nothing pending, the output buffer refilled
            assert fr.challenger_state(ch)[1].size == pending
            self.chs.append(ch)
        sp = [fr.challenger_state(ch) for ch in self.chs]
        self.states, self.pend = np.stack([s for s, _ in sp]), np.stack([p for _, p in sp])
        self.openings = self.words = None
        if prove:
            got = [fr.prove_openings(oracle, self.inst(k), self.ref[k], fr.challenger_clone(oracle, self.chs[k])) for k in range(K)]
            self.openings = np.stack([np.array(op, np.uint64) for op, _ in got])
            self.words = np.stack([w for _, w in got])

    def inst(self, k, zs=None):
        i0, z = self.inst0, self.zs if zs is None else zs
        return fr.Instance(i0.log_n, i0.rate_bits, i0.cap_height, i0.hasher, i0.ncols, i0.salted,
                           [(tuple(int(v) for v in z[k][b]), r) for b, (_, r) in enumerate(i0.points)], i0.arity_bits, i0.pow_bits, i0.nq)

    def data(self):
        """a private copy of what a verifier is handed: (words [K][total], openings [K][count][2], caps per oracle, zs [K][points][2])"""
        return self.words.copy(), self.openings.copy(), [c.copy() for c in self.caps], self.zs.copy()

    def restated(self, oracle, k, data=None):
        """the verdict of tests/fri_restate.py for member k (0 = accepted, else the number of the failed check)"""
        words, openings, caps, zs = self.data() if data is None else data
        mine = [caps[0]] + [c[k] for c in caps[1:]]
        return fr.verify_fri_proof(oracle, self.inst(k, zs), mine, openings[k], words[k], fr.challenger_clone(oracle, self.chs[k]))


def _bump(a, at):
    a[at] = (int(a[at]) + 1) % P


def tampers(case):
    """Section B: [(name, member damaged, numbers the restatement may answer, all_members, fn(words, openings, caps, zs))].  One word
    is replaced by itself + 1 mod p (or by p); a different member each time.  Where the damaged word enters the transcript the proof
    of work fails with probability 63/64 (check 2) and only otherwise a later check."""
    i = case.inst0
    o_q, stride, o_f, final_len, o_pow, total = i.layout()
    depth0, nor, nred = i.lgN - i.cap_height, len(i.ncols), len(i.arity_bits)
    leaf_at = [o_q + sum(i.leaf_len[:o]) + 4 * depth0 * o for o in range(nor)]          # first query round
    rec1 = o_q + stride                                                                 # the second query round
    layer0 = rec1 + sum(ll + 4 * depth0 for ll in i.leaf_len)
    out = []

    def add(name, expect, fn, everyone=False):
        out.append((name, len(out) % case.K, set(expect), everyone, fn))

    def word(at):
        return lambda k: (lambda w, op, caps, zs: _bump(w[k], at))

    per_member = []
    if nred:
        per_member.append(("a layer cap", {2, 5, 6}, word(1)))
    for o in range(nor):
        per_member.append(("a leaf word of oracle %d" % o, {4}, word(leaf_at[o] + i.leaf_len[o] // 2)))
    for o in range(nor):
        if i.salted[o]:
            per_member.append(("the last salt of oracle %d" % o, {4}, word(leaf_at[o] + i.leaf_len[o] - 1)))
    if depth0:
        per_member.append(("an initial path word", {4}, word(leaf_at[1] + i.leaf_len[1] + 2)))
    if nred:
        per_member.append(("a fold evaluation in the second query round", {5, 6}, word(layer0 + 1)))
        if i.lgN - i.arity_bits[0] - i.cap_height:
            per_member.append(("a layer path word", {6}, word(layer0 + (2 << i.arity_bits[0]) + 1)))
    per_member.append(("a final-polynomial word", {2, 7}, word(o_f + 1)))
    per_member.append(("the witness", {2, 4}, word(o_pow)))
    per_member.append(("a word set to p", {1}, lambda k: (lambda w, op, caps, zs: w[k].__setitem__(leaf_at[2] + 1, np.uint64(P)))))
    per_member.append(("one claimed opening", {5, 7}, lambda k: (lambda w, op, caps, zs: _bump(op[k].reshape(-1), 2 * (len(op[k]) - 2)))))
    per_member.append(("a per-proof cap word", {4}, lambda k: (lambda w, op, caps, zs: _bump(caps[nor - 1][k].reshape(-1), 2))))
    per_member.append(("one coordinate of one point", {5, 7}, lambda k: (lambda w, op, caps, zs: _bump(zs[k].reshape(-1), 3))))
    for name, expect, mk in per_member:
        add(name, expect, mk(len(out) % case.K))
    add("the shared cap word", {4}, lambda w, op, caps, zs: _bump(caps[0].reshape(-1), 1), everyone=True)
    return out


def plonk_desc(which):
    """the arithmetic circuits of test_restated_verifier_on_the_oracle_provers_fri"""
    if which == "poseidon":
        return synth.arith_circuit(6, synth.Config.standard_recursion_config(), seed=106)
    d = synth.arith_circuit(7, synth.Config.standard_recursion_config(), seed=12)
    d.hasher, d.circuit_digest = 1, None
    return d


# ------------------------------------------------------------------ the fixtures, pinned on the CPU
@pytest.fixture(scope="module")
def case_c(oracle):
    return Case(oracle, np.random.default_rng(909), shape_c, 3, 3, [1, 2], 0)


def test_shape_c_is_what_it_claims(oracle, case_c):
    i = case_c.inst0
    assert i.leaf_len == [4, 20, 17, 9] and len(i.points) == 4 and i.num_openings == 28 + 12 + 4 + 3
    named = [set(c for b in range(4) for o, c in i.columns(b) if o == k) for k in range(4)]
    assert named[3] == set(range(8)) and named[1] == set(range(16)) and max(r[2] for _, rs in i.points for r in rs) == 17
    assert {b for b in range(4) for o, _ in i.columns(b) if o == 1} == {0, 1}
    assert any(cb > 0 for _, rs in i.points for _, cb, _ in rs)


def test_restated_verifier_accepts_the_restated_prover_on_shape_c(oracle, case_c):
    assert case_c.words.shape == (3, case_c.inst0.layout()[5])
    for k in range(3):
        assert case_c.restated(oracle, k) == 0


def test_every_tamper_is_rejected_with_an_expected_check(oracle, case_c):
    seen = set()
    for name, member, expect, everyone, fn in tampers(case_c):
        data = case_c.data()
        fn(*data)
        for k in range(case_c.K):
            code = case_c.restated(oracle, k, data)
            if everyone or k == member:
                assert code in expect, (name, k, code)
                seen.add(code)
            else:
                assert code == 0, (name, k, code)
    assert {1, 2, 4, 6} <= seen and (5 in seen or 7 in seen)


# ------------------------------------------------------------------ sizes and bindings
def _plonk_instance(which):
    desc = plonk_desc(which)
    inst = fr.plonk_instance(desc, (3, 5))
    return inst


@pytest.mark.parametrize("which", ["shape_b", "shape_c", "plonk", "plonk keccak"])
def test_sizes_equal_the_restatement(oracle, which):
    rng = np.random.default_rng(3)
    if which.startswith("plonk"):
        inst = _plonk_instance("keccak" if "keccak" in which else "poseidon")
    else:
        inst = (shape_b if which == "shape_b" else shape_c)(rng, oracle, 5, [1, 2], 2)[0]
    shapes = [(c, int(s), 0) for c, s in zip(inst.ncols, inst.salted)]
    words, nopen = glp.fri_verify_sizes(shapes, inst.points, inst.arity_bits, inst.pow_bits, inst.nq, log_n=inst.log_n, rate_bits=inst.rate_bits,
                                        cap_height=inst.cap_height, hasher=inst.hasher)
    assert words == inst.layout()[5] and nopen == inst.num_openings
    # a description the verifier refuses has no size
    assert glp.fri_verify_sizes(shapes, inst.points, [5], inst.pow_bits, inst.nq, log_n=inst.log_n, rate_bits=inst.rate_bits,
                                cap_height=inst.cap_height, hasher=inst.hasher) == (0, 0)


def test_new_functions_are_declared_exported_bound_and_documented():
    glp.build_library()
    declared = glp.exported_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", glp.library_path()]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = glp.load_library()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in declared, name + " is not declared in include/glp.h"
        assert name in exported, name + " is not exported by libglprover.so"
        assert getattr(L, name).argtypes, name + " has no argtypes in binding.py"
        assert "fn " + name + "(" in integration, name + " is missing from INTEGRATION.md's extern block"
    for name in ("fri_verify", "fri_verify_many", "fri_verify_queries_many"):
        assert callable(getattr(glp, name))


def test_without_a_context_the_bindings_raise(oracle, case_c):
    class NoContext:
        _h = None
    c = case_c
    calls = [
        lambda: glp.fri_verify_many(NoContext, c.shapes, c.ranges, c.zs, *c.params, c.openings, c.words, c.states, c.pend, caps=c.caps, **c.geometry),
        lambda: glp.fri_verify_queries_many(NoContext, c.shapes, c.ranges, c.zs, *c.params, c.openings, c.words, np.ones((3, 2), np.uint64),
                                            np.ones((3, 2, 2), np.uint64), np.zeros((3, 3), np.uint64), caps=c.caps, **c.geometry),
        lambda: glp.fri_verify(NoContext, c.shapes, c.inst(0).points, *c.params, c.openings[0], c.words[0], c.states[0], c.pend[0],
                               caps=[c.caps[0]] + [x[0] for x in c.caps[1:]], **c.geometry),
    ]
    for call in calls:
        with pytest.raises(glp.GlpError) as e:
            call()
        assert e.value.code == -1 and "ctx is null" in str(e.value)
    with pytest.raises(glp.GlpError):                         # a wrong length is the binding's to refuse: the C ABI takes bare pointers
        glp.fri_verify_many(NoContext, c.shapes, c.ranges, c.zs, *c.params, c.openings, c.words[:, :-1], c.states, c.pend, caps=c.caps, **c.geometry)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        with pytest.raises(glp.GlpError) as e:
            glp.Context(0)
        assert "no CPU fallback" in str(e.value)
