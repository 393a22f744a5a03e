"""The FRI seam swept word by word: glp_fri_verify_many (the library's transcript) and glp_fri_verify_queries_many (the caller's
challenges) over K members in lock step, member j being member 0's data with input j replaced by itself + 1 mod p, for EVERY word
of the FriProof and, in the steered form, every coordinate of every opening, every cap word and every point coordinate.

Where the words live comes from tests/proof_sections.py::fri_sections, the expected verdicts from reasoning written down below
and from tests/fri_restate.py::verify_fri_proof (on the first and last word of each section of each round and a stride sample;
the device sweep covers everything).  Fixtures: Case, shape_b, shape_c as tests/test_fri_verify.py pins them, with K = 1; the
K-fold copies are built here.

Transcript form: every word either enters the transcript (layer caps, final polynomial, witness: the proof of work then fails
with probability 63/64, check 2, and otherwise a later check: the sets of test_fri_verify.py::tampers, and check 4 where the
indices have moved) or follows the last challenge
and is held by exactly one check (query leaves, salts, paths, fold evaluations: the reasons of proof_sections.reasons).
Steered form: the challenges do not move, so each input is held by its own check or by none, and the verdict is known exactly:
  leaf, salt, initial path            check 4            fold evaluations   5 (the slot of x_index) or 6      layer path   6
  final polynomial coefficient        7 (its term x^i c_i changes)          witness    accepted (the caller checks the proof of work)
  cap word (layer, per proof, shared) the check of its tree (6, 4, 4) if some query index lands under that cap digest, else accepted
  opening, point coordinate           the reduced opening or the denominator of its point moves: 5, or 7 without reductions
Under KeccakHash<25> the fourth word of a digest holds one byte: a damaged value above 0xFF is refused by check 1.

Each sweep prints a `SWEEP` line (inputs swept, seconds on the device path, seconds of the restatement): run with -s."""
import time

import numpy as np
import pytest

import plonky2_lib_amd as glp
import fri_restate as fr
import proof_sections as ps
from test_fri_openings import shape_b
from test_fri_verify import Case, shape_c
from test_gpu_fri_verify import _challenges, _check

pytestmark = pytest.mark.gpu

STRIDE = 5
CASES = {
    "c3": lambda oracle: Case(oracle, np.random.default_rng(909), shape_c, 1, 3, [1, 2], 0),
    "b5": lambda oracle: Case(oracle, np.random.default_rng(5151), shape_b, 1, 5, [4], 2),
    "c3 keccak": lambda oracle: Case(oracle, np.random.default_rng(910), shape_c, 1, 3, [1, 2], 0, hasher=1),
}
# tampers' sets, plus check 4 for the words that enter the transcript: where the proof of work still passes (1 in 64) the query indices
# have moved with it, and the first initial tree of the first round is the first check to see leaves of other indices
TRANSCRIPT_SETS = {"layer_cap": {2, 4, 5, 6}, "leaf": {4}, "salt": {4}, "path": {4}, "evals": {5, 6}, "layer_path": {6}, "final_poly": {2, 4, 7}, "pow": {2, 4}}


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


_cases = {}


@pytest.fixture(params=list(CASES))
def case(request, oracle):
    if request.param not in _cases:
        c = CASES[request.param](oracle)
        i = c.inst0
        c.secs = ps.fri_sections(i.ncols, i.salted, i.log_n, i.rate_bits, i.cap_height, i.arity_bits, i.nq)
        assert ps.tiles(c.secs, c.words.shape[1]) and c.restated(oracle, 0) == 0
        c.sec_of = ps.section_of(c.secs)
        c.label = request.param
        _cases[request.param] = c
    return _cases[request.param]


def _inputs(c, steered):
    """[(where, flat index)]: where = 'words', and steered also 'openings', 'points' and 'caps<o>' of every per-proof oracle"""
    out = [("words", at) for at in range(c.words.shape[1])]
    if steered:
        out += [("openings", j) for j in range(c.openings[0].size)]
        out += [("caps%d" % o, j) for o in range(1, len(c.caps)) for j in range(c.caps[o][0].size)]
        out += [("points", j) for j in range(c.zs[0].size)]
    return out


def _members(c, inputs):
    """K-fold copies of member 0's data with input j damaged in a member of its own, an untouched copy first, last and in the middle;
    K odd: the K x 3 groups never fill the last workgroup -> (data, states, pend, rows of the damaged members, rows of the untouched)"""
    clean = [0, 1 + len(inputs) // 2, len(inputs) + 2]
    if (len(inputs) + 3) % 2 == 0:
        clean.append(len(inputs) + 3)
    K = len(inputs) + len(clean)
    assert K % 2 == 1 and K <= 65536
    rows = [k for k in range(K) if k not in set(clean)]
    rep = lambda a: np.repeat(np.asarray(a)[None], K, axis=0)
    data = {"words": rep(c.words[0]), "openings": rep(c.openings[0]), "points": rep(c.zs[0])}
    for o in range(1, len(c.caps)):
        data["caps%d" % o] = rep(c.caps[o][0])
    for k, (where, j) in zip(rows, inputs):
        flat = data[where][k].reshape(-1)
        flat[j] = np.uint64(ps.bumped(flat[j]))
    return data, rep(c.states[0]), rep(c.pend[0]), rows, clean


def _caps(c, data, shared=None):
    return [c.caps[0].copy() if shared is None else shared] + [data["caps%d" % o] for o in range(1, len(c.caps))]


def _one(c, data, k, shared=None):
    """member k as a batch of one, the form Case.restated takes"""
    return (data["words"][k:k + 1], data["openings"][k:k + 1], [c.caps[0] if shared is None else shared] + [data["caps%d" % o][k:k + 1] for o in range(1, len(c.caps))],
            data["points"][k:k + 1])


def _keccak_byte(c, where, j):
    """True if input j is the fourth word of a KeccakHash<25> digest and its damaged value no longer fits one byte"""
    if c.hasher != 1 or j % 4 != 3:
        return False
    if where == "words":
        sec = c.secs[c.sec_of[j]]
        if sec.kind not in ps.DIGEST_KINDS or (j - sec.lo) % 4 != 3:
            return False
        return ps.bumped(c.words[0][j]) > 0xFF
    if where.startswith("caps"):
        return ps.bumped(c.caps[int(where[4:])][0].reshape(-1)[j]) > 0xFF
    return where == "shared" and ps.bumped(c.caps[0].reshape(-1)[j]) > 0xFF


def _sample(c, inputs):
    """positions in `inputs` the restatement is asked about: first and last word of each section of each round and every STRIDE-th
    word of the proof; first, last and every STRIDE-th of the other inputs"""
    words = set(ps.sample(c.secs, STRIDE))
    out, seen = [], {}
    for n, (where, j) in enumerate(inputs):
        seen.setdefault(where, []).append(n)
        if where == "words" and j in words:
            out.append(n)
    for where, ns in seen.items():
        if where != "words":
            out += sorted(set([ns[0], ns[-1]] + ns[::STRIDE]))
    return out


def _allowed(sec):
    """reasons of a query-phase section with the seam's check numbers: 4 initial tree, 5 consistency, 6 layer tree"""
    merkle = " [check 4]" if sec.kind in ("leaf", "salt", "path") else " [check 6]"
    return [r + (" [check 5]" if r == ps.fold_reason(sec) else merkle) for r in ps.reasons(sec)]


def _assert_clean(status, reasons, clean):
    for k in clean:
        assert status[k] == 0 and reasons[k] == "", ("an untouched member was rejected", k, reasons[k])


def test_transcript_form(ctx, oracle, case):
    c = case
    inputs = _inputs(c, steered=False)
    data, states, pend, rows, clean = _members(c, inputs)
    t0 = time.perf_counter()
    status, reasons = glp.fri_verify_many(ctx, c.shapes, c.ranges, data["points"], *c.params, data["openings"], data["words"], states, pend,
                                          caps=_caps(c, data), **c.geometry)
    device_s = time.perf_counter() - t0
    _assert_clean(status, reasons, clean)
    assert len(rows) == c.words.shape[1]
    accepted = [j for k, (_, j) in zip(rows, inputs) if status[k] == 0]
    assert accepted == [], "%d damaged members accepted: %s" % (len(accepted), [(j, c.secs[c.sec_of[j]].name) for j in accepted[:8]])
    wrong, folds = [], {}
    for k, (_, j) in zip(rows, inputs):
        sec = c.secs[c.sec_of[j]]
        code = _check(reasons[k])
        if _keccak_byte(c, "words", j):
            ok = code == 1
        elif sec.kind in ps.QUERY_KINDS:                   # held by one check of its own: the reason names the round and the tree
            ok = reasons[k] in _allowed(sec)
            if sec.kind == "evals" and reasons[k].startswith(ps.fold_reason(sec)):
                folds.setdefault(sec.name, []).append(j - sec.lo)
        else:
            ok = code in TRANSCRIPT_SETS[sec.kind]
        if not ok or status[k] != -5:
            wrong.append((j, sec.name, reasons[k]))
    assert wrong == [], wrong[:8]
    for sec in c.secs:
        if sec.kind == "evals":
            slot = folds.get(sec.name, [])
            assert len(slot) == 2 and slot[0] % 2 == 0 and slot[1] == slot[0] + 1, (sec.name, slot)
    t0 = time.perf_counter()
    sample = _sample(c, inputs)
    for n in sample:
        k = rows[n]
        want = c.restated(oracle, 0, _one(c, data, k))
        assert want != 0 and (_check(reasons[k]) == want or _keccak_byte(c, "words", inputs[n][1])), (inputs[n], want, reasons[k])
    print("\nSWEEP fri %-10s transcript  inputs %4d  K %4d in one call  device %.2f s  restatement %.2f s (%d inputs, s = %d)"
          % (c.label, len(inputs), len(rows) + len(clean), device_s, time.perf_counter() - t0, len(sample), STRIDE))


class Fixed:
    """the Challenger of fri_restate.verify_fri_proof, answering with the caller's challenges: alpha and the betas, a proof-of-work
    response that passes, the indices"""

    def __init__(self, alpha, betas, idx):
        self.ext = [tuple(int(v) for v in alpha)] + [tuple(int(v) for v in b) for b in betas]
        self.vals = [0] + [int(x) for x in idx]

    def observe(self, *a):
        pass

    observe_hashes = observe

    def get_ext(self):
        return self.ext.pop(0)

    def get(self):
        return self.vals.pop(0)


def _steered_expect(c, where, j, idx):
    """the check that holds input j under fixed challenges (0: none), by the reasoning at the top of this file"""
    i = c.inst0
    under = {int(x) >> (i.lgN - i.cap_height) for x in idx}           # cap digests some query's paths end in
    if _keccak_byte(c, where, j):
        return 1
    if where == "words":
        kind = c.secs[c.sec_of[j]].kind
        if kind == "layer_cap":
            return 6 if ((j - c.secs[c.sec_of[j]].lo) // 4) in under else 0
        return {"leaf": 4, "salt": 4, "path": 4, "evals": (5, 6), "layer_path": 6, "final_poly": 7, "pow": 0}[kind]
    if where.startswith("caps") or where == "shared":
        return 4 if (j // 4) in under else 0
    return 5 if i.arity_bits else 7                                  # openings, points


def test_steered_form(ctx, oracle, case):
    c = case
    al, be, ix = _challenges(oracle, c, c.data())
    inputs = _inputs(c, steered=True)
    data, _, _, rows, clean = _members(c, inputs)
    K = len(rows) + len(clean)
    rep = lambda a: np.repeat(np.asarray(a)[None], K, axis=0)
    t0 = time.perf_counter()
    status, reasons = glp.fri_verify_queries_many(ctx, c.shapes, c.ranges, data["points"], *c.params, data["openings"], data["words"], rep(al[0]), rep(be[0]),
                                                  rep(ix[0]), caps=_caps(c, data), **c.geometry)
    device_s = time.perf_counter() - t0
    _assert_clean(status, reasons, clean)
    assert len(rows) == c.words.shape[1] + c.openings[0].size + sum(x[0].size for x in c.caps[1:]) + c.zs[0].size
    wrong, folds, held_by_none = [], {}, 0
    for k, (where, j) in zip(rows, inputs):
        want = _steered_expect(c, where, j, ix[0])
        got = 0 if status[k] == 0 else _check(reasons[k])
        held_by_none += want == 0
        if (got not in want if isinstance(want, tuple) else got != want) or (status[k] == 0) != (reasons[k] == ""):
            wrong.append((where, j, want, reasons[k]))
        if where == "words" and c.secs[c.sec_of[j]].kind in ps.QUERY_KINDS:
            sec = c.secs[c.sec_of[j]]
            if reasons[k] not in _allowed(sec) and not _keccak_byte(c, where, j):
                wrong.append((where, j, sec.name, reasons[k]))
            if got == 5:
                folds.setdefault(sec.name, []).append(j - sec.lo)
    assert wrong == [], "%d inputs with another verdict, the first: %s" % (len(wrong), wrong[:8])
    for sec in c.secs:
        if sec.kind == "evals":
            slot = folds.get(sec.name, [])
            assert len(slot) == 2 and slot[0] % 2 == 0 and slot[1] == slot[0] + 1, (sec.name, slot)
    # only the witness and cap digests no query lands under are held by no check
    i = c.inst0
    capn, under = 1 << i.cap_height, len({int(x) >> (i.lgN - i.cap_height) for x in ix[0]})
    assert held_by_none <= 1 + 4 * (capn - under) * (len(i.arity_bits) + len(c.caps) - 1)
    t0 = time.perf_counter()
    sample = _sample(c, inputs)
    for n in sample:
        k = rows[n]
        words, openings, caps, zs = _one(c, data, k)
        want = fr.verify_fri_proof(oracle, c.inst(0, zs), [caps[0]] + [x[0] for x in caps[1:]], openings[0], words[0], Fixed(al[0], be[0], ix[0]))
        got = 0 if status[k] == 0 else _check(reasons[k])
        assert got == want or _keccak_byte(c, *inputs[n]), (inputs[n], want, reasons[k])
    restated_s = time.perf_counter() - t0
    # the shared cap damages every member: a call of its own per word, three members each
    t0 = time.perf_counter()
    three = lambda a: np.repeat(np.asarray(a)[None], 3, axis=0)
    base = {"words": three(c.words[0]), "openings": three(c.openings[0]), "points": three(c.zs[0])}
    for o in range(1, len(c.caps)):
        base["caps%d" % o] = three(c.caps[o][0])
    for j in range(c.caps[0].size):
        shared = c.caps[0].copy()
        shared.reshape(-1)[j] = np.uint64(ps.bumped(shared.reshape(-1)[j]))
        status, reasons = glp.fri_verify_queries_many(ctx, c.shapes, c.ranges, base["points"], *c.params, base["openings"], base["words"], three(al[0]),
                                                      three(be[0]), three(ix[0]), caps=_caps(c, base, shared), **c.geometry)
        want = _steered_expect(c, "shared", j, ix[0])
        got = [0 if status[k] == 0 else _check(reasons[k]) for k in range(3)]
        assert got == [want] * 3, (j, want, reasons)
        if j in (0, c.caps[0].size - 1):
            words, openings, caps, zs = _one(c, base, 1, shared)
            assert want == fr.verify_fri_proof(oracle, c.inst(0, zs), [caps[0]] + [x[0] for x in caps[1:]], openings[0], words[0], Fixed(al[0], be[0], ix[0]))
    device_s += time.perf_counter() - t0
    print("\nSWEEP fri %-10s steered     inputs %4d  K %4d in one call + %d calls of 3 (shared cap)  device %.2f s  restatement %.2f s (%d inputs, s = %d)"
          % (c.label, len(inputs) + c.caps[0].size, K, c.caps[0].size, device_s, restated_s, len(sample), STRIDE))
