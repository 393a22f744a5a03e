"""glp_verify_batch swept word by word: member j of the batch is an accepted proof with word j replaced by itself + 1 mod p, for
EVERY word j of the proof, on the circuits at which k_fri_verify_queries branches.  The true verifier rejects each of them, for the
reason plonky2's order of checks dictates, and accepts the untouched copies that sit between them.

Where the words live and which reason each query-phase word must give comes from tests/proof_sections.py (pinned against the
oracle on the CPU by tests/test_proof_sections.py), never from the library.  Head words (caps, openings, layer caps, final
polynomial, witness, public inputs) move the transcript, so their expected reason is glp_verify's (host code), word by word; a
stride sample of the query words is held to glp_verify's string as well, and a thinner one to the oracle verifier's verdict.  The
device sweep itself is never thinned.

What a section pick (test_gpu_verify_batch.py::_tampered_batch) can miss and this cannot: a leaf's last partial sponge chunk or
its salts left out of the hash, a path one level short, a wrong sibling at one depth, the last column of a 16-lane stride dropped
from the alpha combination, rounds after the first checked less thoroughly.  (A cap entry compared on three of its four words is
out of reach here, since every cap word moves the transcript: the steered sweep of test_gpu_fri_verify_sweep.py sees that one.)

Each case prints one `SWEEP` line (words, launches, seconds on the device path, seconds of the host comparison): run with -s to
see them; profiles/r13_verify_sweep.txt keeps a set."""
import os
import time

import numpy as np
import pytest

import plonky2_lib_amd as glp
import plonky2_lib_amd.synth as synth
import proof_sections as ps

pytestmark = pytest.mark.gpu

RC = synth.Config.standard_recursion_config
SALT_SEED = [11, 22, 33, 44]
CHUNK = 2039                  # members per launch, at most 2048; odd, so the groups (members x query rounds) never fill the last workgroup
HOST_STRIDE = 31              # s: glp_verify is asked about the first and last word of each section of each round and every s-th word
ORACLE_EVERY = 8              # the oracle verifier about every 8th word of that sample


def _keccak(desc):
    desc.hasher, desc.circuit_digest = 1, None
    return desc


CASES = {
    # no reduction, depth-2 initial paths, 28 rounds
    "zkdsa": lambda: synth.zkdsa_circuit(3),
    # one arity-16 reduction: 16 evaluations on 16 lanes, a layer path
    "smt7": lambda: synth.smt_shape_circuit(7, seed=9),
    # two reductions: the second `within` from the shifted index, subgroup_x squared between the layers
    "smt10": lambda: synth.smt_shape_circuit(10, seed=9),
    # salted leaves of oracles 1..3 (leaf_len != oracle_cols).  A circuit that carries plonky2's blinding rows has at least 2^8 rows
    # (synth.blinding_counts); this one, the smallest of test_gpu_zk.py with more than one round, has 2^10 and two rounds
    "zk": lambda: synth.zkdsa_circuit(config=synth.Config.standard_recursion_zk_config(num_query_rounds=2), blinding_seed=7),
    # the Keccak leg of merkle_bad
    "keccak": lambda: _keccak(synth.zkdsa_circuit(3)),
    # cap_height = the depth of the initial trees: empty paths, the leaf digest compared with the cap directly
    "cap_is_depth": lambda: synth.zkdsa_circuit(3, config=RC(cap_height=6)),
    # arity 8: lanes 8..15 idle in the interpolation loop
    "arity8": lambda: synth.smt_shape_circuit(7, config=RC(arity_bits=3), seed=9),
}
WORDS = {"zkdsa": 8771, "smt7": 11735, "smt10": 14479}          # the lengths these circuits are known by


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    c.set_salt_seed(SALT_SEED)
    yield c
    for s in _cache.values():
        s.gc.free()
    _cache.clear()
    c.close()


def _chunks(words):
    for at in range(0, len(words), CHUNK - 3):
        yield words[at:at + CHUNK - 3]


def _device_sweep(gc, proof, words, value=None):
    """every word of `words` damaged in a member of its own (value None: w + 1 mod p), CHUNK members per launch, an untouched copy
    first, last and in the middle of every launch -> (ok [len(words)], reasons, launches, seconds).  The untouched copies are
    checked here: each accepted, with an empty reason."""
    ok, why, launches, t0 = [], [], 0, time.perf_counter()
    for part in _chunks(words):
        part = np.asarray(part)
        mid = 1 + len(part) // 2
        clean = [0, mid, len(part) + 2]
        if (len(part) + 3) % 2 == 0:
            clean.append(len(part) + 3)                   # an odd member count: idle groups in the last workgroup
        K = len(part) + len(clean)
        rows = np.setdiff1d(np.arange(K), clean)
        batch = np.tile(proof, (K, 1))
        batch[rows, part] = np.array([ps.bumped(proof[w]) if value is None else value for w in part], np.uint64)
        assert K <= 2048 and K % 16 != 0
        got_ok, got_why = gc.verify_batch(batch, reasons=True)
        launches += 1
        for k in clean:
            assert got_ok[k] and got_why[k] == "", ("an untouched member was rejected", k, K, got_why[k])
        ok += [bool(got_ok[k]) for k in rows]
        why += [got_why[k] for k in rows]
    return np.array(ok), why, launches, time.perf_counter() - t0


class Swept:
    pass


_cache = {}


def _sweep_of(ctx, name):
    """the whole-proof sweep of one case, run once and shared by the tests below"""
    if name not in _cache:
        s = Swept()
        s.name, s.desc = name, CASES[name]()
        s.gc = glp.Circuit(ctx, s.desc)
        s.proof = s.gc.prove()
        s.secs = ps.sections(s.desc)
        s.total = ps.total_words(s.secs)
        assert s.proof.size == s.total and ps.tiles(s.secs, s.total)
        assert s.gc.verify(s.proof)
        s.sec_of = ps.section_of(s.secs)
        s.ok, s.why, s.launches, s.device_s = _device_sweep(s.gc, s.proof, np.arange(s.total))
        s.keccak = int(getattr(s.desc, "hasher", 0)) == 1
        _cache[name] = s
    return _cache[name]


@pytest.fixture(params=list(CASES))
def swept(request, ctx):
    return _sweep_of(ctx, request.param)


def _expected_query_reasons(s, at):
    """the reasons the map allows for word `at` damaged alone; under KeccakHash<25> the fourth word of a digest holds one byte, and a
    larger value is refused before any hashing (include/glp.h, GLP_HASH_KECCAK25)"""
    sec = s.secs[s.sec_of[at]]
    if s.keccak and sec.kind in ps.DIGEST_KINDS and (at - sec.lo) % 4 == 3 and ps.bumped(s.proof[at]) > 0xFF:
        return ("digest at word %d is longer than 25 bytes" % (at - 3),)
    return ps.reasons(sec)


def test_circuits_are_the_ones_meant(swept):
    s, d = swept, swept.desc
    if s.name in WORDS:
        assert s.total == WORDS[s.name]
    depth0 = d.degree_bits + d.rate_bits - d.cap_height
    want = {"zkdsa": ([], 2), "smt7": ([4], 6), "smt10": ([4, 4], 9), "zk": ([4, 4], 9), "keccak": ([], 2), "cap_is_depth": ([], 0), "arity8": ([3], 6)}[s.name]
    assert (list(d.reduction_arity_bits), depth0) == want
    assert any(x.kind == "salt" for x in s.secs) == (s.name == "zk") == s.gc.zero_knowledge
    assert len(s.ok) == len(s.why) == s.total                       # members swept = words in the map


def test_every_damaged_member_is_rejected(swept):
    s = swept
    accepted = [(at, s.secs[s.sec_of[at]].name) for at in np.nonzero(s.ok)[0]]
    assert accepted == [], "%d damaged members accepted, the first: %s" % (len(accepted), accepted[:8])
    assert all(s.why)


def test_query_words_give_the_reason_the_check_order_dictates(swept):
    s = swept
    wrong, folds = [], {}
    for at in range(s.total):
        sec = s.secs[s.sec_of[at]]
        if sec.kind not in ps.QUERY_KINDS:
            continue
        if s.why[at] not in _expected_query_reasons(s, at):
            wrong.append((at, sec.name, s.why[at]))
        if sec.kind == "evals" and s.why[at] == ps.fold_reason(sec):
            folds.setdefault(sec.name, []).append(at - sec.lo)
    assert wrong == [], "%d query words with another reason, the first: %s" % (len(wrong), wrong[:8])
    # exactly the two coordinates of one evaluation give the consistency reason: the slot x_index & (arity - 1)
    evals = [x for x in s.secs if x.kind == "evals"]
    assert len(evals) == s.desc.num_query_rounds * len(s.desc.reduction_arity_bits)
    for sec in evals:
        slot = folds.get(sec.name, [])
        assert len(slot) == 2 and slot[0] % 2 == 0 and slot[1] == slot[0] + 1, (sec.name, slot)


def test_reasons_equal_the_host_verifier_and_verdicts_the_oracle(swept, oracle):
    s = swept
    L = glp.load_library()
    head = [at for at in range(s.total) if s.secs[s.sec_of[at]].kind not in ps.QUERY_KINDS]
    words = sorted(set(head) | set(ps.sample(s.secs, HOST_STRIDE, ps.QUERY_KINDS)))
    oc = None if s.gc.zero_knowledge else oracle.OracleCircuit(s.desc)         # the oracle has no salted layout
    assert oc is None or oc.verify(s.proof) == 0
    t0 = time.perf_counter()
    differ, oracle_accepts = [], []
    for i, at in enumerate(words):
        bad = s.proof.copy()
        bad[at] = np.uint64(ps.bumped(bad[at]))
        host_ok = s.gc.verify(bad)
        host_why = "" if host_ok else L.glp_last_error().decode()
        if host_ok != s.ok[at] or host_why != s.why[at]:
            differ.append((at, s.secs[s.sec_of[at]].name, s.why[at], host_why))
        if oc is not None and i % ORACLE_EVERY == 0 and oc.verify(bad) == 0:
            oracle_accepts.append(at)
    host_s = time.perf_counter() - t0
    print("\nSWEEP %-12s words %5d  launches %2d of <= %d members  device %.2f s  host comparison %.2f s (%d words, s = %d)"
          % (s.name, s.total, s.launches, CHUNK, s.device_s, host_s, len(words), HOST_STRIDE))
    assert differ == [], "%d words where glp_verify_batch and glp_verify differ, the first: %s" % (len(differ), differ[:6])
    assert oracle_accepts == []


def test_a_word_set_to_p_is_named(swept):
    """the canonical-form check comes first and names the word; a KeccakHash<25> digest is bytes, not field elements, so its words
    are left out here (the sweep above covers them)"""
    s = swept
    kinds = [k for k in sorted({x.kind for x in s.secs}) if not (s.keccak and k in ps.DIGEST_KINDS)]
    words = ps.sample(s.secs, HOST_STRIDE, kinds)
    ok, why, _, _ = _device_sweep(s.gc, s.proof, words, value=ps.P)
    assert not ok.any()
    wrong = [(at, r) for at, r in zip(words, why) if r != "proof word %d is not a canonical field element" % at]
    assert wrong == [], wrong[:8]


def test_host_transcript_gives_the_same_sweep(ctx):
    """GLP_VERIFY_HOST_TRANSCRIPT=1 keeps the K transcripts on host threads: the zkdsa sweep again, same verdicts, same reasons"""
    s = _sweep_of(ctx, "zkdsa")
    os.environ["GLP_VERIFY_HOST_TRANSCRIPT"] = "1"
    try:
        ok, why, _, _ = _device_sweep(s.gc, s.proof, np.arange(s.total))
    finally:
        del os.environ["GLP_VERIFY_HOST_TRANSCRIPT"]
    assert (ok == s.ok).all() and why == s.why
