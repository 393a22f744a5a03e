"""Circuits and polynomials past the flush bounds of the carry-free accumulators (csrc/acc.h: an AccLimb holds ACC_MAX_TERMS = 1024
terms), where three prover kernels count terms and no other test reaches the count:

  k_final_values_small   never flushes; stage_fri_values takes it only while lane 0 of a point carries at most 1024 terms
                         (final_values_small_fits) and falls back to k_final_values past that
  k_final_values         flushes every 1024 opened columns
  k_open_dot             flushes every 1024 coefficients per lane: n / 8192 coefficients each, so from 2^23 coefficients on

Natural data wraps a 64-bit register only past about 4096 terms, so each kernel gets two kinds of shape: widths on the counting
boundary (which kernel runs; a flush neither drops nor double-counts a term) and widths well past it, where a missing flush or a
missing fallback gives a wrong proof with certainty.  The circuits are launch_matrix.WIDE_CASES; the HIP proof must equal the
oracle's word for word, section by section, and glp_verify, glp_verify_batch and the oracle verifier must accept it.  The same
circuits take k_tr_fri_alpha / k_open_reduce over thousands of openings, leaf hashes with more than 1000 absorptions, the verifiers'
16-lane Horner over a leaf of 10 000 words and the partial-product kernels with 250 chunks.  k_open_dot is reached through the FRI
seam with period-4 coefficients, whose opening has a closed form in Python integers (fri_restate.periodic_opening, pinned on the
CPU by test_fri_openings.py)."""
import time

import numpy as np
import pytest

import fri_restate as fr
import launch_matrix as lm
import plonky2_lib_amd as glp
import proof_sections as ps

pytestmark = pytest.mark.gpu

P = glp.P


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _host_verdict(gc, proof):
    """glp_verify's verdict and its reason ("" when accepted)"""
    ok = gc.verify(proof)
    return ok, "" if ok else glp.load_library().glp_last_error().decode()


def _parity(ctx, oracle, cid, batch=(), what=None):
    """prove on the GPU against the oracle's proof, all three verifiers; for each `host_transcript` flag in `batch` a
    glp_prove_batch of two whose members must be that proof.  Returns the live circuit, its description and the proof."""
    desc, oc, ref = lm.oracle_ref(oracle, cid)
    assert lm.BY_ID[cid].paths <= lm.launch_plan(desc)
    gc = glp.Circuit(ctx, desc)
    assert gc.proof_words == oc.proof_words == ps.total_words(ps.sections(desc))
    assert (gc.constants_sigmas_cap() == oc.cs_cap).all()
    t0 = time.time()
    got = gc.prove()
    print("WIDE %s: %d proof words, prove %.2f s" % (what or cid, got.size, time.time() - t0))
    lm.assert_sections_equal(got, ref, desc, "prove")
    assert gc.verify(got), glp.load_library().glp_last_error().decode()
    ok, why = gc.verify_batch(got[None, :], reasons=True)
    assert list(ok) == [True] and why == [""], why
    assert oc.verify(got) == 0
    for host in batch:
        proofs = lm.prove_batch(gc, desc, 2, host)
        for k in range(2):
            lm.assert_sections_equal(proofs[k], ref, desc, "prove_batch K=2 proof %d%s" % (k, " (host transcript)" if host else ""))
    return gc, desc, got


@pytest.mark.parametrize("lg,nw", [(lg, nw) for lg, nw, _ in lm.WIDE_WIDTHS], ids=[lm.wide_id(lg, nw) for lg, nw, _ in lm.WIDE_WIDTHS])
def test_wide_circuit_parity(ctx, oracle, lg, nw):
    """mixed(lg, [], nw=W) opens [83, W, 20, 16] columns.  The term count of the busiest lane is asserted from the description, so a
    change in synth's column counts fails here instead of moving the case off its boundary.  The two widths at 128 rows next to the
    bound also go through glp_prove_batch (K = 2, device and host transcripts): the batch takes the same kernel choice."""
    desc, _, _ = lm.oracle_ref(oracle, lm.wide_id(lg, nw))
    assert desc.degree_bits == lg and lm.opened_columns(desc) == [83, nw, 20, 16]
    lanes = 2 if lg == 7 else 1
    terms = sum(-(-c // lanes) for c in lm.opened_columns(desc))
    assert terms == lm.final_values_terms(desc) == lm.WIDE_TERMS[lg, nw]
    assert terms == {1928: 1024, 1929: 1025, 905: 1024, 906: 1025}.get(nw, terms)
    if nw in (10000, 6000):
        assert terms > 4400                      # every register of an unflushed accumulator has wrapped by then
    if nw == 2100:
        assert terms // lm.ACC_MAX_TERMS == 2 and terms % lm.ACC_MAX_TERMS
    gc, _, _ = _parity(ctx, oracle, lm.wide_id(lg, nw), batch=(False, True) if (lg, nw) in ((7, 1928), (7, 1929)) else ())
    gc.free()


def test_verify_batch_reasons_on_ten_thousand_wires(ctx, oracle):
    """(7, 10000): the untouched proof, one with the last wire opening incremented, one with the last column of the first query's
    wires leaf incremented (the end of the 16-lane Horner over 10 000 words and of a leaf hash of 1250 absorptions)"""
    cid = lm.wide_id(7, 10000)
    desc, oc, ref = lm.oracle_ref(oracle, cid)
    gc = glp.Circuit(ctx, desc)
    got = gc.prove()
    lm.assert_sections_equal(got, ref, desc, "prove")
    by = {s.name: s for s in ps.sections(desc)}
    cols = lm.opened_columns(desc)
    bad_open, bad_leaf = got.copy(), got.copy()
    at = by["openings"].lo + 2 * (cols[0] + cols[1] - 1)
    bad_open[at] = np.uint64(ps.bumped(bad_open[at]))
    leaf = by["q0_leaf1"]
    assert leaf.hi - leaf.lo == 10000
    bad_leaf[leaf.hi - 1] = np.uint64(ps.bumped(bad_leaf[leaf.hi - 1]))
    proofs = np.stack([got, bad_open, bad_leaf])
    ok, why = gc.verify_batch(proofs, reasons=True)
    for k in range(3):
        host_ok, host_why = _host_verdict(gc, proofs[k])
        assert bool(ok[k]) == host_ok and why[k] == host_why, (k, why[k], host_why)
        assert (oc.verify(proofs[k]) == 0) == host_ok
    assert list(ok) == [True, False, False]
    assert why[2] in ps.reasons(leaf)
    gc.free()


def test_wide_routed_circuit(ctx, oracle):
    """2000 routed wires: 249 partial products per challenge (the partial-product kernels with 250 chunks, 500 columns in the
    third oracle), 2003 sigma / constant columns; prove and prove_batch at K = 2 against the oracle"""
    desc, _, _ = lm.oracle_ref(oracle, "wide_routed_lg7")
    assert desc.num_partial_products == 249 and desc.degree_bits == 7
    assert lm.final_values_terms(desc) > lm.ACC_MAX_TERMS
    gc, _, _ = _parity(ctx, oracle, "wide_routed_lg7", batch=(False,))
    gc.free()


def test_arity_32(ctx, oracle):
    """arity_bits = 5, the largest glp_circuit_create takes and the only arity where a 16-lane group of k_fri_verify_queries takes two
    interpolation points per lane: parity, the three verifiers, and one damaged word of the layer's 64-word leaf rejected for the same
    reason by glp_verify and glp_verify_batch"""
    desc, oc, _ = lm.oracle_ref(oracle, "arity32_lg10")
    assert list(desc.reduction_arity_bits) == [5] and desc.num_query_rounds == 3
    gc, _, got = _parity(ctx, oracle, "arity32_lg10")
    by = {s.name: s for s in ps.sections(desc)}
    for q in range(3):
        sec = by["q%d_step0_evals" % q]
        assert sec.hi - sec.lo == 64
        # slot 3 (a lane's first point), slot 18 (its second) and the last word of the leaf, one per round
        bad = got.copy()
        at = sec.lo + (6, 37, 63)[q]
        bad[at] = np.uint64(ps.bumped(bad[at]))
        host_ok, host_why = _host_verdict(gc, bad)
        ok, why = gc.verify_batch(np.stack([got, bad]), reasons=True)
        assert list(ok) == [True, False] and not host_ok and why == ["", host_why], (q, why, host_why)
        assert host_why in ps.reasons(sec) and oc.verify(bad) != 0
    gc.free()


# ------------------------------------------------------------------ k_open_dot past its flush
# period-4 coefficients c_p = C[p mod 4]: near-maximal 22-bit limbs, p - 1, 1 and a fixed random value
OPEN_C = [0xFFFFFFFEFFFFFFFF, P - 1, 1, 0x9E3779B97F4A7C15 % P]
# With OPEN_C half of a lane's coefficients have a middle limb near 2^22, so 2048 unflushed terms fill a register to about
# 1024 * 2^22 * 2^31 + 512 * 2^21 * 2^31 = 0.63 * 2^64 (0.67 * 2^64 at most over the lanes walked on the CPU): the count is pinned, a wrap is
# not forced.  Four coefficients with that limb near 2^22 bring the expectation to 2048 * 2^22 * 2^31 = 2^64 in each of four registers
# per lane, and 8192 lanes are summed: without the flush some register wraps, with certainty (9 of 48 in the four lanes walked).
OPEN_C_HEAVY = [P - 2, P - 1, P - 3, P - 4]
OPEN_Z = (0x0123456789ABCDEF, 0xFEDCBA9876543210 % P)


@pytest.mark.parametrize("log_n,C", [(22, OPEN_C), (23, OPEN_C), (24, OPEN_C), (24, OPEN_C_HEAVY)], ids=["2^22", "2^23", "2^24", "2^24 heavy"])
def test_open_dot_past_its_flush(ctx, log_n, C):
    """one column of 2^log_n coefficients opened at OPEN_Z through glp_fri_open: a lane of k_open_dot takes n / 8192 of them, 512 at
    2^22 (no flush: the control), 1024 at 2^23 (the flush fires on the last one), 2048 at 2^24 (two flushes); then 2^24 of
    OPEN_C_HEAVY, where a missing flush wraps a register"""
    n = 1 << log_n
    assert n // (32 * 256) == {22: 512, 23: 1024, 24: 2048}[log_n]
    t0 = time.time()
    coeffs = np.tile(np.array(C, np.uint64), n // 4)[None, :]
    b = ctx.batch_from_coeffs(coeffs, rate_bits=1, cap_height=0)
    f = glp.FriOpenings(ctx, [b], [(OPEN_Z, [(0, 0, 1)])], [4] * 5, 0, 1)
    got = f.open()
    f.end()
    b.free()
    print("WIDE open 2^%d: %.2f s" % (log_n, time.time() - t0))
    assert got.shape == (1, 2) and (int(got[0, 0]), int(got[0, 1])) == fr.periodic_opening(C, log_n, OPEN_Z)
