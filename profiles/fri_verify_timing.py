"""The query-round kernel through its two entry points, glp_verify_batch and glp_fri_verify_many, on the same proofs.  Both launch
k_fri_verify_queries (csrc/verify_dev.h); profiles/r09_fri_verify.txt is the record from when glp_verify_batch still had a kernel of
its own (k_verify_queries), measured by this script as it was then.

  python profiles/fri_verify_timing.py [--out profiles/r09_fri_verify.txt] [--batches 32 256] [--reps 9]
  python profiles/fri_verify_timing.py --rehearse      # no GPU: the slicing alone, on the CPU prover's proof, held to the restatement

K proofs of the zkdsa circuit (`bench.py --workload zkdsa-batch`: 2^3 rows, standard_recursion_config) come from glp_prove_batch.
  whole:     glp_verify_batch on them (the plonk instance filled from the circuit's layout); the device time of its `verify_queries` stage
  seam:      the same proofs sliced into their plonk FRI instance -- four oracles (constants_sigmas shared, the other three per
             proof), zeta and g zeta, the openings in point order, the FriProof words, the transcript state right after the
             openings (tests/fri_restate.py: plonk_instance, plonk_openings_to_points) -- through glp_fri_verify_many; the device
             time of its `fri_verify_queries` stage and the wall time of the whole call
Every witness of the batch is the same one, so the K proofs are equal words; the kernel walks the same hash chains either way.
Stage times: hipEvent pairs with profiling on, median of --reps calls after two warm-up calls, the two verifiers alternating; wall
times: profiling off, host clock around the call (which ends synchronised: it copies the verdicts back)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonky2_lib_amd as glp                      # noqa: E402
import plonky2_lib_amd.synth as synth             # noqa: E402
import fri_restate as fr                           # noqa: E402
from oracle import oracle                          # noqa: E402


def fri_slice(desc, digest, cs_cap, proof, hasher=0):
    """(instance, caps of the four oracles, openings in point order, FriProof words, transcript right after the openings) of one proof"""
    capw, nch = 4 << desc.cap_height, desc.num_challenges
    caps = [np.asarray(cs_cap, np.uint64).reshape(-1, 4)] + [proof[k * capw:(k + 1) * capw].reshape(-1, 4) for k in range(3)]
    nopen = (desc.num_constants + desc.num_routed_wires + desc.num_wires + 2 * nch + nch * desc.num_partial_products + nch * desc.quotient_degree_factor)
    op = proof[3 * capw:3 * capw + 2 * nopen].reshape(-1, 2)
    ch = oracle.Challenger(hasher)
    ch.observe_hashes(np.asarray(digest, np.uint64))
    ch.observe(oracle.hash_no_pad(np.asarray(desc.public_inputs, np.uint64)))
    ch.observe_hashes(caps[1])
    ch.get_n(2 * nch)
    ch.observe_hashes(caps[2])
    ch.get_n(nch)
    ch.observe_hashes(caps[3])
    zeta = ch.get_ext()
    pts = fr.plonk_openings_to_points(desc, op)
    ch.observe(pts)
    inst = fr.plonk_instance(desc, zeta)
    start = 3 * capw + 2 * nopen
    words = proof[start:start + inst.layout()[5]].copy()
    assert start + words.size + len(desc.public_inputs) == proof.size
    return inst, caps, pts, words, ch


def stage_ms(ctx, name):
    return sum(ms for n, ms, _ in ctx.stages() if n == name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    oracle.build()
    desc = synth.zkdsa_circuit(3)
    if a.rehearse:
        oc = oracle.OracleCircuit(desc)
        rc, proof = oc.prove()
        assert rc == 0
        inst, caps, pts, words, ch = fri_slice(desc, desc.circuit_digest, oc.cs_cap, proof)
        assert fr.verify_fri_proof(oracle, inst, caps, pts, words, fr.challenger_clone(oracle, ch)) == 0
        print("rehearsal ok: the slice of the CPU prover's proof verifies under the restatement (%d FriProof words, %d openings)" % (words.size, len(pts)))
        return
    ctx = glp.Context(0)
    gc = glp.Circuit(ctx, desc)
    lines = ["glp_fri_verify_many against glp_verify_batch on the same K zkdsa proofs (2^3 rows, %d query rounds, arities %s, %d-word proofs); stage = device "
             "time between hipEvent pairs with profiling on, wall = host clock with profiling off; median (min..max) of %d calls after 2 warm-up calls, "
             "the two verifiers alternating" % (desc.num_query_rounds, list(desc.reduction_arity_bits), gc.proof_words, a.reps),
             "%6s | %-34s | %-34s | %6s | %-30s | %-30s" % ("K", "verify_queries stage ms", "fri_verify_queries stage ms", "ratio",
                                                          "glp_verify_batch wall ms", "glp_fri_verify_many wall ms")]
    for K in a.batches:
        proofs = gc.prove_batch(np.stack([desc.wires] * K), np.stack([desc.public_inputs] * K))
        inst, caps, pts, words, ch = fri_slice(desc, gc.digest(), gc.constants_sigmas_cap(), proofs[0])
        assert (proofs == proofs[0]).all()
        assert fr.verify_fri_proof(oracle, inst, caps, pts, words, fr.challenger_clone(oracle, ch)) == 0
        state, pend = fr.challenger_state(ch)
        shapes = [(c, 0, int(o == 0)) for o, c in enumerate(inst.ncols)]
        ranges = [((0, 0), r) for _, r in inst.points]
        zs = np.tile(np.array([z for z, _ in inst.points], np.uint64), (K, 1, 1))
        args = (ctx, shapes, ranges, zs, inst.arity_bits, inst.pow_bits, inst.nq, np.tile(pts, (K, 1, 1)), np.tile(words, (K, 1)), np.tile(state, (K, 1)),
                np.tile(pend, (K, 1)))
        kw = dict(caps=[caps[0]] + [np.tile(c, (K, 1, 1)) for c in caps[1:]], log_n=inst.log_n, rate_bits=inst.rate_bits, cap_height=inst.cap_height, hasher=0)

        def whole():
            assert gc.verify_batch(proofs).all()

        def seam():
            status, _ = glp.fri_verify_many(*args, **kw)
            assert not status.any()

        def timed(profiling, stage_a, stage_b):
            ctx.set_profiling(profiling)
            ta, tb = [], []
            for i in range(a.reps + 2):
                ctx.stage_reset(); t0 = time.perf_counter(); whole(); wa = (time.perf_counter() - t0) * 1e3; sa = stage_ms(ctx, stage_a)
                ctx.stage_reset(); t0 = time.perf_counter(); seam(); wb = (time.perf_counter() - t0) * 1e3; sb = stage_ms(ctx, stage_b)
                if i >= 2:
                    ta.append(sa if profiling else wa); tb.append(sb if profiling else wb)
            ctx.set_profiling(False)
            return ta, tb

        sa, sb = timed(True, "verify_queries", "fri_verify_queries")
        wa, wb = timed(False, "", "")
        fmt = lambda t: "%.3f (%.3f..%.3f)" % (float(np.median(t)), min(t), max(t))      # noqa: E731
        lines.append("%6d | %-34s | %-34s | %5.2fx | %-30s | %-30s" % (K, fmt(sa), fmt(sb), float(np.median(sb)) / float(np.median(sa)), fmt(wa), fmt(wb)))
    lines.append("The wall time of glp_fri_verify_many here includes the Python binding's marshalling of the arrays (a few array copies per call).")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    gc.free()
    ctx.close()


if __name__ == "__main__":
    main()
