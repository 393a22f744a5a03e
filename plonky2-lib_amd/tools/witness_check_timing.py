"""glp_witness_check on the clock, beside the proof of the same witnesses in the same run.

    python -m plonky2_lib_amd.tools.witness_check_timing [--out profiles/r19_witness_check.txt] [--reps 7] [--log-n 20] [--batch 256]
    (from the repository root: python plonky2-lib_amd/tools/witness_check_timing.py)

Two shapes: one witness of the headline circuit (synth.ecdsa_shape_circuit: 2^20 rows x 136 wires, 80 routed, the secp256k1 gate set)
in HBM, and --batch witnesses of the zkdsa circuit (2^3 rows x 135 wires) from host memory in one call.  Per shape the wall time of
glp_witness_check (host clock around the call: it ends with the copy of the reports, so it is synchronous), its three device stages
(glp_ctx_set_profiling: hipEvent pairs on the ctx stream) -- witness_check.sigma, the decode of the permutation, which only the first
check of a circuit runs (its time is that one call's); witness_check.gates, every gate on the rows of H; witness_check.copies, the
compare -- and the wall time of glp_prove_device / glp_prove_batch of the same inputs.  3 warm-up rounds, then --reps rounds with the
two calls alternating; median (min..max).  The sigma stage is the figure that decided that the decoded permutation is kept with the
circuit."""
import argparse
import os
import sys
import time

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import plonky2_lib_amd as glp                    # noqa: E402
from plonky2_lib_amd import synth                # noqa: E402

WARM = 3
STAGES = ("witness_check.sigma", "witness_check.gates", "witness_check.copies")


def fmt(ts):
    return "%9.3f ms (%.3f..%.3f)" % (float(np.median(ts)), min(ts), max(ts))


def measure(ctx, title, check, prove, reps, lines):
    t = {k: [] for k in STAGES + ("check", "prove")}
    first_sigma = None
    for i in range(WARM + reps):
        ctx.synchronize()
        ctx.set_profiling(True)
        ctx.stage_reset()
        t0 = time.perf_counter()
        reports = check()
        t1 = time.perf_counter()
        st = ctx.stages()
        ctx.set_profiling(False)
        assert all(r.ok for r in reports), "the timed witness does not satisfy its circuit: %s" % reports[0]
        t2 = time.perf_counter()
        prove()
        t3 = time.perf_counter()
        if i == 0:
            first_sigma = sum(ms for s, ms, _ in st if s == STAGES[0])
        if i >= WARM:
            for k in STAGES:
                t[k].append(sum(ms for s, ms, _ in st if s == k))
            t["check"].append(1e3 * (t1 - t0))
            t["prove"].append(1e3 * (t3 - t2))
    lines.append(title)
    lines.append("  glp_witness_check, wall        %s" % fmt(t["check"]))
    lines.append("    stage %-22s %9.3f ms, in the circuit's first check only" % (STAGES[0], first_sigma))
    for k in STAGES[1:]:
        lines.append("    stage %-22s %s" % (k, fmt(t[k])))
    lines.append("  proof of the same inputs, wall %s" % fmt(t["prove"]))
    lines.append("  check / proof = %.3f; first check (with the decode) / proof = %.3f"
                 % (np.median(t["check"]) / np.median(t["prove"]), (np.median(t["check"]) + first_sigma) / np.median(t["prove"])))
    lines.append("")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args(argv)
    lines = ["glp_witness_check beside the proof of the same witnesses: %d warm-up rounds, %d timed, median (min..max)" % (WARM, a.reps), ""]
    with glp.Context(0) as ctx:
        desc = synth.ecdsa_shape_circuit(a.log_n, seed=3)
        gc = glp.Circuit(ctx, desc)
        w = np.ascontiguousarray(desc.wires)
        dev = ctx.dev_alloc(w.nbytes)
        ctx.dev_upload(dev, w)
        measure(ctx, "synth.ecdsa_shape_circuit(%d): 2^%d rows x %d wires, %d routed, %d gates; one witness in HBM; proof = glp_prove_device"
                % (a.log_n, a.log_n, desc.num_wires, desc.num_routed_wires, len(desc.gates)),
                lambda: [gc.check_witness(dev_wires_ptr=dev)], lambda: gc.prove_device(dev), a.reps, lines)
        ctx.dev_free(dev)
        gc.free()
        rng = np.random.default_rng(9)
        descs = [synth.zkdsa_circuit(3, seed=5, private_key=synth.gl.rand(rng, 4), message=synth.gl.rand(rng, 4)) for _ in range(a.batch)]
        gc = glp.Circuit(ctx, descs[0])
        W = np.ascontiguousarray(np.stack([d.wires for d in descs]))
        pis = np.ascontiguousarray(np.stack([np.asarray(d.public_inputs, np.uint64) for d in descs]))
        out = np.empty((a.batch, gc.proof_words), np.uint64)
        measure(ctx, "synth.zkdsa_circuit(3): %d witnesses of 2^%d rows x %d wires from host memory in one call; proof = glp_prove_batch"
                % (a.batch, descs[0].degree_bits, descs[0].num_wires),
                lambda: gc.check_witness(W, pis), lambda: gc.prove_batch(W, pis, out=out), a.reps, lines)
        gc.free()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
