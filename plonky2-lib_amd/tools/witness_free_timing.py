"""glp_witness_generate with free units on the clock: a whole secp256k1 witness from the 40 words a caller sets per signature.

    python -m plonky2_lib_amd.tools.witness_free_timing [--out FILE] [--reps 5] [--big] [--resources FILE]
    (from the repository root: python plonky2-lib_amd/tools/witness_free_timing.py)

Rows (include/glp.h, "witness generation, the dataflow half", FREE UNITS):
  gadgets_ecdsa.ecdsa_circuit(random_signatures(1)), 2^17 rows        plan wall time, waves, widest wave, free units per kind;
                                                                      glp_witness_generate at K = 1 and K = 16; glp_prove_device
  --big: ecdsa_circuit(random_signatures(10), min_log_n=20), 2^20     the same at K = 1: the workload bench.py times
The inputs of a plan are the circuit's `witness_inputs` (40 words per signature) followed by `witness_zero_inputs` (cells of value 0 that
the unused operations of partly filled rows read).  2 warm-up rounds, then --reps timed; median (min..max), host clock around call +
synchronize; the generate times include the wait for the stream and the copy of the input values.  Every generated witness is checked
(glp_witness_check counts all zero) and compared with the builder's before anything is timed.  --resources FILE appends the kernels'
register figures (hipcc -Rpass-analysis=kernel-resource-usage on csrc/witness.hip, which needs no GPU)."""
import argparse
import os
import sys
import time

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import plonky2_lib_amd as glp                    # noqa: E402
from plonky2_lib_amd import gadgets_ecdsa as E   # noqa: E402

WARM = 2
KIND_NAMES = ("", "EQUALITY", "NONNATIVE_ADD", "NONNATIVE_MULTI_ADD", "NONNATIVE_SUB", "NONNATIVE_MUL", "NONNATIVE_INV", "BIGUINT_DIV_REM", "GLV_SECP256K1")


def fmt(ts):
    return "%9.3f ms (%.3f..%.3f)" % (float(np.median(ts)), min(ts), max(ts))


def say(msg):
    print("[witness_free_timing] " + msg, file=sys.stderr, flush=True)


def timed(ctx, fn, reps):
    out = []
    for i in range(WARM + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if i >= WARM:
            out.append(1e3 * (time.perf_counter() - t0))
    return out


def one_circuit(ctx, lines, label, c, Ks, reps):
    say(label + ": planning")
    gc = glp.Circuit(ctx, c)
    ins = np.concatenate([c.witness_inputs, c.witness_zero_inputs])
    t0 = time.perf_counter()
    plan = gc.witness_plan(ins, free_units=(c.free_units, c.free_cells), moduli=c.moduli)
    t_plan = 1e3 * (time.perf_counter() - t0)
    info, finfo = plan.info, plan.free_info
    kinds = np.bincount(c.free_units[:, 0], minlength=9)
    lines.append("%s: 2^%d rows x %d wires; %d input words (+ %d zero cells of unused operations)" % (label, int(c.degree_bits), int(c.num_wires), c.witness_inputs.size,
                                                                                               c.witness_zero_inputs.size))
    lines.append("  glp_witness_plan_create_ex, wall (once; includes the sigma decode) %9.1f ms" % t_plan)
    lines.append("  %d waves; %d gate units (widest wave %d, %d stuck), %d free units (widest wave %d, %d stuck), %d copies, %d of %d cells known"
                 % (info["num_waves"], info["num_units"], info["widest_wave_units"], info["num_stuck_units"], finfo["num_free_units"], finfo["widest_wave_free_units"],
                    finfo["num_stuck_free_units"], info["num_copies"], info["num_cells_known"], c.wires.size))
    lines.append("  free units per kind: " + ", ".join("%s %d" % (KIND_NAMES[k], kinds[k]) for k in range(1, 9) if kinds[k]))
    vals1 = c.wires.reshape(-1)[ins.astype(np.int64)]
    for K in Ks:
        say("%s: K = %d" % (label, K))
        vals = np.ascontiguousarray(np.tile(vals1, (K, 1)))
        dev = ctx.dev_alloc(K * c.wires.nbytes)
        plan.generate(dev, vals, K, zero_first=True)
        reps_ = gc.check_witness(dev_wires_ptr=dev, num_proofs=K, public_inputs=np.tile(c.public_inputs, (K, 1)))
        assert all(r.ok for r in (reps_ if K > 1 else [reps_])), "a generated witness fails the check"
        if K == 1:
            W = np.empty_like(c.wires)
            ctx.dev_download(dev, W)
            assert (W == c.wires).all(), "the generated witness is not the builder's"
        t = timed(ctx, lambda: plan.generate(dev, vals, K, zero_first=True), reps)
        lines.append("  glp_witness_generate (ZERO_FIRST), K = %-3d wall %s = %.3f us per wave, %.3f ms per witness"
                     % (K, fmt(t), 1e3 * np.median(t) / info["num_waves"], np.median(t) / K))
        if K == 1:
            tp = timed(ctx, lambda: gc.prove_device(dev), reps)
            lines.append("  glp_prove_device of that witness,          wall %s; generate / prove = %.2f" % (fmt(tp), np.median(t) / np.median(tp)))
            tu = timed(ctx, lambda: ctx.dev_upload(dev, c.wires), reps)
            lines.append("  glp_dev_upload of the complete witness,    wall %s" % fmt(tu))
        ctx.dev_free(dev)
    lines.append("")
    plan.free()
    gc.free()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", action="store_true", help="also the 10-signature circuit at 2^20 rows")
    ap.add_argument("--resources", default=None, help="text file appended as the kernel-resources section")
    a = ap.parse_args(argv)
    lines = ["glp_witness_generate with free units: %d warm-up rounds, %d timed, median (min..max)" % (WARM, a.reps), ""]
    os.environ.pop("GLP_WITNESS_NARROW_MAX", None)
    say("building the one-signature circuit")
    small = E.ecdsa_circuit(E.random_signatures(1))
    big = None
    if a.big:
        say("building the ten-signature circuit")
        big = E.ecdsa_circuit(E.random_signatures(10), min_log_n=20)
    with glp.Context(0) as ctx:
        one_circuit(ctx, lines, "ecdsa_circuit(random_signatures(1))", small, (1, 16), a.reps)
        if big is not None:
            one_circuit(ctx, lines, "ecdsa_circuit(random_signatures(10), min_log_n=20)", big, (1,), a.reps)
    if a.resources:
        lines.append("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
        lines += ["  " + s for s in open(a.resources).read().splitlines()]
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
