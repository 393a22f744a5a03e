"""glp_witness_generate with random cells on the clock, beside the path it replaces: the same plan with the blinding cells listed as
inputs, their values drawn on the host and uploaded with the inputs.

    python -m plonky2_lib_amd.tools.witness_random_timing [--out profiles/r29_witness_random.txt] [--reps 5] [--ks 1,16,256]
    (from the repository root: python plonky2-lib_amd/tools/witness_random_timing.py)

The circuit is synth.zkdsa_circuit under Config.standard_recursion_zk_config (28 query rounds, 2^14 rows).  Rows:
  per K     glp_witness_generate (ZERO_FIRST) of the plan with random_cells = witness_random_cells, 8 input words per proof |
            glp_witness_generate of the plan that lists those cells as inputs, the values ready in host memory | the host-side draw of
            those values alone (synth.blinding_values: OS entropy reduced mod p) | glp_prove_batch of the generated witnesses
  kernels   k_witness_random alone: the stage time of a generation on a NoopGate circuit of the same shape whose plan holds nothing
            but the random cells (the stage also holds one empty walked-wave launch) | k_salt_lde of the wires commitment of the same
            proofs: the first `salt` stage of glp_prove_batch (stage events of the context)
3 warm-up rounds, then --reps rounds with the compared calls alternating; median (min..max), host clock around call + synchronize.
The generate times include what the call does before its kernels: it waits for the stream and copies the input values."""
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


def fmt(ts):
    return "%10.3f ms (%.3f..%.3f)" % (float(np.median(ts)), min(ts), max(ts))


def say(msg):
    print("[witness_random_timing] " + msg, file=sys.stderr, flush=True)


def timed(ctx, calls, reps):
    """calls: {name: thunk}; alternating, each followed by a synchronize -> {name: [ms]}"""
    t = {k: [] for k in calls}
    for i in range(WARM + reps):
        for k, fn in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if i >= WARM:
                t[k].append(1e3 * (time.perf_counter() - t0))
    return t


def stage_ms(ctx, fn, name, first_only=False):
    """the device time of the stages called `name` in one profiled call of fn"""
    ctx.set_profiling(True)
    ctx.stage_reset()
    fn()
    ctx.synchronize()
    ms = [m for nm, m, _ in ctx.stages() if nm == name]
    ctx.set_profiling(False)
    return ms[0] if first_only else sum(ms)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="1,16,256")
    a = ap.parse_args(argv)
    ks = [int(k) for k in a.ks.split(",")]
    os.environ.pop("GLP_WITNESS_NARROW_MAX", None)
    cfg = synth.Config.standard_recursion_zk_config()
    desc = synth.zkdsa_circuit(config=cfg)
    n, nw = 1 << int(desc.degree_bits), int(desc.num_wires)
    rnd = desc.witness_random_cells
    r, z, _ = synth.blinding_counts(cfg, 6)
    ins = np.array([c * n + row for row, cols in ((1, range(4)), (2, range(4, 8))) for c in cols], np.uint64)    # private key, message
    flat = desc.wires.reshape(-1)
    lines = ["glp_witness_generate with random cells beside the same cells as uploaded inputs: %d warm-up rounds, %d timed, median (min..max)" % (WARM, a.reps),
             "synth.zkdsa_circuit under standard_recursion_zk_config: 2^%d rows x %d wires, %d query rounds; blinding_counts: r = %d rows of random wires, "
             "z = %d copy-constrained pairs; %d random cells (r x %d + z x %d + %d PublicInputGate wires)"
             % (desc.degree_bits, nw, cfg.num_query_rounds, r, z, rnd.size, nw, cfg.num_routed_wires, nw - 4), ""]
    with glp.Context(0) as ctx:
        gc = glp.Circuit(ctx, desc)
        plan_r = gc.witness_plan(ins, random_cells=rnd)
        plan_i = gc.witness_plan(np.concatenate([ins, rnd]))
        assert plan_r.info == plan_i.info and plan_r.info["num_stuck_units"] == 0
        info = plan_r.info
        lines.append("the plan (either way): %d waves, %d units, %d copies, %d cells known of %d" % (info["num_waves"], info["num_units"], info["num_copies"],
                                                                                                   info["num_cells_known"], nw * n))
        noop = synth.Builder(synth.Config(nw, cfg.num_routed_wires), int(desc.degree_bits), seed=0, random_from_row=n).build()
        gn = glp.Circuit(ctx, noop)
        plan_n = gn.witness_plan([], random_cells=rnd)
        for K in ks:
            say("K = %d" % K)
            dev = ctx.dev_alloc(K * nw * n * 8)
            v8 = np.ascontiguousarray(np.tile(flat[ins.astype(np.int64)], (K, 1)))
            t0 = time.perf_counter()
            drawn = synth.blinding_values((K, rnd.size))
            say("  drew %d words in %.2f s" % (drawn.size, time.perf_counter() - t0))
            vall = np.ascontiguousarray(np.concatenate([v8, drawn], axis=1))
            pis = np.ascontiguousarray(np.tile(np.asarray(desc.public_inputs, np.uint64), (K, 1)))
            reps = a.reps if K < 256 else max(3, a.reps // 2)
            t = timed(ctx, {"rand": lambda: plan_r.generate(dev, v8, K, zero_first=True), "inputs": lambda: plan_i.generate(dev, vall, K, zero_first=True)}, reps)
            td = []
            for _ in range(3):
                t0 = time.perf_counter()
                synth.blinding_values((K, rnd.size))
                td.append(1e3 * (time.perf_counter() - t0))
            plan_r.generate(dev, v8, K, zero_first=True)
            assert all(rep.ok for rep in (lambda x: x if isinstance(x, list) else [x])(gc.check_witness(dev_wires_ptr=dev, num_proofs=K, public_inputs=pis))), \
                "generated zk witnesses fail the check"
            tp = timed(ctx, {"prove": lambda: gc.prove_batch_device(dev, K, pis)}, min(reps, 3))["prove"]
            salt = stage_ms(ctx, lambda: gc.prove_batch_device(dev, K, pis), "salt", first_only=True)
            kern = stage_ms(ctx, lambda: plan_n.generate(dev, np.zeros((K, 0), np.uint64), K), "witness_generate")
            gen_r = stage_ms(ctx, lambda: plan_r.generate(dev, v8, K, zero_first=True), "witness_generate")
            gen_i = stage_ms(ctx, lambda: plan_i.generate(dev, vall, K, zero_first=True), "witness_generate")
            perms_r, perms_s = K * ((rnd.size + 7) // 8), K * (n << int(desc.rate_bits))
            lines += ["", "K = %d" % K,
                      "  generate, random cells on the device: %d input words per proof          wall %s" % (ins.size, fmt(t["rand"])),
                      "  generate, those cells as inputs: %d input words per proof (%.1f MB uploaded) wall %s" % (ins.size + rnd.size, vall.nbytes / 1e6, fmt(t["inputs"])),
                      "  the host-side draw of those values alone (not in the line above)            wall %s" % fmt(td),
                      "  random / inputs = %.3f; random / (inputs + draw) = %.4f" % (np.median(t["rand"]) / np.median(t["inputs"]),
                                                                                      np.median(t["rand"]) / (np.median(t["inputs"]) + np.median(td))),
                      "  glp_prove_batch of the generated witnesses (wires on the device)            wall %s" % fmt(tp),
                      "  generate with random cells / prove = %.4f" % (np.median(t["rand"]) / np.median(tp)),
                      "  device time of the witness_generate stage: random cells %.3f ms, cells as inputs %.3f ms" % (gen_r, gen_i),
                      "  k_witness_random alone (+ one empty walked launch): %.3f ms for %d permutations = %.2f ns per permutation, %.1f GB/s of stores"
                      % (kern, perms_r, 1e6 * kern / perms_r, K * rnd.size * 8 / kern / 1e6),
                      "  k_salt_lde of the wires commitment of the same proofs: %.3f ms for %d permutations = %.2f ns per permutation"
                      % (salt, perms_s, 1e6 * salt / perms_s)]
            del drawn, vall
            ctx.dev_free(dev)
        plan_r.free(); plan_i.free(); plan_n.free()
        gc.free(); gn.free()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
