"""glp_witness_generate on the clock, beside the upload it replaces and the proof of the same witnesses in the same run.

    python -m plonky2_lib_amd.tools.witness_generate_timing [--out profiles/r23_witness_generate.txt] [--reps 7] [--log-n 20]
    (from the repository root: python plonky2-lib_amd/tools/witness_generate_timing.py)

Rows (include/glp.h, "witness generation, the dataflow half"):
  zkdsa at K = 256 and 2048   glp_witness_generate from 8 words per proof with ZERO_FIRST | glp_dev_upload of the same K complete
                              witnesses from pageable host memory | glp_prove_batch of them
  poseidon_chain_circuit(13)  K = 1 and 64: time per wave of a deep narrow plan (every wave walked)
  ecdsa_shape_circuit(log_n)  K = 1: wall time of glp_witness_plan_create (host planner) and generation
  GLP_WITNESS_NARROW_MAX      0, 64, 256, 1024, 4096, all walked: arith_circuit(12) at K = 1 and 64, zkdsa at K = 256
3 warm-up rounds, then --reps rounds with the compared calls alternating; median (min..max), host clock around call + synchronize.
The inputs of a circuit are one cell per copy class that some unit reads and no unit writes (the smallest position), found here with
numpy from the circuit description and the library's unit tables.  --resources FILE appends the kernels' register figures (the output
of hipcc -Rpass-analysis=kernel-resource-usage on csrc/witness.hip, which needs no GPU).
profiles/r23_witness_generate.txt is this tool's output annotated by hand: the "written by" and "reading" lines at its head and the
glp_witness_fill comparison at its end are not printed here.  The generate times include what the call does before its kernels: it
waits for the stream and copies the input values."""
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
ENV = "GLP_WITNESS_NARROW_MAX"
SWEEP = ("0", "64", "256", "1024", "4096", str(1 << 31))


def fmt(ts):
    return "%9.3f ms (%.3f..%.3f)" % (float(np.median(ts)), min(ts), max(ts))


def class_names(desc):
    """int64 [num_wires * n]: the smallest flat position of every cell's copy class, from the sigma values alone"""
    gl = synth.gl
    lg, nr, nw = int(desc.degree_bits), int(desc.num_routed_wires), int(desc.num_wires)
    n = 1 << lg
    table = gl.mul(np.asarray(desc.k_is, np.uint64)[:, None], gl.powers(gl.root_of_unity(lg), n)[None, :]).reshape(-1)
    order = np.argsort(table, kind="stable")
    nxt = order[np.searchsorted(table[order], np.asarray(desc.sigmas, np.uint64).reshape(-1))].astype(np.int64)
    name = np.minimum(np.arange(nr * n, dtype=np.int64), nxt)
    while True:                                   # pointer doubling along the cycles: name = the minimum over the next 2^t cells
        name2 = np.minimum(name, name[nxt])
        if (name2 == name).all():                 # no window's minimum grows by doubling: every window already spans its cycle's minimum
            break
        name, nxt = name2, nxt[nxt]
    return np.concatenate([name, np.arange(nr * n, nw * n, dtype=np.int64)])


def input_cells(gc, desc):
    cls = class_names(desc)
    n = 1 << int(desc.degree_bits)
    read, written = [], []
    for gi, g in enumerate(desc.gates):
        rows = np.nonzero(desc.constants[int(g["selector_index"])] == gi)[0].astype(np.int64)
        role = gc.witness_columns(gi)
        for want, into in ((2, read), (1, written)):
            cols = np.nonzero(role == want)[0].astype(np.int64)
            if len(rows) and len(cols):
                into.append(np.unique(cls[(cols[:, None] * n + rows[None, :]).reshape(-1)]))
    read = np.unique(np.concatenate(read)) if read else np.zeros(0, np.int64)
    written = np.unique(np.concatenate(written)) if written else np.zeros(0, np.int64)
    return np.setdiff1d(read, written).astype(np.uint64)


def say(msg):
    print("[witness_generate_timing] " + msg, file=sys.stderr, flush=True)


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


def zkdsa_batch(K, seed=9):
    rng = np.random.default_rng(seed)
    few = [synth.zkdsa_circuit(3, seed=5, private_key=synth.gl.rand(rng, 4), message=synth.gl.rand(rng, 4)) for _ in range(min(K, 64))]
    return [few[k % len(few)] for k in range(K)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=20, help="rows of the ecdsa-shape circuit = 2^log_n")
    ap.add_argument("--resources", default=None, help="text file appended as the kernel-resources section")
    a = ap.parse_args(argv)
    lines = ["glp_witness_generate beside the upload it replaces and the proof: %d warm-up rounds, %d timed, median (min..max)" % (WARM, a.reps), ""]
    os.environ.pop(ENV, None)
    with glp.Context(0) as ctx:
        # ---- zkdsa: generation from 8 words per proof against the upload of the complete witnesses
        for K in (256, 2048):
            say("zkdsa, K = %d" % K)
            descs = zkdsa_batch(K)
            gc = glp.Circuit(ctx, descs[0])
            cells = input_cells(gc, descs[0])
            plan = gc.witness_plan(cells)
            W = np.ascontiguousarray(np.stack([d.wires for d in descs]))
            vals = np.ascontiguousarray(np.stack([d.wires.reshape(-1)[cells.astype(np.int64)] for d in descs]))
            pis = np.ascontiguousarray(np.stack([np.asarray(d.public_inputs, np.uint64) for d in descs]))
            dev = ctx.dev_alloc(W.nbytes)
            out = np.empty((K, gc.proof_words), np.uint64)
            t = timed(ctx, {"gen": lambda: plan.generate(dev, vals, K, zero_first=True), "up": lambda: ctx.dev_upload(dev, W),
                            "prove": lambda: gc.prove_batch(W, pis, out=out)}, a.reps)
            plan.generate(dev, vals, K, zero_first=True)
            assert all(r.ok for r in gc.check_witness(dev_wires_ptr=dev, num_proofs=K, public_inputs=pis)), "generated zkdsa witnesses fail the check"
            info = plan.info
            lines.append("synth.zkdsa_circuit(3), K = %d: %d input words per proof, %d waves, %d units; a complete witness is %d words"
                         % (K, len(cells), info["num_waves"], info["num_units"], W[0].size))
            lines.append("  glp_witness_generate (ZERO_FIRST), wall    %s" % fmt(t["gen"]))
            lines.append("  glp_dev_upload of the K witnesses, pageable %s" % fmt(t["up"]))
            lines.append("  glp_prove_batch of them (host wires), wall  %s" % fmt(t["prove"]))
            lines.append("  generate / upload = %.3f; generate / prove = %.4f" % (np.median(t["gen"]) / np.median(t["up"]), np.median(t["gen"]) / np.median(t["prove"])))
            lines.append("")
            if K == 256:                           # the sweep's zkdsa row
                sweep_zk = {}
                for nm in SWEEP:
                    os.environ[ENV] = nm
                    p2 = gc.witness_plan(cells)
                    sweep_zk[nm] = timed(ctx, {"gen": lambda: p2.generate(dev, vals, K, zero_first=True)}, a.reps)["gen"]
                    p2.free()
                os.environ.pop(ENV, None)
            ctx.dev_free(dev)
            plan.free()
            gc.free()
        # ---- a deep narrow plan
        say("poseidon_chain_circuit(13)")
        desc = synth.poseidon_chain_circuit(13)
        gc = glp.Circuit(ctx, desc)
        cells = input_cells(gc, desc)
        plan = gc.witness_plan(cells)
        info = plan.info
        for K in (1, 64):
            vals = np.tile(desc.wires.reshape(-1)[cells.astype(np.int64)], (K, 1))
            dev = ctx.dev_alloc(K * desc.wires.nbytes)
            t = timed(ctx, {"gen": lambda: plan.generate(dev, vals, K, zero_first=True)}, a.reps)["gen"]
            reps = gc.check_witness(dev_wires_ptr=dev, num_proofs=K, public_inputs=np.tile(desc.public_inputs, (K, 1)))
            assert all(r.ok for r in (reps if K > 1 else [reps])), "generated Poseidon-chain witnesses fail the check"
            lines.append("synth.poseidon_chain_circuit(13), K = %d: %d waves, widest %d units, %d inputs: generate %s = %.3f us per wave"
                         % (K, info["num_waves"], info["widest_wave_units"], len(cells), fmt(t), 1e3 * np.median(t) / info["num_waves"]))
            ctx.dev_free(dev)
        lines.append("")
        plan.free()
        gc.free()
        # ---- the headline shape: the host planner's wall time, and generation
        say("ecdsa_shape_circuit(%d): building" % a.log_n)
        desc = synth.ecdsa_shape_circuit(a.log_n, seed=3)
        gc = glp.Circuit(ctx, desc)
        say("choosing the inputs")
        t0 = time.perf_counter()
        cells = input_cells(gc, desc)
        t1 = time.perf_counter()
        say("planning")
        plan = gc.witness_plan(cells)
        t2 = time.perf_counter()
        say("generating")
        info = plan.info
        vals = desc.wires.reshape(-1)[cells.astype(np.int64)][None, :]
        dev = ctx.dev_alloc(desc.wires.nbytes)
        W = np.ascontiguousarray(desc.wires)
        t = timed(ctx, {"gen": lambda: plan.generate(dev, vals, 1, zero_first=True), "up": lambda: ctx.dev_upload(dev, W)}, a.reps)
        plan.generate(dev, vals, 1, zero_first=True)
        assert gc.check_witness(dev_wires_ptr=dev).ok
        lines.append("synth.ecdsa_shape_circuit(%d), K = 1: 2^%d rows x %d wires, %d routed; %d inputs, %d units, %d waves (widest %d), %d copies, %d stuck"
                     % (a.log_n, a.log_n, desc.num_wires, desc.num_routed_wires, len(cells), info["num_units"], info["num_waves"],
                        info["widest_wave_units"], info["num_copies"], info["num_stuck_units"]))
        lines.append("  glp_witness_plan_create, wall (once; first call includes the sigma decode) %9.1f ms; choosing the inputs in numpy %.1f ms"
                     % (1e3 * (t2 - t1), 1e3 * (t1 - t0)))
        lines.append("  glp_witness_generate (ZERO_FIRST), wall    %s" % fmt(t["gen"]))
        lines.append("  glp_dev_upload of the witness, pageable     %s" % fmt(t["up"]))
        lines.append("")
        ctx.dev_free(dev)
        plan.free()
        gc.free()
        # ---- the threshold between walked and wide waves
        say("the sweep")
        desc = synth.arith_circuit(12)
        gc = glp.Circuit(ctx, desc)
        cells = input_cells(gc, desc)
        sweep = {}
        for K in (1, 64):
            vals = np.tile(desc.wires.reshape(-1)[cells.astype(np.int64)], (K, 1))
            dev = ctx.dev_alloc(K * desc.wires.nbytes)
            for nm in SWEEP:
                os.environ[ENV] = nm
                plan = gc.witness_plan(cells)
                sweep[(K, nm)] = timed(ctx, {"gen": lambda: plan.generate(dev, vals, K, zero_first=True)}, a.reps)["gen"]
                info = plan.info
                plan.free()
            ctx.dev_free(dev)
        os.environ.pop(ENV, None)
        gc.free()
        lines.append("GLP_WITNESS_NARROW_MAX sweep (a wave with more units than this is wide while K is below the CU count); arith_circuit(12): %d waves, widest %d units"
                     % (info["num_waves"], info["widest_wave_units"]))
        for nm in SWEEP:
            label = "all walked" if nm == SWEEP[-1] else nm
            lines.append("  %-10s  arith(12) K=1 %s | K=64 %s | zkdsa K=256 %s" % (label, fmt(sweep[(1, nm)]), fmt(sweep[(64, nm)]), fmt(sweep_zk[nm])))
        lines.append("")
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
