"""glp_witness_generate with unit programs on the clock: the reference's 16-level sparse-Merkle inclusion circuit from the words its
`set_witness` sets, against the upload of the complete witnesses.

    python -m plonky2_lib_amd.tools.witness_program_timing [--out FILE] [--reps 5]
    (from the repository root: python plonky2-lib_amd/tools/witness_program_timing.py)

Rows (include/glp.h, "witness generation, the dataflow half", UNIT PROGRAMS), for K = 1, 16 and 256 witnesses in lock step:
  glp_witness_plan_create_prog     wall time (once per circuit), waves, how many of them hold program units, units, copies
  glp_witness_generate             from `witness_inputs` + `witness_zero_inputs`, with and without the launch boundary of the program
                                   waves (the second figure comes from a plan of the same circuit whose split_le sums are inputs: no
                                   program units, every wave walked or wide by its size alone)
  glp_dev_upload                   of the K complete witnesses, pageable host memory, in the same run
2 warm-up rounds, then --reps timed; median (min..max), host clock around call + synchronize; the generate times include the wait for
the stream and the copy of the input values.  Every generated witness is checked (glp_witness_check counts all zero) and compared with
the builder's before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import plonky2_lib_amd as glp                    # noqa: E402
from plonky2_lib_amd import gadgets              # noqa: E402

WARM = 2
WGEN_PROGRAM = 9


def fmt(ts):
    return "%9.3f ms (%.3f..%.3f)" % (float(np.median(ts)), min(ts), max(ts))


def say(msg):
    print("[witness_program_timing] " + msg, file=sys.stderr, flush=True)


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--levels", type=int, default=16)
    a = ap.parse_args(argv)
    os.environ.pop("GLP_WITNESS_NARROW_MAX", None)
    tree = gadgets.SparseMerkleTree()
    for k, v in ((1, 2), (12, 1), (5, 51)):
        tree.insert(gadgets.hash_out_from_u128(k), gadgets.hash_out_from_u128(v))
    c = gadgets.smt_inclusion_circuit(tree, gadgets.hash_out_from_u128(5), n_levels=a.levels)
    n = 1 << int(c.degree_bits)
    lines = ["glp_witness_generate with unit programs: %d warm-up rounds, %d timed, median (min..max)" % (WARM, a.reps), ""]
    lines.append("smt_inclusion_circuit, %d levels: 2^%d rows x %d wires; %d input words (+ %d zero cells of unused operations); %d free units, %d of them program units of %d program(s)"
                 % (a.levels, int(c.degree_bits), int(c.num_wires), c.witness_inputs.size, c.witness_zero_inputs.size, c.free_units.shape[0],
                    int((c.free_units[:, 0] == WGEN_PROGRAM).sum()), len(c.witness_programs)))
    ins = np.concatenate([c.witness_inputs, c.witness_zero_inputs])
    # the same circuit without program units: their output cells (the sums of split_le) are inputs instead
    is_prog = c.free_units[:, 0] == WGEN_PROGRAM
    sums = np.concatenate([c.free_cells[int(r[2]) + int(r[3]):int(r[2]) + int(r[3]) + int(r[4])] for r in c.free_units[is_prog]])
    ins_np = np.concatenate([ins, sums])
    flat = c.wires.reshape(-1)
    with glp.Context(0) as ctx:
        gc = glp.Circuit(ctx, c)
        t_plan = []
        for i in range(3):
            t0 = time.perf_counter()
            plan = gc.witness_plan(ins, free_units=(c.free_units, c.free_cells), moduli=c.moduli, programs=c.witness_programs)
            t_plan.append(1e3 * (time.perf_counter() - t0))
            if i < 2:
                plan.free()
        plan_np = gc.witness_plan(ins_np, free_units=(c.free_units[~is_prog], c.free_cells), moduli=c.moduli)
        info, finfo = plan.info, plan.free_info
        assert info["num_stuck_units"] == 0 and finfo["num_stuck_free_units"] == 0 and plan_np.info["num_stuck_units"] == 0
        cw = plan.cell_waves().reshape(-1)
        prog_waves = sorted({int(cw[int(c.free_cells[int(r[2]) + int(r[3])])]) for r in c.free_units[is_prog]})
        lines.append("  glp_witness_plan_create_prog, wall (3 plans; the first includes the sigma decode) %s ms" % ", ".join("%.1f" % t for t in t_plan))
        lines.append("  %d waves, %d of them hold program units (waves %s); %d gate units (widest wave %d), %d free units (widest wave %d), %d copies, %d of %d cells known"
                     % (info["num_waves"], len(prog_waves), prog_waves, info["num_units"], info["widest_wave_units"], finfo["num_free_units"],
                        finfo["widest_wave_free_units"], info["num_copies"], info["num_cells_known"], c.wires.size))
        lines.append("  the plan without program units (their outputs given as inputs): %d waves" % plan_np.info["num_waves"])
        for K in (1, 16, 256):
            say("K = %d" % K)
            vals = np.ascontiguousarray(np.tile(flat[ins.astype(np.int64)], (K, 1)))
            vals_np = np.ascontiguousarray(np.tile(flat[ins_np.astype(np.int64)], (K, 1)))
            host = np.ascontiguousarray(np.tile(c.wires, (K, 1, 1)))
            dev = ctx.dev_alloc(host.nbytes)
            for p, v in ((plan, vals), (plan_np, vals_np)):
                plan_k = p
                plan_k.generate(dev, v, K, zero_first=True)
                reps_ = gc.check_witness(dev_wires_ptr=dev, num_proofs=K, public_inputs=np.tile(c.public_inputs, (K, 1)))
                assert all(r.ok for r in (reps_ if K > 1 else [reps_])), "a generated witness fails the check"
                W = np.empty_like(host)
                ctx.dev_download(dev, W)
                assert (W == host).all(), "a generated witness is not the builder's"
            t = timed(ctx, lambda: plan.generate(dev, vals, K, zero_first=True), a.reps)
            tn = timed(ctx, lambda: plan_np.generate(dev, vals_np, K, zero_first=True), a.reps)
            tu = timed(ctx, lambda: ctx.dev_upload(dev, host), a.reps)
            lines.append("  K = %-3d glp_witness_generate (ZERO_FIRST)            wall %s = %.3f ms per witness" % (K, fmt(t), np.median(t) / K))
            lines.append("          the same without program units               wall %s; the program waves cost %.3f ms" % (fmt(tn), np.median(t) - np.median(tn)))
            lines.append("          glp_dev_upload of the %3d complete witnesses  wall %s (%.1f MB); generate / upload = %.2f"
                         % (K, fmt(tu), host.nbytes / 1e6, np.median(t) / np.median(tu)))
            ctx.dev_free(dev)
        lines.append("")
        plan.free()
        plan_np.free()
        gc.free()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
