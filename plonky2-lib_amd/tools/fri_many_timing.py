"""glp_fri_prove_many against the loop of glp_fri_prove calls it replaces, at the shape of the zkdsa circuit.

    python -m plonky2_lib_amd.tools.fri_many_timing [--out profiles/r08_fri_many.txt] [--batches 32 64 256] [--reps 7]
    (from the repository root: python plonky2-lib_amd/tools/fri_many_timing.py)

The instance has the column counts, log_n and FRI parameters of the circuit `bench.py --workload zkdsa-batch` proves (synth.zkdsa_circuit:
2^3 rows, standard_recursion_config) under plonky2's plonk instance -- zeta opens the four oracles in full, g zeta the Z columns -- with
random polynomials: oracle 0 (constants and sigmas) is one batch shared by all proofs, oracles 1..3 are many-proof batches.  For K in
--batches it times
    many:  one glp_fri_prove_many call over the K proofs
    loop:  K glp_fri_prove calls on glp_batch_member views of the same batches (all the library offered before the many form)
on the same sponge states, checks once that both give the same words, and reports the median and the spread of --reps repetitions,
the two alternating, after two warm-up rounds of each (the first is the check).  Wall clock around the C calls only -- descriptors,
ctypes arguments and output arrays are built before the timed window, so neither side pays Python marshalling per call -- and every
call ends synchronised (it copies its proofs back).
With profiling on (a run of its own, after the timed one) it adds the per-stage device times of both."""
import argparse
import os
import sys
import time

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import plonky2_lib_amd as glp                    # noqa: E402
import plonky2_lib_amd.synth as synth            # noqa: E402
from plonky2_lib_amd import binding              # noqa: E402


def instance():
    """(ncols per oracle, ranges per point, FRI parameters) of the zkdsa circuit's plonk instance"""
    d = synth.zkdsa_circuit(3, seed=5)
    nch = int(d.num_challenges)
    ncols = [int(d.num_constants) + int(d.num_routed_wires), int(d.num_wires), nch * (1 + int(d.num_partial_products)),
             nch * int(d.quotient_degree_factor)]
    ranges = [[(o, 0, ncols[o]) for o in range(4)], [(2, 0, nch)]]
    return d, ncols, ranges


def stage_table(ctx):
    agg = {}
    for name, ms, _ in ctx.stages():
        agg[name] = agg.get(name, 0.0) + ms
    return agg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 64, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    d, ncols, ranges = instance()
    lg, rb, cap = int(d.degree_bits), int(d.rate_bits), int(d.cap_height)
    params = (list(d.reduction_arity_bits), int(d.proof_of_work_bits), int(d.num_query_rounds))
    n = 1 << lg
    wn = pow(1753635133440165772, 1 << (32 - lg), glp.P)
    ctx = glp.Context(a.device)
    lines = ["glp_fri_prove_many against K glp_fri_prove calls on member views; zkdsa shape: 2^%d rows, columns %s, rate_bits %d, cap_height %d, "
             "arities %s, %d proof-of-work bits, %d query rounds; median of %d repetitions, the two alternating, after 2 warm-up rounds of each "
             "(the first is also the check that both give the same words); wall clock around the C calls alone: descriptors, argument "
             "marshalling and output buffers are made before the timed window" %
             (lg, ncols, rb, cap, params[0], params[1], params[2], a.reps),
             "%6s %12s %12s %12s %12s %8s" % ("K", "many ms", "(min..max)", "loop ms", "(min..max)", "ratio")]
    breakdown = []
    rng = np.random.default_rng(1)
    field = lambda shape: glp.splitmix_field(int(rng.integers(1 << 62)), int(np.prod(shape))).reshape(shape)      # noqa: E731
    shared = ctx.batch_from_coeffs(field((ncols[0], n)), rb, cap)
    for K in a.batches:
        many = [shared] + [ctx.batch_many_from_coeffs(field((K, c, n)), rb, cap) for c in ncols[1:]]
        views = [[shared] + [b.member(k) for b in many[1:]] for k in range(K)]
        zs = np.zeros((K, 2, 2), np.uint64)
        zs[:, 0] = field((K, 2))
        for k in range(K):                                           # g zeta: the extension element scaled by the base-field root
            zs[k, 1] = [int(zs[k, 0, 0]) * wn % glp.P, int(zs[k, 0, 1]) * wn % glp.P]
        points = [[((int(zs[k, b, 0]), int(zs[k, b, 1])), ranges[b]) for b in range(2)] for k in range(K)]
        st, pend = field((K, 12)), field((K, 3))

        # descriptors, argument marshalling and output buffers are made once, outside the timed calls: what is timed is the library
        # (one C call for the many form, K C calls for the loop), as a C or Rust integrator would drive it
        L, C, bd = glp.load_library(), binding.C, binding
        nopen = sum(nc for r in ranges for _, _, nc in r)
        words = glp.fri_proof_words(views[0], *params[::2])
        dm, keep_m = bd._fri_desc_to_c(many, points[0], *params)
        ops, proofs = np.zeros((K, nopen, 2), np.uint64), np.zeros((K, words), np.uint64)
        args_m = (ctx._h, C.byref(dm), K, bd._p(zs), bd._p(st), bd._p(pend), pend.shape[1], bd._p(ops), bd._p(proofs))
        sop, sproofs = np.zeros((K, nopen, 2), np.uint64), np.zeros((K, words), np.uint64)
        descs = [bd._fri_desc_to_c(views[k], points[k], *params) for k in range(K)]
        args_l = [(ctx._h, C.byref(descs[k][0]), bd._p(st[k]), bd._p(pend[k]), pend.shape[1], bd._p(sop[k]), bd._p(sproofs[k])) for k in range(K)]

        def run_many():
            bd._chk(L.glp_fri_prove_many(*args_m))

        def run_loop():
            for ak in args_l:
                bd._chk(L.glp_fri_prove(*ak))

        run_many(); run_loop()                                       # first warm-up round, and the check that both give the same words
        assert (ops == sop).all() and (proofs == sproofs).all(), "the two forms differ at K = %d" % K
        assert proofs.any() and ops.any()
        run_many(); run_loop()
        tm, tl = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); run_many(); t1 = time.perf_counter(); run_loop(); t2 = time.perf_counter()
            tm.append((t1 - t0) * 1e3); tl.append((t2 - t1) * 1e3)
        med_m, med_l = float(np.median(tm)), float(np.median(tl))
        lines.append("%6d %12.3f %12s %12.3f %12s %7.1fx" % (K, med_m, "%.2f..%.2f" % (min(tm), max(tm)), med_l,
                                                             "%.2f..%.2f" % (min(tl), max(tl)), med_l / med_m))
        # per-stage device time (hipEvent pairs; profiling synchronises per stage, so this run is not the timed one)
        ctx.set_profiling(True)
        ctx.stage_reset(); t0 = time.perf_counter(); run_many(); wall_m = (time.perf_counter() - t0) * 1e3; sm = stage_table(ctx)
        ctx.stage_reset(); t0 = time.perf_counter(); run_loop(); wall_l = (time.perf_counter() - t0) * 1e3; sl = stage_table(ctx)
        ctx.set_profiling(False)
        breakdown.append("K = %d, profiling on: many %.3f ms wall, %.3f ms in device stages; loop %.3f ms wall, %.3f ms in device stages" %
                         (K, wall_m, sum(sm.values()), wall_l, sum(sl.values())))
        for name in sorted(set(sm) | set(sl)):
            breakdown.append("    %-16s many %9.3f ms   loop %9.3f ms" % (name, sm.get(name, 0.0), sl.get(name, 0.0)))
        del views
        for b in many[1:]:
            b.free()
    lines += ["", "Per-stage breakdown (device time between hipEvent pairs; wall minus device stages = host: transcripts, launches, copies)"] + breakdown
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    shared.free()
    ctx.close()


if __name__ == "__main__":
    main()
