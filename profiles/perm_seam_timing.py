"""glp_perm_zs_commit and glp_perm_quotient_values against the session's own permutation stages (profiles/r13_perm_seam.txt).

  python profiles/perm_seam_timing.py [--out profiles/r13_perm_seam.txt] [--log-n 20] [--batch 256] [--reps 9]

Baseline: a circuit of the shape's dimensions whose rows are all NoopGate (synth.Builder with nothing placed).  Its quotient stage is
the permutation terms alone: `quotient_eval` brackets k_l0_table + k_quotient<2, 0> and no light, limb or single-gate launch;
`partial_products` brackets the K5 kernels.  The seam runs over that session's own oracles (constants ++ sigmas at
sigma_col_begin = num_constants, wires, Z ++ partial products), everything in HBM: `perm.quotient_values` brackets k_l0_table +
k_perm_quotient, `perm.partial_products` the same K5 kernels.  Timing is data independent; the witness is random words.
Shapes: the headline (2^log_n rows, 136 wires / 80 routed, chunk 8, sub_bits 3, one proof) and the zkdsa batch (2^3 rows, 135 / 80,
K proofs in lock step).  The session has no K: at the batch shape the baseline is one session call on one proof, and the table also
gives the lock-step call against K such calls.
Stage times: hipEvent pairs with profiling on, median (min..max) of --reps rounds after two warm-up rounds, the two sides alternating
inside a round.  Before timing, the seam's values are committed with glp_batch_from_coset_values and held to the session's quotient
cap, and its Z commitment to the session's."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plonky2_lib_amd as glp                      # noqa: E402
import plonky2_lib_amd.synth as synth             # noqa: E402

P = glp.P


def stage_ms(ctx, name):
    return sum(ms for n, ms, _ in ctx.stages() if n == name)


def rand_field(seed, shape):
    return glp.splitmix_field(seed, int(np.prod(shape))).reshape(shape)


def fmt(t):
    return "%.3f (%.3f..%.3f)" % (float(np.median(t)), min(t), max(t))


def measure(ctx, cfg, log_n, K, reps, lines):
    desc = synth.Builder(cfg, log_n, seed=3, random_from_row=1 << log_n).build()       # every row a NoopGate, identity sigmas
    n, nw, nr, nch, nc = 1 << log_n, desc.num_wires, desc.num_routed_wires, desc.num_challenges, desc.num_constants
    rb, chh, sub_bits = desc.rate_bits, min(desc.cap_height, log_n + desc.rate_bits), desc.quotient_degree_factor.bit_length() - 1
    desc.cap_height = chh
    M = n << sub_bits
    gc = glp.Circuit(ctx, desc)
    wires, wires_b = ctx.dev_alloc(K * nw * n * 8), None
    if K == 1:
        ctx.fill_random_device(wires, nw * n, 77)
    else:                                               # small: the same words on the host for the many-proof wires oracle
        w_host = rand_field(77, (K, nw, n))
        ctx.dev_upload(wires, w_host)
        wires_b = ctx.batch_many_from_values(w_host, rb, chh)
    sigmas = ctx.dev_alloc(nr * n * 8)
    ctx.dev_upload(sigmas, desc.sigmas)
    chal = rand_field(5, (3, K, nch))
    gs_host = rand_field(6, (K, nch, M))
    gsum, out = ctx.dev_alloc(gs_host.nbytes), ctx.dev_alloc(gs_host.nbytes)
    ctx.dev_upload(gsum, gs_host)
    del gs_host
    one = lambda a: a[0] if K == 1 else a                                                # noqa: E731

    def session():
        s = glp.Session(gc, dev_wires_ptr=wires)                                         # proof 0 of the batch
        s.partial_products(chal[0, 0], chal[1, 0])
        return s

    def seam_zs():
        return ctx.perm_zs_commit(desc, None, None, one(chal[0]), one(chal[1]), rb, chh, wires_dev_ptr=wires, sigmas_dev_ptr=sigmas)

    def seam_q(cs, wb, zb, gate_sums):
        ctx.perm_quotient_values(desc, cs, nc, wb, zb, sub_bits, one(chal[0]), one(chal[1]), one(chal[2]),
                                 gate_sums_dev_ptr=gsum if gate_sums else None, out_dev_ptr=out)
        ctx.synchronize()

    # correctness at this size, once: the seam's Z commitment and its quotient are the session's
    s = session()
    zb = seam_zs()
    z0 = zb.member(0) if K > 1 else zb
    assert (z0.cap() == s.oracle(2).cap()).all(), "glp_perm_zs_commit differs from the session"
    wb0 = wires_b if K > 1 else s.oracle(1)
    seam_q(s.oracle(0), wb0, zb, False)
    s.quotient(chal[2, 0])
    qb = ctx.batch_from_coset_values(None, sub_bits, rb, chh, dev_ptr=out, shape=(nch, M))      # proof 0's values lead the buffer
    assert (qb.cap() == s.oracle(3).cap()).all(), "glp_perm_quotient_values differs from the session's quotient"
    qb.free(); zb.free(); s.end()

    ctx.set_profiling(True)
    t = {k: [] for k in ("pp", "spp", "q", "sq", "sqg")}
    for i in range(reps + 2):
        ctx.stage_reset()
        s = session()
        zb = seam_zs()
        wb = wires_b if K > 1 else s.oracle(1)
        seam_q(s.oracle(0), wb, zb, False)
        a = stage_ms(ctx, "perm.quotient_values")
        s.quotient(chal[2, 0])
        seam_q(s.oracle(0), wb, zb, True)
        b = stage_ms(ctx, "perm.quotient_values") - a
        if i >= 2:
            t["pp"].append(stage_ms(ctx, "partial_products")); t["spp"].append(stage_ms(ctx, "perm.partial_products"))
            t["q"].append(stage_ms(ctx, "quotient_eval")); t["sq"].append(a); t["sqg"].append(b)
        zb.free(); s.end()
    ctx.set_profiling(False)
    med = {k: float(np.median(v)) for k, v in t.items()}
    lines.append("2^%d rows, %d wires / %d routed, chunk %d, %d challenges, sub_bits %d, K = %d (the seam's %s)" %
                 (log_n, nw, nr, desc.quotient_degree_factor, nch, sub_bits, K, "one proof" if K == 1 else "lock-step batch; the session runs one proof"))
    lines.append("  %-58s %s ms" % ("session partial_products (K5 kernels, one proof)", fmt(t["pp"])))
    lines.append("  %-58s %s ms   %.2fx the session's call%s" % ("glp_perm_zs_commit perm.partial_products (K proofs)", fmt(t["spp"]), med["spp"] / med["pp"],
                                                                 "" if K == 1 else ", %.3fx %d of them" % (med["spp"] / (K * med["pp"]), K)))
    lines.append("  %-58s %s ms" % ("session quotient_eval (k_l0_table + k_quotient<2, 0>)", fmt(t["q"])))
    for key, what in (("sq", "gate_sums NULL"), ("sqg", "gate_sums in HBM")):
        lines.append("  %-58s %s ms   %.2fx the session's call%s" % ("glp_perm_quotient_values, " + what, fmt(t[key]), med[key] / med["q"],
                                                                     "" if K == 1 else ", %.3fx %d of them" % (med[key] / (K * med["q"]), K)))
    for p in (wires, sigmas, gsum, out):
        ctx.dev_free(p)
    if wires_b is not None:
        wires_b.free()
    gc.free()
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    ctx = glp.Context(0)
    lines = ["glp_perm_zs_commit / glp_perm_quotient_values against the stages of a session over an all-NoopGate circuit of the same dimensions "
             "(profiles/perm_seam_timing.py); device time between hipEvent pairs with profiling on, median (min..max) of %d rounds after 2 warm-up "
             "rounds, the two sides alternating; every operand in HBM" % a.reps]
    measure(ctx, synth.Config.standard_ecc_config(), a.log_n, 1, a.reps, lines)
    measure(ctx, synth.Config.standard_recursion_config(), 3, a.batch, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
