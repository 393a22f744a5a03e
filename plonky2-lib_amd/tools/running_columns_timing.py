"""The caller-defined running arguments on the clock: the stages gate_program.rows, running.terms and running.scan of
glp_gate_program_rows and glp_running_columns, beside the partial_products stage of glp_perm_zs_commit on a trace with as many
inverted elements per row.

    python -m plonky2_lib_amd.tools.running_columns_timing [--out profiles/r18_running_columns.txt] [--reps 15]
    (from the repository root: python plonky2-lib_amd/tools/running_columns_timing.py)

Two shapes: one proof of 2^20 rows, and 256 proofs of 2^10 rows in lock step; A = 2 arguments of T = 8 terms each, so 16 inverted
elements per row.  Everything is in HBM: the witness (A T columns per proof) is filled on the device, the rows program EMITs the 16
denominators col_t + gamma and then the 16 numerators beta col_t(next row) + gamma, and glp_running_columns reads them where they lie
(dens = rows_out, nums = rows_out + A T n, in_proof_stride = 2 A T n).  The comparison is glp_perm_zs_commit's perm.partial_products
stage with num_routed_wires = 16, chunk_size = 1 and one challenge: 16 inverted elements per row as well, one Fermat inversion per row
and the same three-step scan; its kernels (pp_kernels.inc) are the ones this stage had before the running columns existed.

Stage times are the library's own (glp_ctx_set_profiling: hipEvent pairs on the ctx stream around the launches of a stage); 3 warm-up
rounds of every call at every shape, then --reps rounds with the calls alternating inside a round; median (min..max).  Bytes are the
algorithmic ones the stage record carries: every input word read once and every output word written once."""
import argparse
import os
import sys

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import plonky2_lib_amd as glp                    # noqa: E402
from plonky2_lib_amd import gate_program as gp   # noqa: E402

A, T = 2, 8
WARM = 3


def rows_program():
    asm = gp.Assembler([A * T], num_params=2)
    F = gp.TraceField(asm)
    beta, gamma = asm.param(0), asm.param(1)
    for t in range(A * T):
        asm.emit(F.add(asm.col(0, t), gamma))
    for t in range(A * T):
        asm.emit(F.add(F.mul(beta, asm.col_next(0, t)), gamma))
    asm.end(asm.imm(1))
    return asm.assemble(hoist_emits=True)


def fmt(ts):
    return "%9.3f ms (%.3f..%.3f)" % (float(np.median(ts)), min(ts), max(ts))


def measure(ctx, K, log_n, reps, lines):
    n = 1 << log_n
    cols = A * T
    prog = ctx.gate_program(rows_program())
    witness = ctx.dev_alloc(8 * K * cols * n)
    ctx.fill_random_device(witness, K * cols * n, 21)
    terms = ctx.dev_alloc(8 * K * 2 * cols * n)
    out = ctx.dev_alloc(8 * K * A * (T + 1) * n)
    sigmas = ctx.dev_alloc(8 * cols * n)
    ctx.fill_random_device(sigmas, cols * n, 22)
    params = glp.splitmix_field(5, 2 * K).reshape(K, 2)
    chal = glp.splitmix_field(6, 2 * K).reshape(2, K, 1)
    perm = type("PermShape", (), dict(degree_bits=log_n, num_wires=cols, num_routed_wires=cols, num_challenges=1, quotient_degree_factor=1,
                                      k_is=np.array([pow(7, j, glp.P) for j in range(cols)], np.uint64)))
    cap_h = min(4, log_n + 1)
    names = ("gate_program.rows", "running.terms", "running.scan", "perm.partial_products")
    t = {(name, kind): [] for name in names for kind in (glp.RUN_SUM, glp.RUN_PRODUCT)}
    by = {}
    for i in range(WARM + reps):
        for kind in (glp.RUN_SUM, glp.RUN_PRODUCT):
            ctx.stage_reset()
            prog.rows([(K, cols, n)], params, in_dev_ptrs=[witness], out_dev_ptr=terms)
            _, totals = ctx.running_columns(kind, None, None, K, A, T, log_n, 2 * cols * n, nums_dev_ptr=terms + 8 * cols * n, dens_dev_ptr=terms,
                                            out_dev_ptr=out)
            zb = ctx.perm_zs_commit(perm, None, None, chal[0] if K > 1 else chal[0][0], chal[1] if K > 1 else chal[1][0], 1, cap_h,
                                    wires_dev_ptr=witness, sigmas_dev_ptr=sigmas)
            ctx.synchronize()
            st = ctx.stages()
            zb.free()
            if i >= WARM:
                for name in names:
                    t[(name, kind)].append(sum(ms for s, ms, _ in st if s == name))
                    by[name] = sum(b for s, _, b in st if s == name)
    elements = float(K) * n * A * T
    lines.append("K = %d proofs of 2^%d rows, A = %d arguments of T = %d terms (%d inverted elements per row, %.1f M in all)" %
                 (K, log_n, A, T, A * T, elements / 1e6))
    med = {}
    for kind, kname in ((glp.RUN_SUM, "GLP_RUN_SUM"), (glp.RUN_PRODUCT, "GLP_RUN_PRODUCT")):
        lines.append("  %s" % kname)
        for name in names:
            ts = t[(name, kind)]
            m = med[(name, kind)] = float(np.median(ts))
            lines.append("    %-24s %s  %8.1f MB algorithmic  %7.1f GB/s  %6.3f ns per inverted element" %
                         (name, fmt(ts), by[name] / 1e6, by[name] / m / 1e6, m * 1e6 / elements))
        ours = med[("running.terms", kind)] + med[("running.scan", kind)]
        ratio = ours / med[("perm.partial_products", kind)]
        lines.append("    running.terms + running.scan = %.3f ms: %.2fx perm.partial_products per inverted element%s" %
                     (ours, ratio, "  (MORE THAN TWICE: see the note on what bounds it)" if ratio > 2 else ""))
    ctx.synchronize()
    for p in (witness, terms, out, sigmas):
        ctx.dev_free(p)
    prog.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shapes", default="1x20,256x10", help="K x log_n, comma separated")
    a = ap.parse_args()
    ctx = glp.Context(a.device)
    ctx.set_profiling(True)
    lines = ["glp_gate_program_rows and glp_running_columns by stage (plonky2-lib_amd/tools/running_columns_timing.py); device time between the "
             "library's hipEvent pairs, median (min..max) of %d rounds after %d warm-up rounds, the calls alternating inside a round; every operand "
             "in HBM.  perm.partial_products: glp_perm_zs_commit with 16 routed wires, chunk_size 1, one challenge, on the same witness." % (a.reps, WARM), ""]
    for shape in a.shapes.split(","):
        K, log_n = (int(v) for v in shape.split("x"))
        measure(ctx, K, log_n, a.reps, lines)
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    ctx.set_profiling(False)
    ctx.close()


if __name__ == "__main__":
    main()
