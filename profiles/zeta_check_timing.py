"""The vanishing identity at zeta of a caller-held circuit (glp_gate_program_eval_ext + glp_perm_check_zeta) beside the two things it
stands next to (profiles/r17_zeta_check.txt).

  python profiles/zeta_check_timing.py [--out profiles/r17_zeta_check.txt] [--batches 1 64 256 4096] [--reps 9]

Per circuit -- synth.arith_circuit and synth.ext_gates_circuit at 2^4 rows, two challenges -- one proof comes from glp_prove and is
taken K times: timing is data independent.  The gate program is traced from the gate bodies of tests/zeta_identity.py
(tests/gate_program_restate.py: trace_circuit); tests/test_gpu_zeta_check.py pins the calls word for word.
  new        eval_ext (gate sums to HBM) then perm_check_zeta (gate sums from HBM) on the host openings array of fri_verify_many: wall
             time of the two calls together, scan and upload of the openings included; and the device time of their two stages
  host       glp_verify_batch on the K proofs under GLP_BATCH_TRACE: the time its host threads spend on the same identity with the
             built-in gate bodies, "identity at zeta done at" minus "challenges back at"
  fri        glp_fri_verify_many on the proofs' plonk FRI instance (profiles/fri_verify_timing.py: fri_slice), wall time
Wall times: profiling off, host clock around calls that end synchronised (each copies its verdicts back); stage times: hipEvent pairs
with profiling on.  Median (min..max) of --reps rounds after two warm-up rounds, the three alternating within a round."""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import plonky2_lib_amd as glp                      # noqa: E402
import plonky2_lib_amd.synth as synth             # noqa: E402
import gate_program_restate as gr                  # noqa: E402
import zeta_identity as zi                         # noqa: E402
from fri_verify_timing import fri_slice, stage_ms  # noqa: E402
import fri_restate as fr                           # noqa: E402
from oracle import oracle                          # noqa: E402


def traced_stderr(fn):
    """fn() with the process's stderr going to a file: what the library printed there"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return tmp.read().decode()


def fmt(t):
    return "%.3f (%.3f..%.3f)" % (float(np.median(t)), min(t), max(t)) if t else "not measured"


def measure(ctx, what, desc, batches, reps, lines):
    gc = glp.Circuit(ctx, desc)
    proof = np.array(gc.prove(), np.uint64)
    digest = gc.digest()
    prog = gr.trace_circuit(desc)[0]
    g = ctx.gate_program(prog)
    inst, caps, pts, words, ch = fri_slice(desc, digest, gc.constants_sigmas_cap(), proof)
    state, pend = fr.challenger_state(ch)
    betas, gammas, alphas, zeta, pih = zi.challenges(desc, proof, digest)
    nch, qdf = int(desc.num_challenges), int(desc.quotient_degree_factor)
    lines.append("%s, 2^%d rows, %d wires (%d routed), %d challenges, %d query rounds; program: %d instructions, %d registers, max %d EMITs per gate; "
                 "%d openings, %d-word proofs" % (what, desc.degree_bits, desc.num_wires, desc.num_routed_wires, nch, desc.num_query_rounds, len(prog),
                                                  prog.num_regs, prog.max_constraints, len(pts), proof.size))
    lines.append("%6s | %-28s | %-28s | %-28s | %-28s | %-28s" % ("K", "new: two calls, wall ms", "gate_program.eval_ext stage", "perm.check_zeta stage",
                                                                "host identity in verify_batch", "fri_verify_many wall ms"))
    for K in batches:
        tile = lambda v: np.tile(np.asarray(v, np.uint64), (K,) + (1,) * np.ndim(v))      # noqa: E731
        proofs, openings = tile(proof), tile(pts)
        zetas, al, be, ga, ph = tile(zeta), tile(alphas), tile(betas), tile(gammas), tile(pih)
        parts = glp.plonk_ext_openings(desc, openings)
        dsum = ctx.dev_alloc(K * nch * 2 * 8)
        shapes = [(c, 0, int(o == 0)) for o, c in enumerate(inst.ncols)]
        ranges = [((0, 0), r) for _, r in inst.points]
        fargs = (ctx, shapes, ranges, tile(np.array([z for z, _ in inst.points], np.uint64)), inst.arity_bits, inst.pow_bits, inst.nq, openings, tile(words),
                 tile(state), tile(pend))
        fkw = dict(caps=[caps[0]] + [tile(c) for c in caps[1:]], log_n=inst.log_n, rate_bits=inst.rate_bits, cap_height=inst.cap_height, hasher=0)

        def new():
            g.eval_ext(zetas, parts["program"], al, ph, out_dev_ptr=dsum)
            status = ctx.perm_check_zeta(desc, qdf, zetas, parts["sigmas"], parts["wires"], parts["zs"], parts["zs_next"], parts["quotient"], be, ga, al,
                                         gate_sums_dev_ptr=dsum)
            assert not status.any()

        def fri():
            status, _ = glp.fri_verify_many(*fargs, **fkw)
            assert not status.any()

        def whole():
            assert gc.verify_batch(proofs).all()

        t = {k: [] for k in ("new", "eval", "perm", "host", "fri")}
        for profiling in (False, True):
            ctx.set_profiling(profiling)
            for i in range(reps + 2):
                ctx.stage_reset()
                t0 = time.perf_counter(); new(); w_new = (time.perf_counter() - t0) * 1e3      # noqa: E702
                s_eval, s_perm = stage_ms(ctx, "gate_program.eval_ext"), stage_ms(ctx, "perm.check_zeta")
                if profiling:
                    if i >= 2:
                        t["eval"].append(s_eval); t["perm"].append(s_perm)                   # noqa: E702
                    continue
                t0 = time.perf_counter(); fri(); w_fri = (time.perf_counter() - t0) * 1e3      # noqa: E702
                os.environ["GLP_BATCH_TRACE"] = "1"
                err = traced_stderr(whole)
                del os.environ["GLP_BATCH_TRACE"]
                m = re.search(r"challenges back at ([\d.]+) \| identity at zeta done at ([\d.]+)", err)
                if i >= 2:
                    t["new"].append(w_new); t["fri"].append(w_fri)                           # noqa: E702
                    if m:
                        t["host"].append(float(m.group(2)) - float(m.group(1)))
        ctx.set_profiling(False)
        ctx.dev_free(dsum)
        lines.append("%6d | %-28s | %-28s | %-28s | %-28s | %-28s" % (K, fmt(t["new"]), fmt(t["eval"]), fmt(t["perm"]), fmt(t["host"]), fmt(t["fri"])))
    g.free()
    gc.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 256, 4096])
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    oracle.build()
    ctx = glp.Context(0)
    lines = ["glp_gate_program_eval_ext + glp_perm_check_zeta on K proofs (profiles/zeta_check_timing.py), beside the host threads of glp_verify_batch on the "
             "same identity and glp_fri_verify_many on the same openings; median (min..max) of %d rounds after 2 warm-up rounds, ms" % a.reps]
    measure(ctx, "synth.arith_circuit", synth.arith_circuit(4), a.batches, a.reps, lines)
    measure(ctx, "synth.ext_gates_circuit", synth.ext_gates_circuit(4), a.batches, a.reps, lines)
    lines.append("The wall times include the Python binding's marshalling of the arrays; the host figure is the span between two marks of one "
                 "glp_verify_batch call, its host threads working beside the query-round kernel.")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
