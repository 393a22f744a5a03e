"""GLP_GATE_PROGRAM inside a glp_circuit against the built-in gate bodies of the same circuit (profiles/r27_circuit_programs.txt).

  python profiles/circuit_program_timing.py [--out profiles/r27_circuit_programs.txt] [--log-n 16 20] [--reps 9]

The twin of a circuit gives every gate that has constraints type 23, its program traced from the gate bodies of
profiles/gate_program_timing.py (one program per gate, closed with END IMM(1): the selector filter is the library's).  Measured: a
session's `quotient_eval` stage on the circuit, on its twin and on a circuit of the same dimensions whose rows are all NoopGate; the
gate cost of either is its stage minus the NoopGate one.  The twin's stage holds the same permutation launch and one
k_quotient_gate_program launch per gate.  Two challenges, quotient_degree_factor 8, everything in HBM; timing is data independent.
Stage times: hipEvent pairs with profiling on, median (min..max) of --reps rounds after two warm-up rounds."""
import argparse
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plonky2_lib_amd as glp                      # noqa: E402
import plonky2_lib_amd.synth as synth             # noqa: E402
from plonky2_lib_amd import gate_program as gp    # noqa: E402
from gate_program_timing import gate_constraints, stage_ms, fmt, _config_of      # noqa: E402


def twin(desc):
    nsel, nc, nw = int(desc.num_selectors), int(desc.num_constants), int(desc.num_wires)
    d2 = copy.copy(desc)
    d2.gates = [dict(g) for g in desc.gates]
    programs = []
    for g in d2.gates:
        if not int(g["num_constraints"]):
            continue
        asm = gp.Assembler([nc, nw], num_params=4)
        F = gp.TraceField(asm)
        for v in gate_constraints(F, g, [asm.col(0, j) for j in range(nsel, nc)], [asm.col(1, j) for j in range(nw)], [asm.param(j) for j in range(4)]):
            asm.emit(v)
        asm.end(asm.imm(1))
        g.update(type=glp.GATE_PROGRAM, p0=len(programs), p1=0)
        programs.append(asm.assemble(hoist_emits=True, sink_single_use=True))
    return d2, programs


def measure(ctx, what, desc, log_n, reps, lines):
    n, nw, nch = 1 << log_n, int(desc.num_wires), int(desc.num_challenges)
    desc.cap_height = min(int(desc.cap_height), log_n + int(desc.rate_bits))
    noop = synth.Builder(_config_of(desc), log_n, seed=3, random_from_row=n).build()
    noop.cap_height = desc.cap_height
    d2, programs = twin(desc)
    circuits = {"gates": glp.Circuit(ctx, desc), "twin": glp.Circuit(ctx, d2, programs=programs), "noop": glp.Circuit(ctx, noop)}
    wires = ctx.dev_alloc(nw * n * 8)
    ctx.fill_random_device(wires, nw * n, 77)
    chal = glp.splitmix_field(5, 3 * nch).reshape(3, nch)
    ctx.set_profiling(True)
    t = {k: [] for k in circuits}
    for i in range(reps + 2):
        for k, c in circuits.items():
            ctx.stage_reset()
            s = glp.Session(c, dev_wires_ptr=wires)
            s.partial_products(chal[0], chal[1])
            s.quotient(chal[2])
            if i >= 2:
                t[k].append(stage_ms(ctx, "quotient_eval"))
            s.end()
    ctx.set_profiling(False)
    med = {k: float(np.median(v)) for k, v in t.items()}
    built_in, prog = med["gates"] - med["noop"], med["twin"] - med["noop"]
    lines.append("%s, 2^%d rows, %d wires, %d program gates: %s instructions, %s registers, %s EMITs" %
                 (what, log_n, nw, len(programs), "+".join(str(len(p)) for p in programs), "/".join(str(p.num_regs) for p in programs),
                  "+".join(str(p.max_constraints) for p in programs)))
    lines.append("  %-66s %s ms" % ("session quotient_eval, built-in gates", fmt(t["gates"])))
    lines.append("  %-66s %s ms" % ("session quotient_eval, the twin (every gate a program)", fmt(t["twin"])))
    lines.append("  %-66s %s ms" % ("session quotient_eval, all-NoopGate circuit", fmt(t["noop"])))
    lines.append("  %-66s %.3f ms built-in, %.3f ms programs: %.1fx; the whole stage %.2fx" %
                 ("gate cost = stage minus the NoopGate stage (medians)", built_in, prog, prog / built_in if built_in > 0 else float("nan"),
                  med["twin"] / med["gates"]))
    ctx.dev_free(wires)
    for c in circuits.values():
        c.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    ctx = glp.Context(0)
    lines = ["GLP_GATE_PROGRAM gates of a glp_circuit against the built-in bodies of the same gates (profiles/circuit_program_timing.py); device time "
             "between hipEvent pairs with profiling on, median (min..max) of %d rounds after 2 warm-up rounds; two challenges, every operand in HBM" % a.reps]
    for log_n in a.log_n:
        measure(ctx, "synth.arith_circuit", synth.arith_circuit(log_n), log_n, a.reps, lines)
        measure(ctx, "synth.ext_gates_circuit", synth.ext_gates_circuit(log_n), log_n, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
