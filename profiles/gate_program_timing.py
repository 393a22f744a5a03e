"""glp_gate_program_sums against the library's own gate bodies (profiles/r16_gate_program.txt).

  python profiles/gate_program_timing.py [--out profiles/r16_gate_program.txt] [--log-n 16 20] [--batch 256] [--reps 9]

The programs: the gates of synth.arith_circuit (PublicInput, Constant, Arithmetic, Noop) and of synth.ext_gates_circuit (PublicInput,
Constant, ArithmeticExtension, MulExtension, Reducing, ReducingExtension, Noop), selector filters included, traced once from a gate
body written over an abstract field (the bodies below restate plonky2's `eval_unfiltered` of these gates; tests/zeta_identity.py holds
the same bodies for the test suite, and tests/test_gpu_gate_program.py pins such programs word for word).
Built-in cost of the same gates: a session's `quotient_eval` stage on the circuit minus the same stage on a circuit of the same
dimensions whose rows are all NoopGate (the baseline of profiles/r13_perm_seam.txt): what k_quotient's gate kernels add to the
permutation terms.  The gate program runs over that session's own oracles (constants ++ sigmas, wires), everything in HBM, two
challenges, sub_bits = quotient_degree_bits = 3.  At the batch shape (2^3 rows) the session proves one proof and the program runs K
proofs in lock step over a many-proof wires oracle.  Timing is data independent.
Stage times: hipEvent pairs with profiling on, median (min..max) of --reps rounds after two warm-up rounds."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plonky2_lib_amd as glp                      # noqa: E402
import plonky2_lib_amd.synth as synth             # noqa: E402
from plonky2_lib_amd import gate_program as gp    # noqa: E402

W7, UNUSED_SELECTOR = 7, 0xFFFFFFFF


def _alg_mul(F, a, b):
    return (F.add(F.mul(a[0], b[0]), F.mul(F.lift(W7), F.mul(a[1], b[1]))), F.add(F.mul(a[0], b[1]), F.mul(a[1], b[0])))


def gate_constraints(F, g, gc, w, pih):
    """unfiltered constraints of one gate of the two circuits, over the field F"""
    t, p0 = int(g["type"]), int(g["p0"])
    if t == synth.GATE_CONSTANT:
        return [F.sub(gc[i], w[i]) for i in range(p0)]
    if t == synth.GATE_PUBLIC_INPUT:
        return [F.sub(w[i], pih[i]) for i in range(4)]
    if t == synth.GATE_ARITHMETIC:
        return [F.sub(w[4 * i + 3], F.add(F.mul(F.mul(w[4 * i], w[4 * i + 1]), gc[0]), F.mul(w[4 * i + 2], gc[1]))) for i in range(p0)]
    out = []
    if t in (synth.GATE_ARITHMETIC_EXTENSION, synth.GATE_MUL_EXTENSION):
        st = 8 if t == synth.GATE_ARITHMETIC_EXTENSION else 6
        for i in range(p0):
            o = st * i
            comp = [F.mul(v, gc[0]) for v in _alg_mul(F, (w[o], w[o + 1]), (w[o + 2], w[o + 3]))]
            if t == synth.GATE_ARITHMETIC_EXTENSION:
                comp = [F.add(comp[k], F.mul(w[o + 4 + k], gc[1])) for k in range(2)]
            out += [F.sub(w[o + st - 2 + k], comp[k]) for k in range(2)]
    elif t in (synth.GATE_REDUCING, synth.GATE_REDUCING_EXTENSION):
        cw = 1 if t == synth.GATE_REDUCING else 2
        alpha, acc = (w[2], w[3]), (w[4], w[5])
        for i in range(p0):
            c = 6 + cw * i
            a = 6 + cw * p0 + 2 * i if i + 1 < p0 else 0
            pr = _alg_mul(F, acc, alpha)
            out += [F.sub(F.add(pr[0], w[c]), w[a]), F.sub(F.add(pr[1], w[c + 1]) if cw == 2 else pr[1], w[a + 1])]
            acc = (w[a], w[a + 1])
    elif t != synth.GATE_NOOP:
        raise NotImplementedError("gate type %d" % t)
    return out


def trace(desc):
    nsel, nc = int(desc.num_selectors), int(desc.num_constants)
    asm = gp.Assembler([nc, int(desc.num_wires)], num_params=4)
    F = gp.TraceField(asm)
    cs, lw, pih = [asm.col(0, j) for j in range(nc)], [asm.col(1, j) for j in range(int(desc.num_wires))], [asm.param(j) for j in range(4)]
    nconstraints = 0
    for g in desc.gates:
        s, filt = cs[int(g["selector_index"])], F.one
        for v in range(int(g["group_start"]), int(g["group_end"])):
            if v != int(g["row"]):
                filt = F.mul(filt, F.sub(F.lift(v), s))
        if nsel > 1:
            filt = F.mul(filt, F.sub(F.lift(UNUSED_SELECTOR), s))
        vs = gate_constraints(F, g, cs[nsel:], lw, pih)
        nconstraints += len(vs)
        for v in vs:
            asm.emit(v)
        asm.end(filt)
    return asm.assemble(hoist_emits=True), nconstraints


def stage_ms(ctx, name):
    return sum(ms for n, ms, _ in ctx.stages() if n == name)


def fmt(t):
    return "%.3f (%.3f..%.3f)" % (float(np.median(t)), min(t), max(t))


def measure(ctx, what, desc, log_n, K, reps, lines):
    n, nw, nch = 1 << log_n, int(desc.num_wires), int(desc.num_challenges)
    sub_bits = int(desc.quotient_degree_factor).bit_length() - 1
    desc.cap_height = min(int(desc.cap_height), log_n + int(desc.rate_bits))
    noop = synth.Builder(_config_of(desc), log_n, seed=3, random_from_row=n).build()
    noop.cap_height = desc.cap_height
    assert (noop.num_wires, noop.num_routed_wires, noop.num_challenges, noop.quotient_degree_factor) == \
        (desc.num_wires, desc.num_routed_wires, desc.num_challenges, desc.quotient_degree_factor)
    prog, nconstraints = trace(desc)
    ops = {name: sum(i.op == op for i in prog.instructions) for op, name in gp.OP_NAMES.items()}
    g = ctx.gate_program(prog)
    gc, gn = glp.Circuit(ctx, desc), glp.Circuit(ctx, noop)
    wires = ctx.dev_alloc(nw * n * 8)
    ctx.fill_random_device(wires, nw * n, 77)
    wires_b = ctx.batch_many_from_values(glp.splitmix_field(78, K * nw * n).reshape(K, nw, n), int(desc.rate_bits), desc.cap_height) if K > 1 else None
    chal = glp.splitmix_field(5, 3 * K * nch).reshape(3, K, nch)
    params = glp.splitmix_field(6, K * 4).reshape(K, 4)
    out = ctx.dev_alloc(K * nch * (n << sub_bits) * 8)
    one = lambda a: a[0] if K == 1 else a                                                # noqa: E731
    ctx.set_profiling(True)
    t = {k: [] for k in ("gates", "noop", "prog")}
    for i in range(reps + 2):
        ctx.stage_reset()
        s = glp.Session(gc, dev_wires_ptr=wires)
        s.partial_products(chal[0, 0], chal[1, 0])
        s.quotient(chal[2, 0])
        a = stage_ms(ctx, "quotient_eval")
        g.sums([s.oracle(0), wires_b if K > 1 else s.oracle(1)], sub_bits, one(chal[2]), one(params), out_dev_ptr=out)
        ctx.synchronize()
        p = stage_ms(ctx, "gate_program.sums")
        s.end()
        s = glp.Session(gn, dev_wires_ptr=wires)
        s.partial_products(chal[0, 0], chal[1, 0])
        s.quotient(chal[2, 0])
        b = stage_ms(ctx, "quotient_eval") - a
        s.end()
        if i >= 2:
            t["gates"].append(a); t["noop"].append(b); t["prog"].append(p)
    ctx.set_profiling(False)
    med = {k: float(np.median(v)) for k, v in t.items()}
    built_in = med["gates"] - med["noop"]
    lines.append("%s, 2^%d rows, %d wires, %d gate types, %d constraints; program: %d instructions (%s), %d registers, max %d EMITs per gate; K = %d" %
                 (what, log_n, nw, len(desc.gates), nconstraints, len(prog), ", ".join("%d %s" % (v, k) for k, v in ops.items()), prog.num_regs,
                  prog.max_constraints, K))
    lines.append("  %-62s %s ms" % ("session quotient_eval, the circuit (one proof)", fmt(t["gates"])))
    lines.append("  %-62s %s ms" % ("session quotient_eval, all-NoopGate circuit (one proof)", fmt(t["noop"])))
    lines.append("  %-62s %.3f ms" % ("built-in gate cost = the difference of the medians", built_in))
    lines.append("  %-62s %s ms   %.1fx the built-in cost%s" % ("gate_program.sums (K proofs)", fmt(t["prog"]), med["prog"] / built_in if built_in > 0 else float("nan"),
                                                               "" if K == 1 else " of one proof, %.2fx that of %d" % (med["prog"] / (K * built_in), K)))
    for ptr in (wires, out):
        ctx.dev_free(ptr)
    if wires_b is not None:
        wires_b.free()
    g.free(); gc.free(); gn.free()


def _config_of(desc):
    cfg = synth.Config.standard_ecc_config() if int(desc.num_wires) == 136 else synth.Config.standard_recursion_config()
    cfg.num_challenges = int(desc.num_challenges)
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    ctx = glp.Context(0)
    lines = ["glp_gate_program_sums on traced gate programs against the built-in gate bodies of the same circuits (profiles/gate_program_timing.py); "
             "device time between hipEvent pairs with profiling on, median (min..max) of %d rounds after 2 warm-up rounds; two challenges, sub_bits 3, "
             "every operand in HBM" % a.reps]
    for log_n in a.log_n:
        measure(ctx, "synth.arith_circuit", synth.arith_circuit(log_n), log_n, 1, a.reps, lines)
        measure(ctx, "synth.ext_gates_circuit", synth.ext_gates_circuit(log_n), log_n, 1, a.reps, lines)
    if a.batch:
        measure(ctx, "synth.arith_circuit", synth.arith_circuit(3, synth.Config.standard_recursion_config(), num_const_rows=2, num_noop_rows=1), 3, a.batch,
                a.reps, lines)
        measure(ctx, "synth.ext_gates_circuit", synth.ext_gates_circuit(3), 3, a.batch, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
