"""Check the witness of a circuit hand-off file on the GPU: which gate, row, constraint or copy constraint it breaks, if any.

    python -m plonky2_lib_amd.tools.check_glpc [--refill] <file.glpc>
    (from the repository root: python plonky2-lib_amd/tools/check_glpc.py [--refill] <file.glpc>)

Opens the file (it must carry a witness), creates the circuit and runs glp_witness_check (include/glp.h) on the file's wires and
public inputs: every gate's unfiltered constraints on the rows of H, every copy constraint.  Prints the report and the failing rows
per gate; exit status 0 if the witness satisfies the circuit, 1 if not, 2 if the file cannot be checked.

--refill: only the routed columns of the file's witness are uploaded, the advice columns are zeroed and glp_witness_fill(only_advice)
derives them before the check, so the report judges the GPU generators against the file's routed inputs (advice wires that no
row-local generator writes are zero then: a gate that constrains such a wire fails here and not without --refill)."""
import argparse
import os
import sys

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import plonky2_lib_amd as glp                    # noqa: E402


def check_file(path, refill=False, out=sys.stdout):
    """True iff the witness of the file satisfies its circuit; the report goes to `out`."""
    with glp.CircuitFile(path) as cf:
        desc = cf.desc
        if not cf.has_witness:
            raise glp.GlpError(-1, "%s carries no witness" % path)
        n = 1 << desc.degree_bits
        print("%s: 2^%d rows x %d wires (%d routed), %d gates, %d public inputs" % (path, desc.degree_bits, desc.num_wires, desc.num_routed_wires,
                                                                                 len(desc.gates), len(desc.public_inputs)), file=out)
        with glp.Context(0) as ctx:
            gc = glp.Circuit(ctx, desc)
            if refill:
                w = np.ascontiguousarray(desc.wires).copy()
                w[desc.num_routed_wires:] = 0
                dev = ctx.dev_alloc(w.nbytes)
                ctx.dev_upload(dev, w)
                gc.witness_fill(dev, only_advice=True)
                rep = gc.check_witness(dev_wires_ptr=dev, by_gate=True)
                ctx.dev_free(dev)
                print("advice columns %d..%d derived on the GPU from the routed columns" % (desc.num_routed_wires, desc.num_wires - 1), file=out)
            else:
                rep = gc.check_witness(by_gate=True)
            print(str(rep), file=out)
            for gi, (g, rows) in enumerate(zip(desc.gates, rep.rows_failed_by_gate)):
                on = int((np.asarray(desc.constants[g["selector_index"]]) == gi).sum())
                print("  gate %2d %-24s (p0 = %d, p1 = %d, %d constraints): %d of its %d rows fail"
                      % (gi, glp.GATE_TYPE_NAMES.get(g["type"], "type %d" % g["type"]), g["p0"], g["p1"], g["num_constraints"], rows, on), file=out)
            print("constraints: %d failing on %d of %d rows; copies: %d of %d routed positions broken"
                  % (rep.failed_constraints, rep.failed_rows, n, rep.failed_copies, desc.num_routed_wires * n), file=out)
            gc.free()
            return rep.ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file")
    ap.add_argument("--refill", action="store_true", help="derive the advice columns on the GPU (glp_witness_fill) before the check")
    a = ap.parse_args(argv)
    try:
        return 0 if check_file(a.file, a.refill) else 1
    except glp.GlpError as e:
        print("check_glpc: %s" % e, file=sys.stderr)
        return 2


if __name__ == "__main__":
    sys.exit(main())
