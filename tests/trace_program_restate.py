"""Gate programs on the rows of H (include/glp.h, glp_gate_program_rows) restated: the third reading of a program, over whole columns
with gl_numpy.  Like gate_program_restate.run it reads the Assembler's instruction list, never the encoded words, so it shares no
decoder with the library.

COL is row i, COL_NEXT row (i + 1) mod n, X is w_n^i, and EMIT number t (counted from the start of the program) is column t of the
result.  The program is a single gate closed by END IMM(1); `shape_error` says why a program is not."""
import numpy as np

import plonky2_lib_amd.gl_numpy as gl
from plonky2_lib_amd import gate_program as gp
from gate_program_restate import P, root_of_unity


def shape_error(prog):
    """None, or (instruction index, field, why) for a program glp_gate_program_rows refuses by its shape"""
    ends = [i for i, ins in enumerate(prog.instructions) if ins.op == gp.OP_END]
    if len(ends) != 1:
        return ends[0], "op", "END before the last instruction"
    last = prog.instructions[-1]
    if last.a.kind != gp.IMM:
        return len(prog.instructions) - 1, "a", "END on an operand that is not IMM"
    if int(prog.pool[last.a.index]) != 1:
        return len(prog.instructions) - 1, "a", "END on a pool word that is not 1"
    if not any(ins.op == gp.OP_EMIT for ins in prog.instructions):
        return len(prog.instructions) - 1, "op", "no EMIT"
    return None


def rows_points(lg):
    """w_n^i, i < n"""
    return gl.powers(root_of_unity(lg), 1 << lg)


def run_rows(prog, cols, params=()):
    """prog: a gate_program.Program; cols[o]: [>= oracle_cols[o]][n] values of input o on H, any u64 words (reduced mod p as they are
    read); params [num_params] -> [number of EMITs][n]"""
    assert shape_error(prog) is None, shape_error(prog)
    cols = [gl.canon(np.asarray(c, np.uint64)) for c in cols]
    n = cols[0].shape[-1]
    x = rows_points(n.bit_length() - 1)
    regs, out = {}, []

    def value(o):
        if o.kind == gp.REG:
            return regs[o.index]
        if o.kind == gp.COL:
            return cols[o.oracle][o.index]
        if o.kind == gp.COL_NEXT:
            return np.roll(cols[o.oracle][o.index], -1)
        if o.kind == gp.IMM:
            return np.full(n, prog.pool[o.index], np.uint64)
        if o.kind == gp.PARAM:
            return np.full(n, int(params[o.index]) % P, np.uint64)
        assert o.kind == gp.X
        return x
    for ins in prog.instructions:
        a = value(ins.a)
        if ins.op == gp.OP_ADD:
            regs[ins.dst.index] = gl.add(a, value(ins.b))
        elif ins.op == gp.OP_SUB:
            regs[ins.dst.index] = gl.sub(a, value(ins.b))
        elif ins.op == gp.OP_MUL:
            regs[ins.dst.index] = gl.mul(a, value(ins.b))
        elif ins.op == gp.OP_MOV:
            regs[ins.dst.index] = a
        elif ins.op == gp.OP_EMIT:
            out.append(np.array(a, np.uint64))
        else:
            assert ins.op == gp.OP_END
    return np.stack(out)
