"""A caller-defined lookup argument end to end at the commitment seam, through the library's entry points only (include/glp.h,
"caller-defined running arguments at the commitment seam").

The trace has n = 16 rows and four columns: a table, a multiplicity column and two looking columns (running_restate.lookup_trace).
With the challenge gamma arriving as a PARAM the logUp argument is
    sum_i ( m_i / (gamma + t_i) - 1 / (gamma + f0_i) - 1 / (gamma + f1_i) ) = 0.
GateProgram.rows writes the three denominators and the three numerators per row into HBM, Context.running_columns reads them where
they lie and writes the helper columns h_0..h_2 and the running sum Z (total 0), batch_from_values_device commits those four columns,
and a second program states the constraints over the two committed oracles: h_t den_t - num_t for each term and
Z(w x) - Z(x) - (h_0 + h_1 + h_2) with COL_NEXT.  GateProgram.sums evaluates it on the coset of 4 n points; divided by Z_H there as
tests/coset_quotient.py does, the quotient's coset iFFT has no coefficient at or above M - n: the constraints vanish on H.  With one
multiplicity off by one the total is not 0, the last row's transition fails and the high coefficients are not zero."""
import numpy as np
import pytest

import plonky2_lib_amd as glp
from plonky2_lib_amd import gate_program as gp
import plonky2_lib_amd.gl_numpy as gl
import coset_quotient as cq
import running_restate as rr

pytestmark = pytest.mark.gpu

P, GEN = cq.P, cq.GEN
LG, SUB_BITS, RB, CAP_H = 4, 2, 3, 4
T = 3


@pytest.fixture(scope="module")
def ctx():
    c = glp.Context(0)
    yield c
    c.close()


def _terms(asm, F, trace_oracle=0):
    """(denominators, numerators) of the three terms as operands over the trace columns table, multiplicity, f0, f1"""
    gamma = asm.param(0)
    dens = [F.add(gamma, asm.col(trace_oracle, c)) for c in (0, 2, 3)]
    nums = [asm.col(trace_oracle, 1), asm.imm(P - 1), asm.imm(P - 1)]
    return dens, nums


def _rows_program():
    asm = gp.Assembler([4], num_params=1)
    dens, nums = _terms(asm, gp.TraceField(asm))
    for v in dens + nums:                                       # all denominators, then all numerators: glp_running_columns' pass-through layout
        asm.emit(v)
    asm.end(asm.imm(1))
    return asm.assemble()


def _constraint_program():
    asm = gp.Assembler([4, T + 1], num_params=1)                # oracle 0: the trace; oracle 1: h_0, h_1, h_2, Z
    F = gp.TraceField(asm)
    dens, nums = _terms(asm, F)
    h = [asm.col(1, t) for t in range(T)]
    for t in range(T):
        asm.emit(F.sub(F.mul(h[t], dens[t]), nums[t]))
    step = F.sub(asm.col_next(1, T), asm.col(1, T))
    asm.emit(F.sub(step, F.add(F.add(h[0], h[1]), h[2])))
    asm.end(asm.imm(1))
    return asm.assemble(hoist_emits=True)


def _high_coefficients(ctx, trace, gamma, alpha):
    """-> (the argument's total, the quotient's coefficients at and above M - n)"""
    n, M, S = 1 << LG, 1 << (LG + SUB_BITS), 1 << SUB_BITS
    rows, cons = ctx.gate_program(_rows_program()), ctx.gate_program(_constraint_program())
    assert rows.num_out == 2 * T and cons.num_out == T + 1
    d_trace = ctx.dev_alloc(trace.nbytes)
    d_terms = ctx.dev_alloc(8 * 2 * T * n)
    d_cols = ctx.dev_alloc(8 * (T + 1) * n)
    tb = hb = None
    try:
        ctx.dev_upload(d_trace, trace)
        assert rows.rows([trace.shape], [gamma], in_dev_ptrs=[d_trace], out_dev_ptr=d_terms) is None
        out, totals = ctx.running_columns(glp.RUN_SUM, None, None, 1, 1, T, LG, 2 * T * n, nums_dev_ptr=d_terms + 8 * T * n, dens_dev_ptr=d_terms,
                                          out_dev_ptr=d_cols)
        assert out is None and totals.shape == (1, 1)
        cols = np.empty((T + 1, n), np.uint64)                  # only to pin them against the restatement: the pipeline does not need them
        ctx.dev_download(d_cols, cols)
        want, want_tot = rr.running_columns(rr.SUM, *(v[None] for v in rr.lookup_terms(trace, gamma)))
        assert (cols == want[0]).all() and totals[0, 0] == want_tot[0]
        tb = ctx.batch_from_values_device(d_trace, 4, LG, RB, CAP_H)
        hb = ctx.batch_from_values_device(d_cols, T + 1, LG, RB, CAP_H)
        sums = cons.sums([tb, hb], SUB_BITS, [alpha], [gamma])
        assert sums.shape == (1, M)
        gn, wS = pow(GEN, n, P), cq.root_of_unity(SUB_BITS)
        zh_inv = [cq._inv((gn * pow(wS, r, P) - 1) % P) for r in range(S)]        # Z_H(g W_M^i) = g^n w_S^(i mod S) - 1
        q = np.array([int(v) * zh_inv[i % S] % P for i, v in enumerate(sums[0])], np.uint64)
        coeffs = ctx.coset_ifft(q, GEN)[0]
        return int(totals[0, 0]), coeffs[M - n:]
    finally:
        ctx.synchronize()
        for b in (tb, hb):
            if b is not None:
                b.free()
        for d in (d_trace, d_terms, d_cols):
            ctx.dev_free(d)
        rows.free(); cons.free()


def test_a_lookup_argument_closes_and_its_constraints_vanish_on_h(ctx):
    gamma, alpha = (int(v) for v in gl.rand(np.random.default_rng(41), (2,)))
    total, high = _high_coefficients(ctx, rr.lookup_trace(LG, seed=8), gamma, alpha)
    assert total == 0
    assert len(high) == 1 << LG and not high.any()


def test_one_multiplicity_off_by_one_does_not(ctx):
    gamma, alpha = (int(v) for v in gl.rand(np.random.default_rng(41), (2,)))
    total, high = _high_coefficients(ctx, rr.lookup_trace(LG, seed=8, off_by_one=True), gamma, alpha)
    assert total != 0
    assert high.any()
