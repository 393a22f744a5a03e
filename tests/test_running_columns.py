"""The CPU restatements of the caller-defined running arguments (include/glp.h: glp_gate_program_rows, glp_running_columns), pinned
before any GPU sees them.  No GPU.
1. running_restate, product kind, on the permutation argument of coset_quotient.seam_circuit with T = num_routed_wires: its Z is the Z
   coset_quotient.zs_partial_products (the restatement perm_restate and the oracle-pinned tests share) computes for that circuit with
   chunk_size = num_routed_wires, i.e. without partial products.  The pairwise-folded form the GPU test uses (T = 40 <= 64) is the same Z.
2. running_restate, sum kind: a lookup with correct multiplicities totals 0; with one multiplicity off by one it does not.
3. trace_program_restate.run_rows equals direct numpy evaluation of the program's formulas."""
from types import SimpleNamespace

import numpy as np

import plonky2_lib_amd.gl_numpy as gl
from plonky2_lib_amd import gate_program as gp
import coset_quotient as cq
import perm_restate as pr
import running_restate as rr
import trace_program_restate as tr

P = cq.P


def one_chunk(desc):
    """the description with chunk_size = num_routed_wires: no partial products, the oracle is Z alone"""
    return SimpleNamespace(degree_bits=desc.degree_bits, num_routed_wires=desc.num_routed_wires, num_challenges=desc.num_challenges,
                           quotient_degree_factor=desc.num_routed_wires, num_partial_products=0, k_is=desc.k_is, sigmas=desc.sigmas)


def test_product_kind_is_the_permutation_arguments_z(oracle):
    desc = cq.seam_circuit(oracle)
    nch, nr, n = int(desc.num_challenges), int(desc.num_routed_wires), 1 << int(desc.degree_bits)
    ch = gl.rand(np.random.default_rng(31), (2, nch))
    want = cq.zs_partial_products(one_chunk(desc), desc.wires, ch[0], ch[1])
    assert want.shape == (nch, n) and pr.num_terms(one_chunk(desc)) == 2 * nch
    terms = [rr.permutation_terms(desc, desc.wires, ch[0][a], ch[1][a]) for a in range(nch)]
    nums, dens = np.stack([t[0] for t in terms]), np.stack([t[1] for t in terms])
    assert dens.shape == (nch, nr, n)
    out, totals = rr.running_columns(rr.PRODUCT, nums, dens)
    assert (out[:, nr] == want).all()
    assert (totals == 1).all()                                   # the argument closes
    assert (gl.mul(out[:, :nr], dens) == nums).all()             # h den = num, every cell
    folded = [rr.permutation_terms(desc, desc.wires, ch[0][a], ch[1][a], pair=True) for a in range(nch)]
    out2, totals2 = rr.running_columns(rr.PRODUCT, np.stack([t[0] for t in folded]), np.stack([t[1] for t in folded]))
    assert out2.shape == (nch, nr // 2 + 1, n) and (out2[:, nr // 2] == want).all() and (totals2 == 1).all()


def test_sum_kind_lookup_closes_with_the_right_multiplicities():
    gamma = int(gl.rand(np.random.default_rng(5), (1,))[0])
    trace = rr.lookup_trace(4, seed=8)
    nums, dens = rr.lookup_terms(trace, gamma)
    out, totals = rr.running_columns(rr.SUM, nums[None], dens[None])
    assert out.shape == (1, 4, 16) and out[0, 3, 0] == 0 and totals[0] == 0
    z = [int(v) for v in out[0, 3]]
    for i in range(15):                                          # Z[i + 1] = Z[i] + sum_t h_t[i]
        assert z[i + 1] == (z[i] + sum(int(out[0, t, i]) for t in range(3))) % P
    assert z[5] != 0
    bad = rr.lookup_trace(4, seed=8, off_by_one=True)
    assert (bad != trace).sum() == 1
    nums, dens = rr.lookup_terms(bad, gamma)
    _out, totals = rr.running_columns(rr.SUM, nums[None], dens[None])
    assert totals[0] != 0
    # all ones for numerators is nums = None
    a, ta = rr.running_columns(rr.SUM, None, dens[None])
    b, tb = rr.running_columns(rr.SUM, np.ones_like(dens)[None], dens[None])
    assert (a == b).all() and (ta == tb).all()
    dens[1, 7] = 0
    dens[2, 3] = P                                               # a word >= p is reduced: zero as well, and later in (a, t, i) order
    try:
        rr.running_columns(rr.SUM, nums[None], dens[None])
        assert False, "a zero denominator went through"
    except rr.ZeroDenominator as e:
        assert e.at == (0, 1, 7)


def test_rows_restatement_is_direct_evaluation():
    lg, n = 4, 16
    rng = np.random.default_rng(12)
    t0, t1 = gl.rand(rng, (3, n)), gl.rand(rng, (2, n))
    beta, gamma = (int(v) for v in gl.rand(rng, (2,)))
    asm = gp.Assembler([3, 2], num_params=2)
    F = gp.TraceField(asm)
    a = F.add(F.mul(asm.param(0), asm.col(0, 1)), asm.param(1))              # beta c01 + gamma
    asm.emit(F.add(a, asm.col(1, 0)))
    asm.emit(F.sub(asm.col_next(0, 2), F.mul(asm.x, asm.col(0, 0))))          # c02(next) - x c00
    asm.emit(F.mul(asm.col_next(1, 1), F.lift(P - 1)))                        # -c11(next)
    asm.emit(asm.x)
    asm.end(asm.imm(1))
    prog = asm.assemble()
    assert tr.shape_error(prog) is None and prog.max_constraints == 4
    got = tr.run_rows(prog, [t0, t1], [beta, gamma])
    x = np.array([pow(cq.root_of_unity(lg), i, P) for i in range(n)], np.uint64)
    assert (got[3] == x).all() and x[1] == cq.root_of_unity(lg) and pow(int(x[1]), n, P) == 1
    want = [gl.add(gl.add(gl.mul(np.uint64(beta), t0[1]), np.uint64(gamma)), t1[0]),
            gl.sub(np.roll(t0[2], -1), gl.mul(x, t0[0])),
            gl.neg(np.roll(t1[1], -1)),
            x]
    assert got.shape == (4, n) and (got == np.stack(want)).all()
    assert got[1][n - 1] == (int(t0[2][0]) - int(x[n - 1]) * int(t0[0][n - 1])) % P       # the last row's next is row 0
    # a word >= p is reduced as it is read
    t0b = t0.copy()
    t0b[1, 3] += np.uint64(P) if t0b[1, 3] < (1 << 64) - P else np.uint64(0)
    assert (tr.run_rows(prog, [t0b, t1], [beta, gamma]) == got).all()
    # shapes the library refuses
    for build, field in ((lambda s: (s.emit(s.x), s.end(s.x), s.emit(s.x), s.end(s.imm(1))), "op"),
                         (lambda s: (s.emit(s.x), s.end(s.x)), "a"),
                         (lambda s: (s.emit(s.x), s.end(s.imm(2))), "a"),
                         (lambda s: (s.end(s.imm(1)),), "op")):
        s = gp.Assembler([1])
        build(s)
        assert tr.shape_error(s.assemble())[1] == field
