"""glp_fri_* against the session's own openings / FRI stages on the same four batches, in one process (profiling on):
the real secp256k1 circuit as bench.py builds it (argv[1] signatures, default 10 = 2^20 rows), the plonk instance (zeta: all four
oracles in full; g zeta: the Z columns), one challenge sequence for both.  Prints the per-stage hipEvent times of every repetition
and requires the same openings and FriProof words from both.

    python profiles/fri_openings_speed.py [signatures] [repetitions]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonky2_lib_amd as glp
from plonky2_lib_amd import gadgets_ecdsa as E

P = glp.P
nsig = int(sys.argv[1]) if len(sys.argv) > 1 else 10
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
SEED = 0x5EED0003

desc = E.ecdsa_circuit(E.random_signatures(nsig, seed=SEED))
ctx = glp.Context(0)
gc = glp.Circuit(ctx, desc)
w = np.ascontiguousarray(desc.wires)
dptr = ctx.dev_alloc(w.nbytes)
ctx.dev_upload(dptr, w)
nch, lg = desc.num_challenges, desc.degree_bits
print("circuit: 2^%d rows, %d wires, %d reductions, %d query rounds" % (lg, desc.num_wires, len(desc.reduction_arity_bits), desc.num_query_rounds))
rng = np.random.default_rng(8)
chal = [int(x) for x in rng.integers(1, 1 << 62, 64, dtype=np.int64)]
g = pow(1753635133440165772, 1 << (32 - lg), P)
SESSION = ("openings", "fri_combine", "fri_commit", "fri_queries")
GENERIC = ("fri.openings", "fri.combine", "fri.commit", "fri.fold", "fri.queries")
ctx.set_profiling(True)
for rep in range(reps):
    s = glp.Session(gc, dev_wires_ptr=dptr)
    s.partial_products(chal[0:nch], chal[4:4 + nch])
    s.quotient(chal[8:8 + nch])
    obs = [s.oracle(i) for i in range(4)]
    zeta = (chal[12], chal[13])
    points = [(zeta, [(o, 0, obs[o].ncols) for o in range(4)]), ((zeta[0] * g % P, zeta[1] * g % P), [(2, 0, nch)])]
    f = glp.FriOpenings(ctx, obs, points, desc.reduction_arity_bits, desc.proof_of_work_bits, desc.num_query_rounds)
    ctx.stage_reset()
    op = s.open(zeta)
    fop = f.open()
    a = nch + sum(b.ncols for b in obs[:2])
    assert (fop == np.concatenate([op[:a], op[a + nch:], op[a:a + nch]])).all()
    s.fri_combine(chal[14:16]); f.combine(chal[14:16])
    for r in range(len(desc.reduction_arity_bits)):
        assert (s.fri_commit() == f.commit()).all()
        s.fri_fold(chal[16 + 2 * r:18 + 2 * r]); f.fold(chal[16 + 2 * r:18 + 2 * r])
    assert (s.fri_final_poly() == f.final_poly()).all()
    idx = [int(x) for x in rng.integers(0, 1 << (lg + desc.rate_bits), desc.num_query_rounds)]
    s.queries(5, idx); f.queries(5, idx)
    proof, fproof = s.proof(), f.proof()
    start = 3 * (4 << desc.cap_height) + 2 * len(op)
    assert (fproof == proof[start:len(proof) - len(desc.public_inputs)]).all()
    tot = {}
    for name, ms, _ in ctx.stages():
        tot[name] = tot.get(name, 0.0) + ms
    print("rep %d  session: %s  sum %.3f ms" % (rep, "  ".join("%s %.3f" % (k, tot.get(k, 0.0)) for k in SESSION), sum(tot.get(k, 0.0) for k in SESSION)))
    print("rep %d  glp_fri: %s  sum %.3f ms   ratio combine %.3f, all %.3f" % (
        rep, "  ".join("%s %.3f" % (k, tot.get(k, 0.0)) for k in GENERIC), sum(tot.get(k, 0.0) for k in GENERIC),
        tot.get("fri.combine", 0.0) / max(tot.get("fri_combine", 0.0), 1e-9),
        sum(tot.get(k, 0.0) for k in GENERIC) / max(sum(tot.get(k, 0.0) for k in SESSION), 1e-9)))
    f.end(); s.end()
print("same openings and FriProof words from both in every repetition")
