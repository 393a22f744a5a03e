"""Random cells of witness generation restated on the CPU (include/glp.h, "witness generation, the dataflow half", RANDOM CELLS, and
the rule beside GLP_SALT_TAG_WITNESS): the PRF over the oracle's Poseidon, as tests/zk_restate.py restates the salts; the plan, which
is the plan of tests/witness_plan_restate.py / witness_free_restate.py over inputs + random cells (a random cell is a wave-0 source
exactly as an input cell is); and generation with the PRF values standing where input values stand.  Nothing here shares code with
csrc/.

    random cell number i of the caller's list, proof k of the call, seed (s0, s1, s2, s3):
    b = i >> 3, j = i & 7
    value = Poseidon([s0, s1, s2, s3 + k mod p, TAG_WITNESS, b & 0xffffffff, b >> 32, 0, 0, 0, 0, 0])[j]
"""
import numpy as np

import witness_free_restate as fr
import witness_plan_restate as wp
import witness_program_restate as wpr

TAG_WITNESS = 4
P = 0xFFFFFFFF00000001


def block(oracle, seed, b, k=0):
    """the eight values of block b of proof k: the rate words of one permutation"""
    s = [int(x) % P for x in seed]
    st = np.array([s[0], s[1], s[2], (s[3] + k) % P, TAG_WITNESS, b & 0xFFFFFFFF, b >> 32, 0, 0, 0, 0, 0], np.uint64)
    return oracle.poseidon_permute(st)[:8]


def values(oracle, seed, num_random, k=0):
    """uint64 [num_random]: the value of every random cell of proof k, in the caller's order"""
    if not num_random:
        return np.zeros(0, np.uint64)
    out = np.concatenate([block(oracle, seed, b, k) for b in range((num_random + 7) // 8)])[:num_random]
    assert (out < np.uint64(P)).all()
    return out


def plan(desc, input_cells, random_cells, free=None, cls=None):
    """the restated plan over inputs + random cells (pl.inputs lists the inputs first); pl.num_inputs, pl.random are kept beside it.
    free: None = gate units only (witness_plan_restate.plan), else the free units (witness_free_restate.plan)"""
    ins, rnd = [int(p) for p in input_cells], [int(p) for p in random_cells]
    pl = wp.plan(desc, ins + rnd, cls) if free is None else fr.plan(desc, ins + rnd, free, cls)
    pl.num_inputs, pl.random = len(ins), rnd
    return pl


def generate(oracle, pl, input_values, seed, start, k=0):
    """glp_witness_generate for proof k of a call on a copy of `start`: the PRF values stand where input values stand"""
    vals = [int(v) for v in input_values] + [int(v) for v in values(oracle, seed, len(pl.random), k)]
    assert len(vals) == len(pl.inputs)
    if not hasattr(pl, "free"):
        return wp.generate(pl, vals, start)
    return wpr.generate(pl, vals, start)
