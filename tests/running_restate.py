"""glp_running_columns (include/glp.h) restated in plain Python integers: helper columns h_t = num_t / den_t, one inversion per
element, and the running column by a plain loop over the rows.  Nothing is batched and nothing is scanned here, which is the point."""
import numpy as np

P = 0xFFFFFFFF00000001
SUM, PRODUCT = 0, 1              # GLP_RUN_SUM, GLP_RUN_PRODUCT


class ZeroDenominator(ValueError):
    def __init__(self, a, t, i):
        super().__init__("zero denominator at argument %d, term %d, row %d" % (a, t, i))
        self.at = (a, t, i)


def first_zero(dens):
    """(a, t, i) of the first zero denominator of dens [A][T][n] in that order, or None"""
    z = np.argwhere(np.asarray(dens, np.uint64) % np.uint64(P) == 0)
    return None if not len(z) else tuple(int(v) for v in z[0])


def running_columns(kind, nums, dens):
    """One proof.  dens [A][T][n] (any u64 words, reduced mod p), nums the same or None for all ones ->
    (out [A][T + 1][n] uint64: the T helper columns of each argument, then its Z; totals [A] uint64)."""
    dens = np.asarray(dens, np.uint64)
    A, T, n = dens.shape
    at = first_zero(dens)
    if at is not None:
        raise ZeroDenominator(*at)
    out = np.zeros((A, T + 1, n), np.uint64)
    totals = np.zeros(A, np.uint64)
    for a in range(A):
        h = []
        for t in range(T):
            d = [int(v) % P for v in dens[a, t]]
            m = [1] * n if nums is None else [int(v) % P for v in np.asarray(nums, np.uint64)[a, t]]
            h.append([m[i] * pow(d[i], -1, P) % P for i in range(n)])
            out[a, t] = h[-1]
        z = 0 if kind == SUM else 1
        for i in range(n):
            out[a, T, i] = z
            for t in range(T):
                z = (z + h[t][i]) % P if kind == SUM else z * h[t][i] % P
        totals[a] = z
    return out, totals


def permutation_terms(desc, wires, beta, gamma, pair=False):
    """The permutation argument of a circuit description as one product-kind running argument: nums[j][i] = w_j + beta k_j x_i + gamma,
    dens[j][i] = w_j + beta sigma_j + gamma over the routed wires, x_i = w_n^i -> (nums, dens) [T][n] uint64, T = num_routed_wires.
    pair: term t is the product of the factors of wires 2 t and 2 t + 1 (T = num_routed_wires / 2; the same Z, within num_terms <= 64
    for the 80 routed wires of the standard configuration)."""
    from coset_quotient import root_of_unity
    lg, nr = int(desc.degree_bits), int(desc.num_routed_wires)
    n, wn = 1 << lg, root_of_unity(lg)
    beta, gamma = int(beta), int(gamma)
    nums, dens = np.zeros((nr, n), np.uint64), np.zeros((nr, n), np.uint64)
    for j in range(nr):
        k, x = int(desc.k_is[j]), 1
        for i in range(n):
            w = int(wires[j][i])
            nums[j, i] = (w + beta * k % P * x + gamma) % P
            dens[j, i] = (w + beta * int(desc.sigmas[j][i]) + gamma) % P
            x = x * wn % P
    if not pair:
        return nums, dens
    assert nr % 2 == 0

    def fold(v):
        return np.array([[int(v[2 * t, i]) * int(v[2 * t + 1, i]) % P for i in range(n)] for t in range(nr // 2)], np.uint64)
    return fold(nums), fold(dens)


def lookup_trace(lg, seed, off_by_one=False):
    """A trace with a lookup in it, [4][n]: a table column of distinct values, the multiplicity column, and two looking columns whose
    every cell is a table value; multiplicity[r] counts the cells that look up table[r].  off_by_one: one multiplicity is one too many."""
    rng = np.random.default_rng(seed)
    n = 1 << lg
    table = rng.choice(np.arange(1, 1 << 20, dtype=np.uint64), n, replace=False) * np.uint64(0x100000001)
    picks = rng.integers(0, max(1, n // 2), (2, n))
    mult = np.bincount(picks.reshape(-1), minlength=n).astype(np.uint64)
    if off_by_one:
        mult[int(picks[0, 0])] += np.uint64(1)
    return np.stack([table, mult, table[picks[0]], table[picks[1]]])


def lookup_terms(trace, gamma):
    """logUp over lookup_trace's columns: sum_i ( m_i / (gamma + t_i) - 1 / (gamma + f0_i) - 1 / (gamma + f1_i) ) = 0
    -> (nums, dens) [3][n]"""
    n, g = trace.shape[1], int(gamma)
    dens = np.array([[(g + int(v)) % P for v in trace[c]] for c in (0, 2, 3)], np.uint64)
    nums = np.stack([trace[1] % np.uint64(P), np.full(n, P - 1, np.uint64), np.full(n, P - 1, np.uint64)])
    return nums, dens
