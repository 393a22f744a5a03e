"""The permutation argument at the commitment seam (glp_perm_*), restated: tests/coset_quotient.py with the gates taken out.

`synthetic` builds a circuit description that has a permutation argument and nothing else: a random permutation of the routed cells,
sigma values k_is[col'] w^row' of each cell's image, wires constant along the cycles, random advice columns.  `perm_quotient` is
coset_quotient.quotient_values without the gates plus alpha^T gate_sums / Z_H, `gate_sums` is the other half: the filtered,
alpha-reduced gate constraints per coset row.  tests/test_perm_seam.py pins perm_quotient(.., gate_sums(..)) == quotient_values on a
circuit that has gates, so the split is the whole."""
from types import SimpleNamespace

import numpy as np

from coset_quotient import P, GEN, root_of_unity, _inv, _chunks
from zeta_identity import gate_constraints, _Fp, UNUSED_SELECTOR


def plonky2_k_is(num_routed):
    """plonky2's `get_unique_coset_shifts`: powers of the generator 7"""
    return np.array([pow(GEN, j, P) for j in range(num_routed)], np.uint64)


def synthetic(lg, num_wires, num_routed, chunk, nch, seed, k_is=None, wires_seed=None):
    """A description with the attributes coset_quotient reads (and the ones Context.perm_* reads), no gates: `sigmas`
    [num_routed][n], `wires` [num_wires][n] satisfying the copy constraints, `k_is` distinct coset shifts (random unless given).
    wires_seed: another witness of the same circuit (the permutation and the sigmas depend on `seed` alone)."""
    rng = np.random.default_rng(seed)
    n = 1 << lg

    def field(shape):
        return (rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)) % np.uint64(P)
    if k_is is None:
        # distinct cosets k H: distinct k^n (n a power of two, so k -> k^n is 2^lg to one; collisions are 2^-64 events, checked)
        k_is = field(num_routed)
        k_is[0] = 1
        assert len({pow(int(k), n, P) for k in k_is}) == num_routed and all(int(k) for k in k_is)
    k_is = np.asarray(k_is, np.uint64)
    cells = num_routed * n
    perm = rng.permutation(cells)                      # cell col * n + row -> its image
    w = root_of_unity(lg)
    wpow = [1] * n
    for i in range(1, n):
        wpow[i] = wpow[i - 1] * w % P
    sigmas = np.zeros((num_routed, n), np.uint64)
    for cell in range(cells):
        img = int(perm[cell])
        sigmas[cell // n, cell % n] = int(k_is[img // n]) * wpow[img % n] % P
    if wires_seed is not None:
        rng = np.random.default_rng(wires_seed)
    wires = field((num_wires, n))
    seen = np.zeros(cells, bool)
    for cell in range(cells):                          # one value per cycle
        if seen[cell]:
            continue
        v, c = wires[cell // n, cell % n], cell
        while not seen[c]:
            seen[c] = True
            wires[c // n, c % n] = v
            c = int(perm[c])
    npp = -(-num_routed // chunk) - 1
    return SimpleNamespace(degree_bits=lg, num_wires=num_wires, num_routed_wires=num_routed, num_challenges=nch, quotient_degree_factor=chunk,
                           num_partial_products=npp, num_constants=0, num_selectors=0, num_gate_constraints=0, gates=[], k_is=k_is,
                           sigmas=sigmas, wires=wires, constants=np.zeros((0, n), np.uint64), public_inputs=[])


def num_terms(desc):
    """T: the permutation terms of the vanishing polynomial"""
    return int(desc.num_challenges) * (int(desc.num_partial_products) + 2)


def perm_quotient(desc, sigma_rows, wires_rows, zs_rows, sub_bits, betas, gammas, alphas, gate_sums=None):
    """glp_perm_quotient_values for one proof: [num_challenges][M].  *_rows row-major [M][columns] on g <W_M>: the sigma columns alone,
    the wires, Zs then partial products.  Terms and order of coset_quotient.quotient_values; gate_sums [num_challenges][M] enters as
    the term of alpha^T."""
    lg = int(desc.degree_bits)
    n, S = 1 << lg, 1 << sub_bits
    M = n * S
    nch, npp = int(desc.num_challenges), int(desc.num_partial_products)
    k_is = [int(k) for k in desc.k_is]
    chunks = _chunks(desc)
    T = num_terms(desc)
    assert len(sigma_rows) == len(wires_rows) == len(zs_rows) == M
    wM, gn, wS = root_of_unity(lg + sub_bits), pow(GEN, n, P), root_of_unity(sub_bits)
    zh_inv = [_inv((gn * pow(wS, r, P) - 1) % P) for r in range(S)]
    out = np.zeros((nch, M), np.uint64)
    x = GEN
    for i in range(M):
        sg = [int(v) for v in sigma_rows[i]]
        lw = [int(v) for v in wires_rows[i]]
        zp = [int(v) for v in zs_rows[i]]
        zn = [int(v) for v in zs_rows[(i + S) % M][:nch]]
        zs, pp = zp[:nch], zp[nch:]
        zh = (gn * pow(wS, i % S, P) - 1) % P
        l0 = zh * _inv((x - 1) * n % P) % P
        terms = [l0 * (zs[k] - 1) % P for k in range(nch)]
        for k in range(nch):
            beta, gamma = int(betas[k]), int(gammas[k])
            for c, ch in enumerate(chunks):
                num = den = 1
                for j in ch:
                    num = num * ((lw[j] + beta * k_is[j] % P * x + gamma) % P) % P
                    den = den * ((lw[j] + beta * sg[j] + gamma) % P) % P
                prev = zs[k] if c == 0 else pp[k * npp + c - 1]
                nxt = zn[k] if c == npp else pp[k * npp + c]
                terms.append((prev * num - nxt * den) % P)
        assert len(terms) == T
        for k in range(nch):
            alpha = int(alphas[k])
            van = 0 if gate_sums is None else int(gate_sums[k][i])
            for v in reversed(terms):
                van = (van * alpha + v) % P
            out[k, i] = van * zh_inv[i % S] % P
        x = x * wM % P
    return out


def gate_sums(desc, cs_rows, wires_rows, alphas, pih):
    """The caller's share: per challenge and coset row, sum_t alpha^t (filtered gate constraint t), [num_challenges][M].  cs_rows
    row-major [M][num_constants (+ anything)], wires_rows [M][num_wires]."""
    nch, nsel, ngc = int(desc.num_challenges), int(desc.num_selectors), int(desc.num_gate_constraints)
    M = len(cs_rows)
    pih = [int(v) for v in pih]
    out = np.zeros((nch, M), np.uint64)
    for i in range(M):
        cs = [int(v) for v in cs_rows[i][:int(desc.num_constants)]]
        lw = [int(v) for v in wires_rows[i]]
        gate_terms = [0] * ngc
        for g in desc.gates:
            s = cs[int(g["selector_index"])]
            filt = 1
            for v in range(int(g["group_start"]), int(g["group_end"])):
                if v != int(g["row"]):
                    filt = filt * (v - s) % P
            if nsel > 1:
                filt = filt * (UNUSED_SELECTOR - s) % P
            for t, v in enumerate(gate_constraints(_Fp, g, cs[nsel:], lw, pih)):
                gate_terms[t] = (gate_terms[t] + filt * v) % P
        for k in range(nch):
            alpha, acc = int(alphas[k]), 0
            for v in reversed(gate_terms):
                acc = (acc * alpha + v) % P
            out[k, i] = acc
    return out
