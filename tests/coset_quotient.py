"""A quotient computed outside the library: plonky2's `compute_quotient_polys` (plonk/prover.rs) and
`wires_permutation_partial_products_and_zs` restated over the base field in plain Python integers.

The gate bodies, the field and the transcript are those of tests/zeta_identity.py (`gate_constraints` is generic in the field:
there it runs on openings at zeta, here on one row of LDE values).  Everything else is restated here: Z and the partial products
on H from the wires and the sigmas, and the quotient's values on the coset g <W_M>, M = n * 2^sub_bits, from ROW-MAJOR LDE rows of
the three oracles, which is the layout `PolynomialBatch::get_lde_values(i, step)` hands the Rust loop and glp_batch_lde_values
serves.  tests/test_coset_quotient.py pins both against the oracle prover's caps before any GPU sees them."""
import numpy as np

from zeta_identity import gate_constraints, _Fp, UNUSED_SELECTOR, challenges  # noqa: F401  (challenges: re-exported for the tests)

P = 0xFFFFFFFF00000001
GEN = 7                          # the coset shift: F::coset_shift()
POW2_GEN = 1753635133440165772   # primitive_root_of_unity(32) of the Goldilocks field


def root_of_unity(lg):
    r = POW2_GEN
    for _ in range(lg, 32):
        r = r * r % P
    return r


def _inv(a):
    return pow(a, P - 2, P)


def seam_circuit(oracle):
    """the circuit both seam tests prove: the family tests/test_ext_gates.py proves with the oracle, every gate of it in
    zeta_identity.gate_constraints"""
    import plonky2_lib_amd.synth as synth
    pi = [9, 1 << 50]
    return synth.arith_circuit(4, synth.Config.standard_recursion_config(), seed=22, public_inputs=pi, pi_hash=oracle.hash_no_pad(pi))


def _chunks(desc):
    """the routed wires in chunks of quotient_degree_factor: num_partial_products + 1 of them"""
    nr, qdf = int(desc.num_routed_wires), int(desc.quotient_degree_factor)
    ch = [range(c, min(c + qdf, nr)) for c in range(0, nr, qdf)]
    assert len(ch) == int(desc.num_partial_products) + 1
    return ch


def zs_partial_products(desc, wires, betas, gammas):
    """Values on H of the partial_products_and_zs oracle, [num_challenges * (1 + num_partial_products)][n]: the Z of every
    challenge first, then each challenge's partial products (plonk/prover.rs `all_wires_permutation_partial_products`)."""
    lg = int(desc.degree_bits)
    n, nch, npp = 1 << lg, int(desc.num_challenges), int(desc.num_partial_products)
    k_is = [int(k) for k in desc.k_is]
    w = [[int(v) for v in col] for col in np.asarray(wires)[:int(desc.num_routed_wires)]]
    sg = [[int(v) for v in col] for col in np.asarray(desc.sigmas)]
    chunks = _chunks(desc)
    out = np.zeros((nch * (1 + npp), n), np.uint64)
    wn = root_of_unity(lg)
    for i in range(nch):
        beta, gamma = int(betas[i]), int(gammas[i])
        z, x = 1, 1
        for row in range(n):
            out[i, row] = z
            for c, ch in enumerate(chunks):
                num = den = 1
                for j in ch:
                    num = num * ((w[j][row] + beta * k_is[j] % P * x + gamma) % P) % P
                    den = den * ((w[j][row] + beta * sg[j][row] + gamma) % P) % P
                z = z * num % P * _inv(den) % P
                if c < npp:
                    out[nch + i * npp + c, row] = z
            x = x * wn % P
        assert z == 1, "the permutation argument does not close: Z(g^n) != 1"
    return out


def quotient_values(desc, cs_rows, wires_rows, zs_rows, sub_bits, betas, gammas, alphas, pih):
    """`compute_quotient_polys`: the quotient's values [num_challenges][M] on the coset g <W_M>, natural order.
    *_rows are row-major [M][columns]: row i holds the oracle's polynomials at g W_M^i (constants then sigmas; wires; Zs then
    partial products); the "next" row of Z is (i + 2^sub_bits) mod M.  Terms in plonky2's order (`eval_vanishing_poly_base_batch`):
    L_0 (Z - 1) per challenge, the partial-product chunk checks per challenge, the filtered gate constraints; reduced by powers
    of alpha_i and divided by Z_H(x) = x^n - 1."""
    F = _Fp
    lg = int(desc.degree_bits)
    n, S = 1 << lg, 1 << sub_bits
    M = n * S
    nch, npp, nc, nr = int(desc.num_challenges), int(desc.num_partial_products), int(desc.num_constants), int(desc.num_routed_wires)
    nsel, ngc = int(desc.num_selectors), int(desc.num_gate_constraints)
    k_is = [int(k) for k in desc.k_is]
    chunks = _chunks(desc)
    pih = [int(v) for v in pih]
    assert len(cs_rows) == len(wires_rows) == len(zs_rows) == M
    wM, gn, wS = root_of_unity(lg + sub_bits), pow(GEN, n, P), root_of_unity(sub_bits)
    zh_inv = [_inv((gn * pow(wS, r, P) - 1) % P) for r in range(S)]        # Z_H(g W_M^i) = g^n w_S^(i mod S) - 1: S values
    out = np.zeros((nch, M), np.uint64)
    x = GEN
    for i in range(M):
        row0 = [int(v) for v in cs_rows[i]]
        cs, sg = row0[:nc], row0[nc:nc + nr]
        lw = [int(v) for v in wires_rows[i]]
        zp = [int(v) for v in zs_rows[i]]
        zn = [int(v) for v in zs_rows[(i + S) % M][:nch]]
        zs, pp = zp[:nch], zp[nch:]
        zh = (gn * pow(wS, i % S, P) - 1) % P
        l0 = zh * _inv((x - 1) * n % P) % P                                # L_0(x) = (x^n - 1) / (n (x - 1))
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
        gate_terms = [0] * ngc
        for g in desc.gates:
            s = cs[int(g["selector_index"])]
            filt = 1
            for v in range(int(g["group_start"]), int(g["group_end"])):
                if v != int(g["row"]):
                    filt = filt * (v - s) % P
            if nsel > 1:
                filt = filt * (UNUSED_SELECTOR - s) % P
            for t, v in enumerate(gate_constraints(F, g, cs[nsel:], lw, pih)):
                gate_terms[t] = (gate_terms[t] + filt * v) % P
        terms += gate_terms
        for k in range(nch):
            alpha, van = int(alphas[k]), 0
            for v in reversed(terms):
                van = (van * alpha + v) % P
            out[k, i] = van * zh_inv[i % S] % P
        x = x * wM % P
    return out


def chunk_coeffs(oracle, q_values, sub_bits):
    """the tail of `prove_with_partition_witness` on the CPU: coset_ifft(g) per polynomial, then chunks of n coefficients"""
    q_values = np.asarray(q_values, np.uint64)
    n = q_values.shape[1] >> sub_bits
    return np.concatenate([oracle.coset_ifft(q, GEN).reshape(1 << sub_bits, n) for q in q_values])
