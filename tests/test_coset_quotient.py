"""tests/coset_quotient.py pinned against the oracle prover, on the CPU: the helper's Z / partial products and its quotient,
committed with the oracle's PolynomialBatch, reproduce the `zs_cap` and the `q_cap` of the oracle's proof word for word.  This
is the quotient tests/test_gpu_coset_seam.py sends through glp_batch_lde_values and glp_batch_from_coset_values.  No GPU."""
import numpy as np

import coset_quotient as cq
import zeta_identity as zi


def lde_rows(oracle, coeffs, rate_bits, sub_bits):
    """row-major [M][ncols] values on g <W_M>: every 2^(rate_bits - sub_bits)-th point of oracle.lde"""
    step = 1 << (rate_bits - sub_bits)
    return np.stack([oracle.lde(c, rate_bits)[::step] for c in coeffs], axis=1)


def test_helper_reproduces_the_oracle_provers_caps(oracle):
    desc = cq.seam_circuit(oracle)
    rb, chh = int(desc.rate_bits), int(desc.cap_height)
    sub_bits = int(desc.quotient_degree_factor).bit_length() - 1
    assert 1 << sub_bits == desc.quotient_degree_factor and sub_bits <= rb
    oc = oracle.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0 and oc.verify(proof) == 0
    betas, gammas, alphas, _zeta, pih = zi.challenges(desc, proof, desc.circuit_digest)
    lay, cap = zi.proof_layout(desc), 4 << chh
    # 1. Z and the partial products
    zp = cq.zs_partial_products(desc, desc.wires, betas, gammas)
    zb = oracle.batch_from_values(zp, rb, chh)
    assert (zb.cap.reshape(-1) == proof[lay["zs_cap"]:lay["zs_cap"] + cap]).all()
    # 2. the quotient over oracle.lde of the three oracles' coefficients
    cs_coeffs = [oracle.ifft(v) for v in np.concatenate([np.asarray(desc.constants, np.uint64), np.asarray(desc.sigmas, np.uint64)])]
    w_coeffs = [oracle.ifft(v) for v in np.asarray(desc.wires, np.uint64)]
    rows = [lde_rows(oracle, c, rb, sub_bits) for c in (cs_coeffs, w_coeffs, zb.coeffs)]
    q = cq.quotient_values(desc, rows[0], rows[1], rows[2], sub_bits, betas, gammas, alphas, pih)
    assert q.shape == (desc.num_challenges, (1 << desc.degree_bits) << sub_bits)
    # 3. coset_ifft, chunks, from_coeffs   4. the cap
    qb = oracle.batch_from_coeffs(cq.chunk_coeffs(oracle, q, sub_bits), rb, chh)
    assert (qb.cap.reshape(-1) == proof[lay["q_cap"]:lay["q_cap"] + cap]).all()
