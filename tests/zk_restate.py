"""Independent restatements for the zero-knowledge tests (test_zk.py, test_gpu_zk.py): the salt PRF of include/glp.h over the
oracle's Poseidon, the salted proof layout, and salt stripping (a zk proof minus its salts is a proof in the non-zk layout)."""
import numpy as np

SALT_SIZE = 4
TAG_WIRES, TAG_ZS, TAG_QUOTIENT, TAG_BATCH = 0, 1, 2, 3
P = 0xFFFFFFFF00000001


def salt(oracle, seed, tag, leaf, k=0):
    """salt(seed, tag, leaf)[0..4) = Poseidon([seed0, seed1, seed2, seed3 + k mod p, tag, leaf lo32, leaf hi32, 0 x 5])[0..4)"""
    s = [int(x) % P for x in seed]
    st = np.array([s[0], s[1], s[2], (s[3] + k) % P, tag, leaf & 0xFFFFFFFF, leaf >> 32, 0, 0, 0, 0, 0], np.uint64)
    return oracle.poseidon_permute(st)[:4]


def salt_columns(oracle, seed, tag, nleaves, k=0):
    """[nleaves][4]: the salts of every leaf"""
    return np.stack([salt(oracle, seed, tag, j, k) for j in range(nleaves)])


def oracle_cols(desc):
    nch = int(desc.num_challenges)
    return [int(desc.num_constants) + int(desc.num_routed_wires), int(desc.num_wires),
            nch * (1 + int(desc.num_partial_products)), nch * int(desc.quotient_degree_factor)]


def layout(desc, zk):
    """(queries offset, query stride, [(leaf offset in the record, leaf_len, path offset)] x 4, total words) of a proof"""
    cap = 4 << int(desc.cap_height)
    nch = int(desc.num_challenges)
    nopen = (int(desc.num_constants) + int(desc.num_routed_wires) + int(desc.num_wires) + 2 * nch + nch * int(desc.num_partial_products)
             + nch * int(desc.quotient_degree_factor))
    lg = int(desc.degree_bits) + int(desc.rate_bits)
    depth0 = lg - int(desc.cap_height)
    queries = 3 * cap + 2 * nopen + len(desc.reduction_arity_bits) * cap
    oracles, o = [], 0
    for k, c in enumerate(oracle_cols(desc)):
        ll = c + (SALT_SIZE if zk and k > 0 else 0)
        oracles.append((o, ll, o + ll))
        o += ll + 4 * depth0
    for ab in desc.reduction_arity_bits:
        lg -= ab
        o += 2 * (1 << ab) + 4 * (lg - int(desc.cap_height))
    final_len = 1 << (lg - int(desc.rate_bits))
    total = queries + o * int(desc.num_query_rounds) + 2 * final_len + 1 + len(desc.public_inputs)
    return queries, o, oracles, total


def proof_words(desc, zk):
    return layout(desc, zk)[3]


def strip_salts(desc, proof):
    """the zk proof without the 4 salt words of each blinded leaf: a proof in the non-zk layout (its Merkle paths still commit to the
    salted leaves)"""
    proof = np.asarray(proof, np.uint64)
    q0, stride, oracles, total = layout(desc, True)
    assert proof.size == total
    keep = np.ones(total, bool)
    for q in range(int(desc.num_query_rounds)):
        for k, (lo, ll, _) in enumerate(oracles):
            if k > 0:
                keep[q0 + q * stride + lo + ll - SALT_SIZE:q0 + q * stride + lo + ll] = False
    return proof[keep]


def query_leaves(desc, proof, zk):
    """per query round: [(leaf words, path [depth][4])] for the four initial oracles"""
    proof = np.asarray(proof, np.uint64)
    q0, stride, oracles, _ = layout(desc, zk)
    depth0 = int(desc.degree_bits) + int(desc.rate_bits) - int(desc.cap_height)
    out = []
    for q in range(int(desc.num_query_rounds)):
        base = q0 + q * stride
        out.append([(proof[base + lo:base + lo + ll], proof[base + po:base + po + 4 * depth0].reshape(-1, 4)) for lo, ll, po in oracles])
    return out
