"""One independent map of where every word of a proof lives, written from the layout documented in include/glp.h (glp_prove's
`proof_out`, glp_fri_proof, GLP_CIRCUIT_ZERO_KNOWLEDGE) and from nothing else: no GPU, no library call, no `Layout` read back.

`sections(desc)` maps a circuit description to the named word ranges of its proof, head and every query round;
`fri_sections(...)` does the same for a bare FriProof (the tail of a proof, which the FRI seam verifies on its own).  The ranges
come in proof order and tile the proof: the first starts at word 0, each starts where the one before ends, the last ends at the
proof's length.  Empty ranges (a path of depth 0) are left out.

For the words that follow the last challenge of the transcript (query leaves, salts, paths, fold evaluations) `reasons(sec)` gives
the rejection reasons plonky2's order of checks allows when one word of the section is damaged alone (fri/verifier.rs
`fri_verifier_query_round`: the initial trees in order, then per reduction the consistency check, the interpolation, the layer's
Merkle path):
    leaf, salt or initial-path word of oracle k in round q   exactly "Invalid Merkle proof (query q, initial tree k)"
    fold-evaluation word of reduction r in round q           "FRI consistency check failed (query q, reduction r)" for the two words
                                                             of the slot x_index & (arity - 1), else "Invalid Merkle proof (query q,
                                                             reduction r)": the leaf of the layer tree no longer hashes to its path
    layer-path word of reduction r in round q                exactly "Invalid Merkle proof (query q, reduction r)"
Head words (caps, openings, layer caps, final polynomial, witness, public inputs) enter the transcript: damage moves every later
challenge and whichever check comes first rejects, so the map names no reason for them (`reasons` returns None)."""
from collections import namedtuple

SALT_SIZE = 4
P = 0xFFFFFFFF00000001

# kind: wires_cap zs_cap quotient_cap openings layer_cap | leaf salt path evals layer_path | final_poly pow public_inputs
# q: query round or None (head); index: oracle for leaf / salt / path, reduction for layer_cap / evals / layer_path, else None
Section = namedtuple("Section", "name kind lo hi q index")

QUERY_KINDS = ("leaf", "salt", "path", "evals", "layer_path")
DIGEST_KINDS = ("wires_cap", "zs_cap", "quotient_cap", "layer_cap", "path", "layer_path")      # [count][4] digests


def oracle_cols(desc):
    """polynomials of the four initial oracles: constants ++ sigmas, wires, Zs ++ partial products, quotient chunks"""
    nch = int(desc.num_challenges)
    return [int(desc.num_constants) + int(desc.num_routed_wires), int(desc.num_wires), nch * (1 + int(desc.num_partial_products)),
            nch * int(desc.quotient_degree_factor)]


class _Walk:
    def __init__(self, base):
        self.at, self.out = base, []

    def add(self, name, kind, count, q=None, index=None):
        if count > 0:
            self.out.append(Section(name, kind, self.at, self.at + count, q, index))
        self.at += count


def fri_sections(ncols, salted, log_n, rate_bits, cap_height, arity_bits, num_query_rounds, base=0):
    """glp_fri_proof: commit_phase_merkle_caps | query_round_proofs | final_poly | pow_witness, starting at word `base`.
    ncols / salted: per oracle, the polynomials of a leaf and whether 4 salts follow them."""
    w = _Walk(base)
    capw, lgN = 4 << cap_height, log_n + rate_bits
    for r in range(len(arity_bits)):
        w.add("layer_cap%d" % r, "layer_cap", capw, None, r)
    for q in range(num_query_rounds):
        for k, (c, s) in enumerate(zip(ncols, salted)):
            w.add("q%d_leaf%d" % (q, k), "leaf", c, q, k)
            w.add("q%d_salt%d" % (q, k), "salt", SALT_SIZE if s else 0, q, k)
            w.add("q%d_path%d" % (q, k), "path", 4 * (lgN - cap_height), q, k)
        lg = lgN
        for r, ab in enumerate(arity_bits):
            lg -= ab
            w.add("q%d_step%d_evals" % (q, r), "evals", 2 << ab, q, r)
            w.add("q%d_step%d_path" % (q, r), "layer_path", 4 * (lg - cap_height), q, r)
    w.add("final_poly", "final_poly", 2 << (log_n - sum(arity_bits)))
    w.add("pow", "pow", 1)
    return w.out


def sections(desc, zk=None):
    """glp_prove's proof_out for the circuit `desc`; zk (default: desc.zero_knowledge): leaves of oracles 1..3 end with 4 salts"""
    zk = bool(getattr(desc, "zero_knowledge", False)) if zk is None else bool(zk)
    cols = oracle_cols(desc)
    capw = 4 << int(desc.cap_height)
    w = _Walk(0)
    w.add("wires_cap", "wires_cap", capw)
    w.add("zs_cap", "zs_cap", capw)
    w.add("quotient_cap", "quotient_cap", capw)
    w.add("openings", "openings", 2 * (sum(cols) + int(desc.num_challenges)))         # every polynomial at zeta, the Zs at g zeta too
    tail = fri_sections(cols, [False] + [zk] * 3, int(desc.degree_bits), int(desc.rate_bits), int(desc.cap_height),
                        [int(a) for a in desc.reduction_arity_bits], int(desc.num_query_rounds), base=w.at)
    w.out += tail
    w.at = tail[-1].hi
    w.add("public_inputs", "public_inputs", len(desc.public_inputs))
    return w.out


def total_words(secs):
    return secs[-1].hi


def tiles(secs, total):
    """first word 0, last word `total`, no gap, no overlap, nothing empty"""
    return (secs[0].lo == 0 and secs[-1].hi == total and all(a.hi == b.lo for a, b in zip(secs, secs[1:]))
            and all(s.hi > s.lo for s in secs))


def section_of(secs):
    """list: word -> index into secs"""
    out = []
    for i, s in enumerate(secs):
        out += [i] * (s.hi - s.lo)
    return out


def reasons(sec):
    """the rejection reasons plonky2's check order allows when one word of `sec` is damaged alone; None for head words"""
    merkle0 = "Invalid Merkle proof (query %s, initial tree %s)" % (sec.q, sec.index)
    merkle = "Invalid Merkle proof (query %s, reduction %s)" % (sec.q, sec.index)
    fold = "FRI consistency check failed (query %s, reduction %s)" % (sec.q, sec.index)
    return {"leaf": (merkle0,), "salt": (merkle0,), "path": (merkle0,), "evals": (fold, merkle), "layer_path": (merkle,)}.get(sec.kind)


def fold_reason(sec):
    return "FRI consistency check failed (query %s, reduction %s)" % (sec.q, sec.index)


def sample(secs, stride, kinds=None):
    """sorted words: the first and last word of every section (of the kinds asked for) plus every stride-th word of them"""
    out = set()
    for s in secs:
        if kinds is None or s.kind in kinds:
            out.update((s.lo, s.hi - 1))
            out.update(range(s.lo + (-s.lo) % stride, s.hi, stride))
    return sorted(out)


def bumped(word):
    """the damage of the sweeps: w -> w + 1 mod p"""
    return (int(word) + 1) % P


def legacy_ranges(desc):
    """{name: (lo, hi)} in the order and with the names tests/test_gpu_verify_batch.py has always picked its tampers from: the head
    sections, every section of query round 0, the wires leaf of the last round, then the tail"""
    secs = sections(desc, zk=False)
    by = {s.name: (s.lo, s.hi) for s in secs}
    nq = int(desc.num_query_rounds)
    o = {k: by[k] for k in ("wires_cap", "zs_cap", "quotient_cap", "openings") if k in by}
    caps = [s for s in secs if s.kind == "layer_cap"]
    if caps:
        o["fri_caps"] = (caps[0].lo, caps[-1].hi)
    for s in secs:
        if s.q == 0:
            o[s.name] = (s.lo, s.hi)
    o["qlast_leaf1"] = by["q%d_leaf1" % (nq - 1)]
    for k in ("final_poly", "pow", "public_inputs"):
        if k in by:
            o[k] = by[k]
    return o
