"""Regenerates tests/golden/*.npz from the CPU oracle (seeded) and the sample circuit hand-off file zkdsa_2_3.glpc.  The oracle itself is pinned by the
reference's Poseidon known-answer vector; see tests/test_oracle_poseidon.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as o  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED_POW = 20261019         # pow_states: Poseidon's stream; Keccak's is + 1, the bits-12 streams + 16


def pow_states(log=print):
    """pow_states.npz: sponge states whose smallest proof-of-work witness lies where the search kernels change path, found by the
    CPU restatement tests/pow_restate.py over seeded random states (tests/test_pow_search.py derives every stored witness again).
    Per hasher one stream of trials: trial t draws 12 field words; words 0..2 are the pending inputs, the candidate goes to slot 3
    (the stored state carries words 9..11 in slots 0..2, which the pending inputs overwrite).
      a     bits 8, witness >= 2048 (two states): past the 8 chunks of 256 candidates that a workgroup which leaves can cover
      c     bits 8, witness exactly 0, 255 and 256: the edges of a chunk
      b     bits 12, witness >= 2^14: past the first launch of the single search"""
    sys.path.insert(0, os.path.dirname(HERE))
    import pow_restate as pr
    o.build()
    out = {}
    for hasher, name in ((pr.POSEIDON, "poseidon"), (pr.KECCAK, "keccak")):
        rows = []           # (kind, state, pending, bits, witness)

        def keep(kind, drawn, bits, w, seed, t, before):
            st = drawn.copy()
            st[:3] = drawn[9:12]
            rows.append((kind, st, drawn[:3].copy(), bits, w))
            log("%s %-4s seed %d trial %5d witness %6d (%d permutations so far)" % (name, kind, seed, t, w, pr.permutations - before))

        # a, c: bits 8
        rng, before = np.random.default_rng(SEED_POW + hasher), pr.permutations
        want = {"a": 2, "c0": 1, "c255": 1, "c256": 1}
        t = 0
        while any(want.values()):
            drawn = o.rand_field(rng, 12)
            try:
                w = pr.smallest_witness(o, hasher, drawn, drawn[:3], 8, 2048)
                kind = {0: "c0", 255: "c255", 256: "c256"}.get(w)
            except ValueError:
                w, kind = None, "a"
            if kind and want[kind]:
                if kind == "a":
                    w = next(c for c in range(2048, 1 << 20) if pr.response(o, hasher, drawn, drawn[:3], c) >> 56 == 0)
                want[kind] -= 1
                keep(kind, drawn, 8, w, SEED_POW + hasher, t, before)
            t += 1
        # b: bits 12, a stream of its own
        rng, before = np.random.default_rng(SEED_POW + 16 + hasher), pr.permutations
        t = 0
        while True:
            drawn = o.rand_field(rng, 12)
            try:
                pr.smallest_witness(o, hasher, drawn, drawn[:3], 12, 1 << 14)
            except ValueError:
                w = next(c for c in range(1 << 14, 1 << 24) if pr.response(o, hasher, drawn, drawn[:3], c) >> 52 == 0)
                keep("b", drawn, 12, w, SEED_POW + 16 + hasher, t, before)
                break
            t += 1
        rows.sort(key=lambda r: r[0])
        out[name + "_kind"] = np.array([r[0] for r in rows])
        out[name + "_state"] = np.stack([r[1] for r in rows])
        out[name + "_pending"] = np.stack([r[2] for r in rows])
        out[name + "_bits"] = np.array([r[3] for r in rows], np.uint32)
        out[name + "_witness"] = np.array([r[4] for r in rows], np.uint64)
    np.savez_compressed(os.path.join(HERE, "pow_states.npz"), **out)


def gpu_proofs(path=None):
    """gpu_proofs.npz: the proofs tests/test_verify_host.py needs and the oracle cannot make (extension-field and recursion gates, salted
    leaves), recorded from glp_prove on a GPU with a fixed salt seed: per circuit of test_verify_host.recorded_circuits its proof and,
    without zero knowledge, the proof of test_verify_host.broken_witness.  The circuits are rebuilt from their seeds by the test."""
    sys.path.insert(0, os.path.dirname(HERE))
    import plonky2_lib_amd as glp
    import test_verify_host as tv
    out = {}
    with glp.Context(0) as ctx:
        ctx.set_salt_seed([11, 22, 33, 44])
        for name, desc in tv.recorded_circuits().items():
            gc = glp.Circuit(ctx, desc)
            out[name + "_proof"] = gc.prove()
            assert gc.verify(out[name + "_proof"])
            if not gc.zero_knowledge:
                out[name + "_broken"] = gc.prove(wires=tv.broken_witness(desc))
                assert not gc.verify(out[name + "_broken"])
            gc.free()
    np.savez_compressed(path or os.path.join(HERE, "gpu_proofs.npz"), **out)


def main():
    if sys.argv[1:] == ["pow_states"]:         # on request only: that file alone, about two minutes of hashing
        return pow_states()
    if sys.argv[1:2] == ["gpu_proofs"]:        # on request only, on a machine with a GPU: that file alone (optionally: where to write it)
        return gpu_proofs(*sys.argv[2:3])
    o.build()
    rng = np.random.default_rng(0x5EED0001)
    vals = o.rand_field(rng, (5, 32))
    b = o.batch_from_values(vals, 3, 2)
    np.savez_compressed(os.path.join(HERE, "batch_5x32.npz"), values=vals, coeffs=b.coeffs, leaves=b.leaves,
                        digests=b.digests, cap=b.cap)
    # one complete proof: the reference's simple-signature circuit [REF src/zkdsa/circuits/mod.rs:24-43] as rebuilt by
    # plonky2_lib_amd.synth.zkdsa_circuit (seeded), proved by the oracle prover
    import plonky2_lib_amd.synth as synth
    desc = synth.zkdsa_circuit(3)
    oc = o.OracleCircuit(desc)
    rc, proof = oc.prove()
    assert rc == 0 and oc.verify(proof) == 0
    np.savez_compressed(os.path.join(HERE, "proof_zkdsa_2_3.npz"), proof=proof, circuit_digest=np.asarray(desc.circuit_digest, np.uint64),
                        constants_sigmas_cap=oc.cs_cap, public_inputs=np.asarray(desc.public_inputs, np.uint64))
    # the same circuit + witness as a circuit hand-off file (include/glp.h, glp_circuit_file_*): what a machine with the Rust
    # builder would ship to the GPU box.  Written by the PRODUCT library's writer (host code, no GPU needed).
    # zkdsa_2_3.glpc is a VERSION 1 file (checksum over the sections only), written by the round-2 library and kept as the
    # fixture of the reader's compatibility path: it is not regenerated.  zkdsa_2_3_v2.glpc is the same content in the current
    # version (checksum over header and sections).
    import plonky2_lib_amd as glp
    glp.write_circuit_file(os.path.join(HERE, "zkdsa_2_3_v2.glpc"), desc, with_witness=True)
    # the 360 Poseidon round constants as data, for the restatements that import nothing from the library or the oracle
    # (tests/limb_gates_restate.py; pinned there to the reference's known-answer vector)
    from oracle.gen_poseidon_constants import all_round_constants
    np.save(os.path.join(HERE, "poseidon_round_constants.npy"), np.array(all_round_constants(), np.uint64))


if __name__ == "__main__":
    main()
