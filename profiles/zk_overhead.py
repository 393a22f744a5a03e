"""Cost of zero-knowledge proving (GLP_CIRCUIT_ZERO_KNOWLEDGE): a blinded circuit proved with salts against the same blinded circuit
proved without them, so that the difference is the salted commitments alone.

  python profiles/zk_overhead.py headline   # 10-signature secp256k1 circuit, 2^20 rows, one proof from an HBM-resident witness
  python profiles/zk_overhead.py batch      # zk zkdsa circuit (2^14 rows), glp_prove_batch + glp_verify_batch at K = 64 and 256

Prints per-stage device times (glp_ctx stage events; the `salt` rows are the k_salt_lde launches) and wall times."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonky2_lib_amd as glp                      # noqa: E402
import plonky2_lib_amd.synth as synth             # noqa: E402

COMMITS = ("wires", "zs_partial_products", "quotient_chunks")


def plain_twin(desc):
    class D:
        pass
    d = D()
    d.__dict__.update(desc.__dict__)
    d.zero_knowledge = False
    return d


def labelled(stages):
    """stage list of one proof -> [(commitment/stage, ms)]: commitment stages are named after the oracle they build"""
    out, k = [], 0
    for name, ms, _ in stages:
        if name in ("intt", "lde", "salt", "merkle_leaves", "merkle_levels", "copy_coeffs") and k < 3:
            out.append(("%s/%s" % (COMMITS[k], name), ms))
            if name == "merkle_levels":
                k += 1
        else:
            out.append((name, ms))
    return out


def sums(rows):
    d = {}
    for k, ms in rows:
        d[k] = d.get(k, 0.0) + ms
    return d


def headline():
    from plonky2_lib_amd import gadgets_ecdsa as E
    t = time.time()
    desc = E.ecdsa_circuit(E.random_signatures(10, seed=0), config=synth.Config.standard_ecc_config(zero_knowledge=True))
    print("built 2^%d rows (%d gate rows + blinding) in %.1f s" % (desc.degree_bits, desc.gadget_rows, time.time() - t), flush=True)
    res = {}
    with glp.Context(0) as ctx:
        ctx.set_salt_seed([1, 2, 3, 4])
        w = np.ascontiguousarray(desc.wires)
        dp = ctx.dev_alloc(w.nbytes)
        ctx.dev_upload(dp, w)
        for tag, d in (("zk", desc), ("plain", plain_twin(desc))):
            gc = glp.Circuit(ctx, d)
            for _ in range(3):
                gc.prove_device(dp)
            ts = []
            for _ in range(10):
                ctx.synchronize()
                t0 = time.perf_counter()
                proof = gc.prove_device(dp)
                ts.append((time.perf_counter() - t0) * 1e3)
            ctx.set_profiling(True)
            ctx.stage_reset()
            gc.prove_device(dp)
            res[tag] = (sorted(ts)[len(ts) // 2], min(ts), sums(labelled(ctx.stages())))
            ctx.set_profiling(False)
            assert gc.verify(proof)
            print("%-5s proof: median %.2f ms, min %.2f ms over 10, %d words, verified" % (tag, res[tag][0], res[tag][1], proof.size), flush=True)
            gc.free()
        ctx.dev_free(dp)
    zk, pl = res["zk"][2], res["plain"][2]
    print("%-40s %10s %10s %8s" % ("stage (one profiled proof)", "zk ms", "plain ms", "delta"))
    for k in list(zk) + [k for k in pl if k not in zk]:
        a, b = zk.get(k, 0.0), pl.get(k, 0.0)
        print("%-40s %10.3f %10.3f %+8.3f" % (k, a, b, a - b))
    a, b = sum(zk.values()), sum(pl.values())
    print("%-40s %10.3f %10.3f %+8.3f (%+.1f %%)" % ("sum of stages", a, b, a - b, 100 * (a - b) / b))
    print("wall median: zk %.2f ms, plain %.2f ms: %+.1f %%" % (res["zk"][0], res["plain"][0], 100 * (res["zk"][0] / res["plain"][0] - 1)))


def batch():
    desc = synth.zkdsa_circuit(config=synth.Config.standard_recursion_zk_config())
    print("zk zkdsa: 2^%d rows" % desc.degree_bits, flush=True)
    with glp.Context(0) as ctx:
        ctx.set_salt_seed([1, 2, 3, 4])
        for K in (64, 256):
            wires = np.ascontiguousarray(np.broadcast_to(desc.wires, (K,) + desc.wires.shape))
            pis = np.ascontiguousarray(np.broadcast_to(desc.public_inputs, (K,) + desc.public_inputs.shape))
            dp = ctx.dev_alloc(wires.nbytes)                  # HBM-resident witnesses: the upload is the same for both and is left out
            ctx.dev_upload(dp, wires)
            del wires
            for tag, d in (("zk", desc), ("plain", plain_twin(desc))):
                gc = glp.Circuit(ctx, d)
                out = gc.prove_batch_device(dp, K, pis)
                tp, tv = [], []
                for _ in range(5):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    out = gc.prove_batch_device(dp, K, pis)
                    t1 = time.perf_counter()
                    ok = gc.verify_batch(out)
                    t2 = time.perf_counter()
                    assert ok.all()
                    tp.append((t1 - t0) * 1e3); tv.append((t2 - t1) * 1e3)
                mp, mv = sorted(tp)[2], sorted(tv)[2]
                print("K=%3d %-5s prove_batch %8.2f ms (%7.0f proofs/s)  verify_batch %7.2f ms  all verified" % (K, tag, mp, K / mp * 1e3, mv),
                      flush=True)
                ctx.set_profiling(True)
                ctx.stage_reset()
                gc.prove_batch_device(dp, K, pis)
                st = sums(labelled(ctx.stages()))
                ctx.set_profiling(False)
                print("      stages: " + ", ".join("%s %.2f" % (k, v) for k, v in st.items() if v >= 0.05), flush=True)
                gc.free()
            ctx.dev_free(dp)


if __name__ == "__main__":
    {"headline": headline, "batch": batch}[sys.argv[1]]()
