"""The `verify_queries` stage of glp_verify_batch on one shape, for comparing two builds of the library (profiles/r15_verify_one_kernel.txt).

  python profiles/verify_queries_timing.py <tree root> <label> <shape> <proof cache dir> [--reps 9] [--wall 40]

One process measures one build: the library is imported from <tree root> (a checkout with its own libglprover.so), so two builds are
compared by running this script once per tree, alternating.  The proofs are proved by the first process that needs them and kept
in <proof cache dir>; every later process, of either build, verifies those same words.
  zkdsa256    256 proofs of the zkdsa circuit (2^3 rows, no reduction, depth-2 paths)
  smt10x256   256 proofs of synth.smt_shape_circuit(10, seed=9) (two arity-16 reductions)
  headline    the one 2^16-row, 136-wire proof of tests/test_gpu_verify_batch.py::test_headline_shape_proof (depth-15 paths, wide leaves)
Stage time: hipEvent pair with profiling on, --reps calls after two warm-up calls.  Wall time of the whole call: profiling off, host
clock, --wall calls after two.  One JSON line; a batch with one damaged member is checked last, its reason goes into the line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("root")
ap.add_argument("label")
ap.add_argument("shape", choices=["zkdsa256", "smt10x256", "headline"])
ap.add_argument("cache")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--wall", type=int, default=40)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import numpy as np                                  # noqa: E402
import plonky2_lib_amd as glp                       # noqa: E402
import plonky2_lib_amd.synth as synth              # noqa: E402

assert os.path.abspath(glp.__file__).startswith(os.path.abspath(a.root)), glp.__file__
make, K = {"zkdsa256": (lambda: synth.zkdsa_circuit(3), 256), "smt10x256": (lambda: synth.smt_shape_circuit(10, seed=9), 256),
           "headline": (lambda: synth.arith_circuit(16, synth.Config.standard_ecc_config(), seed=16), 1)}[a.shape]
desc = make()
ctx = glp.Context(0)
gc = glp.Circuit(ctx, desc)
path = os.path.join(a.cache, a.shape + ".npy")
if os.path.exists(path):
    proofs = np.load(path)
else:
    proofs = gc.prove_batch(np.stack([desc.wires] * K), np.stack([desc.public_inputs] * K)) if K > 1 else gc.prove()[None, :]
    os.makedirs(a.cache, exist_ok=True)
    np.save(path, proofs)
assert proofs.shape == (K, gc.proof_words)
ctx.set_profiling(True)
stage = []
for i in range(a.reps + 2):
    ctx.stage_reset()
    assert gc.verify_batch(proofs).all()
    ms = [m for n, m, _ in ctx.stages() if n == "verify_queries"]
    assert len(ms) == 1, ctx.stages()
    if i >= 2:
        stage.append(ms[0])
ctx.set_profiling(False)
wall = []
for i in range(a.wall + 2):
    t0 = time.perf_counter()
    gc.verify_batch(proofs)
    if i >= 2:
        wall.append((time.perf_counter() - t0) * 1e3)
bad = proofs.copy()
bad[K - 1, proofs.shape[1] // 2] ^= np.uint64(1)
ok, why = gc.verify_batch(bad, reasons=True)
assert not ok[K - 1] and ok.sum() == K - 1
print(json.dumps({"build": a.label, "shape": a.shape, "K": K, "words": int(gc.proof_words),
                  "stage_ms": {"median": round(float(np.median(stage)), 4), "min": round(min(stage), 4), "max": round(max(stage), 4)},
                  "wall_ms": {"median": round(float(np.median(wall)), 4), "min": round(min(wall), 4), "max": round(max(wall), 4)},
                  "reason_of_damaged": why[K - 1]}))
gc.free()
ctx.close()
