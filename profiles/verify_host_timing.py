"""The host-side cost of the verifier and of circuit creation, for one build of the library: the figures of profiles/r29_verify_host.txt,
taken when the verifier's host half moved into device-free headers (csrc/verify_host.h, csrc/circuit_common.h) to show that the move
changed none of them.

  python profiles/verify_host_timing.py [--root TREE] [--reps 9] [--verify-log-n 20]

TREE: the checkout whose library is measured (default: this one); run it for two trees in alternation, a fresh process each.
  create      glp_circuit_create of synth.ecdsa_shape_circuit(16): description checks, uploads, constants/sigmas commitment
  verify      glp_verify on the proof of synth.ecdsa_shape_circuit(--verify-log-n), the shape of bench.py's circuit
  batch-dev   glp_verify_batch on K = 256 zkdsa proofs (2^3 rows), transcripts on the device
  batch-host  the same with GLP_VERIFY_HOST_TRANSCRIPT=1
Wall times in ms, host clock around the call, median (min .. max) of --reps calls after one warm-up call.  The last call of each batch
form runs with GLP_BATCH_TRACE=1: the library's own spans go to stderr."""
import argparse
import os
import statistics
import sys
import time

import numpy as np


def timed(f, reps, warm=1):
    for _ in range(warm):
        f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append(1e3 * (time.perf_counter() - t0))
    return "%9.3f ms  (%.3f .. %.3f, %d calls)" % (statistics.median(ms), min(ms), max(ms), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--verify-log-n", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import plonky2_lib_amd as glp
    import plonky2_lib_amd.synth as synth
    tag = os.path.abspath(a.root)
    with glp.Context(0) as ctx:
        d16 = synth.ecdsa_shape_circuit(16, seed=3)
        made = []

        def create():
            if made:
                made.pop().free()
            made.append(glp.Circuit(ctx, d16))
        print("%s  create      2^16 rows        %s" % (tag, timed(create, min(a.reps, 5))), flush=True)
        made.pop().free()

        big = synth.ecdsa_shape_circuit(a.verify_log_n, seed=3)
        gc = glp.Circuit(ctx, big)
        proof = gc.prove()
        assert gc.verify(proof)
        print("%s  verify      2^%d rows        %s" % (tag, a.verify_log_n, timed(lambda: gc.verify(proof), a.reps)), flush=True)
        gc.free()
        del big

        z = synth.zkdsa_circuit(3)
        gz = glp.Circuit(ctx, z)
        batch = np.tile(gz.prove(), (256, 1))
        for name, env in (("batch-dev ", None), ("batch-host", "1")):
            if env:
                os.environ["GLP_VERIFY_HOST_TRANSCRIPT"] = env
            assert gz.verify_batch(batch).all()
            print("%s  %s  K = 256, 2^3 rows %s" % (tag, name, timed(lambda: gz.verify_batch(batch), a.reps)), flush=True)
            os.environ["GLP_BATCH_TRACE"] = "1"
            sys.stderr.write("%s  %s  " % (tag, name))
            sys.stderr.flush()
            gz.verify_batch(batch)
            del os.environ["GLP_BATCH_TRACE"]
            os.environ.pop("GLP_VERIFY_HOST_TRANSCRIPT", None)
        gz.free()


if __name__ == "__main__":
    main()
