"""The caller's-quotient seam on the clock: glp_batch_lde_values against a plain copy, glp_batch_from_coset_values against the commit
it ends in.

    python -m plonky2_lib_amd.tools.coset_seam_timing [--out profiles/r12_coset_seam.txt] [--reps 7] [--log-n 20]
    (from the repository root: python plonky2-lib_amd/tools/coset_seam_timing.py)

Two shapes: "wires" (136 columns, 2^20 rows, rate_bits = sub_bits = 3: the headline circuit's widest oracle) and "zkdsa x256" (the
circuit of `bench.py --workload zkdsa-batch`: 2^3 rows, 256 proofs in one many-proof batch; 135 wire columns for the reads, the
quotient oracle's 2 x 8 chunks for the commit).  All inputs are filled on the device (glp_fill_random_device).

LDE reads, device to device (out_on_device = 1), whole coset: row-major and column-major, against hipMemcpyAsync device-to-device of
the same number of bytes on the same stream (what a transpose can approach: it reads and writes every byte once, as the copy does).
k_lde_to_natural, the accessor's permutation that was there before, is reachable only inside glp_lde, between a host-to-device and a
device-to-host copy; it is the column-major kernel's permutation at sub_bits = rate_bits, so that row stands in for it, and glp_lde is
timed once on 16 columns to show what its host round trip costs.

Coset commit: glp_batch_from_coset_values (values in HBM) against glp_batch_from_coeffs_device / glp_batch_many_from_coeffs on the
same num_polys << sub_bits columns.  The difference is the de-interleave, the per-plane inverse transform and k_quotient_combine.

Every figure: hipEvent pairs on the ctx stream around the call, 2 warm-up calls, then --reps repetitions; median and (min..max)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import plonky2_lib_amd as glp                    # noqa: E402
from plonky2_lib_amd import binding              # noqa: E402


def _hip():
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not found")


class Timer:
    """hipEvent pairs on one stream"""

    def __init__(self, stream):
        self.hip, self.stream = _hip(), C.c_void_p(stream)
        self.beg, self.end = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.beg)) == 0 and self.hip.hipEventCreate(C.byref(self.end)) == 0

    def ms(self, fn):
        assert self.hip.hipEventRecord(self.beg, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.end, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.end) == 0
        t = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(t), self.beg, self.end) == 0
        return float(t.value)

    def series(self, fn, reps, warm=2):
        for _ in range(warm):
            self.ms(fn)
        return [self.ms(fn) for _ in range(reps)]

    def copy_d2d(self, dst, src, nbytes):
        assert self.hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3, self.stream) == 0     # hipMemcpyDeviceToDevice


def fmt(ts, nbytes=None):
    med = float(np.median(ts))
    s = "%10.3f ms (%.3f..%.3f)" % (med, min(ts), max(ts))
    if nbytes:
        s += "  %7.1f GB/s read + written" % (2 * nbytes / med / 1e6)
    return s


def lde_reads(ctx, tm, lines, name, K, ncols, log_n, rb, reps):
    L = glp.load_library()
    n, sub = 1 << log_n, rb
    M = n << sub
    words = K * ncols * n
    src = ctx.dev_alloc(words * 8)
    ctx.fill_random_device(src, words, 12)
    h = C.c_void_p()
    if K == 1:
        binding._chk(L.glp_batch_from_values_device(ctx._h, C.c_void_p(src), ncols, log_n, rb, 4, C.byref(h)))
    else:
        binding._chk(L.glp_batch_many_from_values(ctx._h, C.c_void_p(src), 1, K, ncols, log_n, rb, 4, 0, None, C.byref(h)))
    ctx.synchronize()
    ctx.dev_free(src)
    nbytes = K * ncols * M * 8
    out, out2 = ctx.dev_alloc(nbytes), ctx.dev_alloc(nbytes)
    lines.append("%s: K = %d, %d columns, 2^%d rows, rate_bits = sub_bits = %d: %.1f MB out" % (name, K, ncols, log_n, rb, nbytes / 1e6))
    med = {}
    for label, layout in (("lde_values row-major", glp.LDE_ROW_MAJOR), ("lde_values col-major", glp.LDE_COL_MAJOR)):
        ts = tm.series(lambda: binding._chk(L.glp_batch_lde_values(h, 0, ncols, sub, 0, M, layout, C.c_void_p(out), 1)), reps)
        lines.append("    %-32s %s" % (label, fmt(ts, nbytes)))
        med[layout] = float(np.median(ts))
    ts = tm.series(lambda: tm.copy_d2d(out2, out, nbytes), reps)
    lines.append("    %-32s %s" % ("hipMemcpyAsync device-to-device", fmt(ts, nbytes)))
    # what bounds the row-major form: the floor of one call (one row of one column through the same kernel: a launch and one
    # load-store round trip), and how much of the tiles the shape fills (ntt.hip: 4096-word tiles as tall as the coset, 16..128 rows)
    floor = float(np.median(tm.series(lambda: binding._chk(L.glp_batch_lde_values(h, 0, 1, sub, 0, 1, glp.LDE_ROW_MAJOR, C.c_void_p(out), 1)), reps)))
    tr = 1 << min(7, max(4, log_n + sub))
    tc = 4096 // tr
    fill = (ncols * M) / float(-(-ncols // tc) * tc * -(-M // tr) * tr)
    copy, row = float(np.median(ts)), med[glp.LDE_ROW_MAJOR]
    lines.append("    %-32s %10.3f ms; tiles of %d rows x %d columns, %.0f %% of their words inside the shape" %
                 ("one-word call, row-major", floor, tr, tc, 100 * fill))
    if row > 2 * copy:
        share = floor / row
        lines.append("    row-major is at %.0f %% of the copy's bandwidth, below half.  The call lasts %.1f us; a one-word call of the same kernel "
                     "lasts %.1f us, %.0f %% of it: the floor of a launch whose blocks each make one dependent global load - LDS - global store "
                     "round trip, which hipMemcpyAsync of these %.1f MB does not pay.  %.0f %% of the tile words are masked.  %s" %
                     (100 * copy / row, row * 1e3, floor * 1e3, 100 * share, nbytes / 1e6, 100 * (1 - fill),
                      "What limits it at this shape is that floor, not bytes." if share >= 0.5 else
                      "The floor does not account for most of it: the rest is not explained by this run."))
    else:
        lines.append("    row-major is at %.0f %% of the copy's bandwidth" % (100 * copy / row))
    ctx.synchronize()
    ctx.dev_free(out); ctx.dev_free(out2)
    L.glp_batch_free(h)


def lde_host_round_trip(ctx, lines, log_n, rb, reps):
    ncols = 16
    coeffs = glp.splitmix_field(3, ncols << log_n).reshape(ncols, 1 << log_n)
    ts = []
    for i in range(2 + reps):
        t0 = time.perf_counter(); ctx.lde(coeffs, rb); t = (time.perf_counter() - t0) * 1e3
        if i >= 2:
            ts.append(t)
    lines.append("lde_to_natural, the accessor's permutation that was there before: no entry point runs it on a batch.  It is reachable only inside "
                 "glp_lde, between a host-to-device and a device-to-host copy, so it cannot be timed on the batches above.  It is the permutation "
                 "the column-major rows above time (sub_bits = rate_bits: out[c][q R + r] = lde[c][r][q]): those rows are the substitute.  For "
                 "what the only existing path costs with its host round trip:")
    lines.append("    glp_lde (upload, LDE, k_lde_to_natural, download), %d columns, 2^%d rows, rate_bits %d, wall clock: %s for %.1f MB out" %
                 (ncols, log_n, rb, fmt(ts), (ncols << (log_n + rb)) * 8 / 1e6))


def coset_commit(ctx, tm, lines, name, K, num_polys, log_n, sub, rb, reps):
    L = glp.load_library()
    ncols, n = num_polys << sub, 1 << log_n
    words = K * ncols * n
    src = ctx.dev_alloc(words * 8)
    ctx.fill_random_device(src, words, 34)
    h = C.c_void_p()

    def from_coset():
        binding._chk(L.glp_batch_from_coset_values(ctx._h, C.c_void_p(src), 1, K, num_polys, log_n, sub, rb, 4, 0, None, C.byref(h)))
        L.glp_batch_free(h)

    def from_coeffs():
        if K == 1:
            binding._chk(L.glp_batch_from_coeffs_device(ctx._h, C.c_void_p(src), ncols, log_n, rb, 4, C.byref(h)))
        else:
            binding._chk(L.glp_batch_many_from_coeffs(ctx._h, C.c_void_p(src), 1, K, ncols, log_n, rb, 4, 0, None, C.byref(h)))
        L.glp_batch_free(h)
    lines.append("%s: K = %d, %d polynomials x 2^%d chunks = %d columns, 2^%d rows, rate_bits %d" % (name, K, num_polys, sub, ncols, log_n, rb))
    a, b = [], []
    for i in range(2 + reps):                                        # the two alternating
        ta, tb = tm.ms(from_coset), tm.ms(from_coeffs)
        if i >= 2:
            a.append(ta); b.append(tb)
    lines.append("    %-32s %s" % ("glp_batch_from_coset_values", fmt(a)))
    lines.append("    %-32s %s" % ("from_coeffs on the same columns", fmt(b)))
    lines.append("    %-32s %10.3f ms (medians)" % ("difference", float(np.median(a)) - float(np.median(b))))
    ctx.synchronize()
    ctx.dev_free(src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=20, help="rows of the wires shape (2^20: the headline circuit)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--commit", default="", help="the commit measured (recorded in the output)")
    a = ap.parse_args()
    ctx = glp.Context(a.device)
    tm = Timer(ctx.stream)
    lines = ["glp_batch_lde_values and glp_batch_from_coset_values on the clock (plonky2-lib_amd/tools/coset_seam_timing.py)%s; hipEvent pairs on "
             "the ctx stream around each call, 2 warm-up calls, median (min..max) of %d repetitions" %
             (", commit " + a.commit if a.commit else "", a.reps), "", "LDE reads, device to device, the whole coset"]
    lde_reads(ctx, tm, lines, "wires", 1, 136, a.log_n, 3, a.reps)
    lde_reads(ctx, tm, lines, "zkdsa x256", 256, 135, 3, 3, a.reps)
    lde_host_round_trip(ctx, lines, a.log_n, 3, min(a.reps, 3))
    lines += ["", "Coset commit, values in HBM"]
    coset_commit(ctx, tm, lines, "wires", 1, 17, a.log_n, 3, 3, a.reps)
    coset_commit(ctx, tm, lines, "zkdsa x256 (quotient oracle)", 256, 2, 3, 3, 3, a.reps)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
