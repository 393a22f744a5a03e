"""bench.py without a GPU: the command line and the --dump-outputs writer (exact float64 halves of the proof words, a fixed
seeded sample of a batch that would not fit the size limit)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d, name):
    lo, hi = np.load(os.path.join(d, name + "_lo32.npy")), np.load(os.path.join(d, name + "_hi32.npy"))
    assert lo.dtype == hi.dtype == np.float64
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout and "--steps" in r.stdout


def test_dump_outputs_round_trip_is_exact(tmp_path):
    words = np.random.default_rng(3).integers(0, 2 ** 64 - 2 ** 32 + 1, 5000, dtype=np.uint64)
    words[:3] = (0, 2 ** 64 - 2 ** 32, 2 ** 32 - 1)                       # extremes of the Goldilocks field and of one half
    bench.dump_outputs(str(tmp_path), {"proof": words})
    assert sorted(os.listdir(str(tmp_path))) == ["proof_hi32.npy", "proof_lo32.npy"]
    assert (_load(str(tmp_path), "proof") == words).all()


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(tmp_path):
    proofs = np.random.default_rng(4).integers(0, 2 ** 63, (100, 1000), dtype=np.uint64)
    limit = 16 * proofs.size // 4                                          # room for a quarter of the batch
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), {"proofs": proofs}, limit=limit)
    rows = np.load(str(tmp_path / "a" / "proofs_rows.npy"))
    assert rows.dtype == np.float64 and len(rows) == 25 and (np.diff(rows) > 0).all()
    assert (rows == np.load(str(tmp_path / "b" / "proofs_rows.npy"))).all()
    got = _load(str(tmp_path / "a"), "proofs")
    assert (got == proofs[rows.astype(np.int64)]).all() and 16 * got.size <= limit
