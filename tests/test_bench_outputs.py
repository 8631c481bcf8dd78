"""bench.py's plain run and --dump-outputs.

CPU: dump_outputs writes the verdicts of a bitmap as float32 in record order, and beyond DUMP_MAX_RECORDS the same
seeded sample in every call; --steps 0 is refused (ms_per_step would be undefined).
GPU: one small plain run (no --full) prints the contract fields, leaves every extra leg out, and dumps the verdicts
its last timed step computed (the seeded generator's records are all valid, so the dump is all ones in every run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _words(bits):
    return np.packbits(bits.astype(np.uint8), bitorder="little").view(np.uint32)


def test_dump_outputs_record_order(tmp_path):
    import at2v
    import bench
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, 4096).astype(bool)
    bench.dump_outputs(str(tmp_path / "d"), at2v, np, _words(bits), 4000)
    got = np.load(tmp_path / "d" / "verdicts.npy")
    assert got.dtype == np.float32 and got.shape == (4000,)
    assert np.array_equal(got, bits[:4000].astype(np.float32))


def test_dump_outputs_large_is_a_fixed_sample(tmp_path):
    import at2v
    import bench
    total = 2 * bench.DUMP_MAX_RECORDS
    bits = np.random.default_rng(8).integers(0, 2, total).astype(bool)
    w = _words(bits)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), at2v, np, w, total)
    a, b = np.load(tmp_path / "a" / "verdicts.npy"), np.load(tmp_path / "b" / "verdicts.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_RECORDS,) and a.nbytes <= 64 << 20
    assert np.array_equal(a, b)
    idx = np.sort(np.random.default_rng(bench.CFG_SEED).choice(total, bench.DUMP_MAX_RECORDS, replace=False))
    assert np.array_equal(a, bits[idx].astype(np.float32))


def test_zero_steps_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 2 and "--steps" in out.stderr and not out.stdout.strip()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_last_step(tmp_path):
    n = 4096 + 64  # more than one block, not a power of two
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--records-per-gpu", str(n), "--dump-outputs", str(tmp_path / "d")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["verdict_match"] == 1.0
    assert r["unit"] == "verifies/s" and r["higher_is_better"] is True and r["dtype"] == "int32"
    assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(n / (r["ms_per_step"] * 1e-3))
    for leg in ("e2e", "e2e_abi", "at2_traffic", "sender_churn", "cpu_baseline", "multi_gpu"):
        assert leg not in r, leg
    assert r["launch_ms_alone"] is None and r["roofline"]["traffic"] is None
    assert "CPU baseline" not in out.stderr and "PMC" not in out.stderr
    got = np.load(tmp_path / "d" / "verdicts.npy")
    assert got.dtype == np.float32 and got.shape == (n,)
    assert bool((got == 1.0).all())  # the generator's records are all valid, in every run
