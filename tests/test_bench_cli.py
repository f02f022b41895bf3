"""bench.py command line: the lossless float64 dump of u64 outputs, and one
tiny plain run with --dump-outputs on the GPU."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def _halves_to_u64(a):
    assert a.dtype == np.float64
    assert np.array_equal(a, np.floor(a)) and a.min() >= 0 and a.max() < 2.0 ** 32
    return np.ascontiguousarray(a.astype(np.uint32)).view(np.uint64)


def test_dump_u64_is_lossless(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 64, size=(5, 157), dtype=np.uint64)
    a[0, 0] = 0
    a[0, 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    bench.dump_u64(tmp_path / "d", "proofs", a)
    back = np.load(tmp_path / "d" / "proofs.npy")
    assert back.shape == (5, 314)
    assert np.array_equal(_halves_to_u64(back), a)


def test_options_present():
    out = subprocess.run([sys.executable, str(REPO / "bench.py"), "--help"],
                         capture_output=True, text=True, check=True).stdout
    assert "--full" in out and "--dump-outputs" in out


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    from renegade_amd import load_prover
    if not load_prover().gpu_available:
        pytest.skip("no GPU")
    jobs, steps = 3, 2
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1",
                        "--steps", str(steps), "--warmup", "1", "--jobs", str(jobs),
                        "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["unit"] == "proofs/s"
    assert res["ms_per_step"] > 0 and res["value"] > 0
    # a plain run carries none of the --full legs
    assert res["roofline"] is None and res["cpu_baseline"] is None
    assert [p.name for p in tmp_path.iterdir()] == ["proofs.npy"]
    proofs = _halves_to_u64(np.load(tmp_path / "proofs.npy"))
    assert proofs.shape == (jobs, 157)
    # distinct seeds -> distinct, non-trivial proofs
    assert all(np.any(proofs[i] != 0) for i in range(jobs))
    assert not np.array_equal(proofs[0], proofs[1])
