"""bench.py command line: a plain run does only the headline measurement,
--full adds the secondary ones, --dump-outputs writes the last timed
step's result reproducibly."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra: str) -> dict:
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--device", "cpu",
           "--triples", "60000", "--steps", "3", "--warmup", "1", *extra]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-1000:]
    return json.loads(lines[0])


def test_plain_run_dumps_reproducible_outputs(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    b = _bench("--dump-outputs", str(tmp_path / "b"))
    assert a["steps"] == 3 and a["ms_per_step"] > 0
    assert abs(a["value"] - 1000.0 / a["ms_per_step"]) < 1e-6 * a["value"]
    cfg = a["config"]
    for k in ("cold_ms_p50", "rows_variant_ms_per_step",
              "shuffle_ms_per_step", "bcast_ms_per_step"):
        assert cfg[k] is None, k
    assert sorted(os.listdir(tmp_path / "a")) == ["result_count.npy"]
    xa = np.load(tmp_path / "a" / "result_count.npy")
    xb = np.load(tmp_path / "b" / "result_count.npy")
    assert xa.dtype == np.float64 and xa.shape == (1,)
    assert xa[0] == cfg["result_count"] > 0
    assert np.array_equal(xa, xb)


def test_full_run_reports_secondary_measurements():
    r = _bench("--full")
    cfg = r["config"]
    assert cfg["cold_ms_p50"] > 0
    assert cfg["rows_variant_ms_per_step"] > 0
    assert cfg["rows_variant_result_rows"] is not None
    assert cfg["result_count"] > 0
