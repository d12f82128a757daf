"""bench.py's command line: a plain run measures the headline only (what takes
runs of its own is behind --full), and --dump-outputs writes what the last
timed step computed as float .npy files that agree with the result line."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def test_plain_run_dumps_outputs(device, tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "64",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["mc_stats"]["maps"] == 3          # --steps sets the timed steps
    assert res["ms_per_step"] == pytest.approx(64 / res["value"] * 1e3, rel=5e-3)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert key in res
    # a plain run: no CPU baseline, no contraction table over further maps
    assert res["cpu_baseline"] is None and res["roofline"]["contractions"] is None
    assert res["roofline"]["achieved"] > 0                            # the dominant layer's events are in the timed region
    files = {p.stem: np.load(p) for p in out.glob("*.npy")}
    names = list(res["mc_stats"]["mean_outputs"])
    assert len(names) >= 2                                            # accuracy and loss
    assert {f"output_{n}" for n in names} | {"blob_fc8", "per_map_outputs", "broken_cells"} <= set(files)
    assert sum(1 for k in files if k.startswith("faulted_weights_")) == len(files["broken_cells"])
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(np.isfinite(a).all() for a in files.values())
    assert files["blob_fc8"].shape == (64 * 1000,)
    pm = files["per_map_outputs"]
    assert pm.shape[0] == 3
    # the last row is the last timed map: the net still holds its outputs
    for k, name in enumerate(names):
        assert files[f"output_{name}"][0] == pytest.approx(pm[-1, k], rel=1e-6, abs=1e-9)
        assert pm[:, k].astype(np.float64).mean() == pytest.approx(res["mc_stats"]["mean_outputs"][name], rel=1e-6, abs=1e-9)
    assert files["broken_cells"].sum() == res["mc_stats"]["broken_cells"]
