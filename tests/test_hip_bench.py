"""GPU: bench.py's own contract -- `--steps` sets the timed steps, `ms_per_step` is their time, and `--dump-outputs` writes
what the last timed step returned, from inputs that are the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu


def _bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NSR_FORCE_SHARDED")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "2", "--windows", "1",
                        "--no-cpu-baseline", "--no-strong-record", "--no-consumed-record", "--dump-outputs", str(out_dir), *extra],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("launch", ["window graph", "eager"])
def test_bench_dump_outputs_repeat_with_the_same_arguments(tmp_path, launch):
    extra = ("--eager",) if launch == "eager" else ()
    runs = []
    for name in ("a", "b"):
        d = _bench(tmp_path / name, *extra)
        assert d["steps"] == 7 and sum(d["config"]["stage_mix"].values()) == 7, d["config"]["stage_mix"]
        assert len(d["config"]["timed_windows_ms"]) == 1
        assert abs(d["ms_per_step"] * 7 - d["config"]["timed_windows_ms"][0]) < 1e-3 * d["config"]["timed_windows_ms"][0] + 1e-3
        rec = d["dump_outputs"]
        files = sorted(os.listdir(tmp_path / name))
        assert rec["arrays"] == len(files) and rec["bytes"] == sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64_000_000
        runs.append((d, {f[:-4]: np.load(tmp_path / name / f) for f in files}))
    (da, a), (db, b) = runs
    assert da["dump_outputs"]["last_step_stage"] == db["dump_outputs"]["last_step_stage"]
    assert sorted(a) == sorted(b)
    assert "loss" in a and any(k.startswith("grid_") for k in a) and any("_decoder." in k for k in a), sorted(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.isfinite(v).all() for v in a.values())
    assert float(np.abs(a["loss"]).max()) > 0
    # the inputs are the same; only the order of the gradients' atomic sums may differ between the two runs
    for k in a:
        assert rel_err(b[k], a[k]) < 1e-3, (k, rel_err(b[k], a[k]))
