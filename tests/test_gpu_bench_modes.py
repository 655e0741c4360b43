"""bench.py's two modes on a small scene.  A plain run prints the headline line and nothing that needs a run of its own (no
stage table, roofline, CPU baseline or side measurement) and still writes --dump-outputs; --full adds the per-view counts, the
stage table and the rooflines."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "windows_ms_per_step", "config")
FULL_ONLY = ("stages", "roofline", "roofline_valu", "kernel_ms_per_step", "cpu_baseline", "forward_only", "train_loop", "ms_per_step_without_kernel_events")


def _bench(args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BH_FORCE_PG"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--splats", "50000"] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone(tmp_path):
    out_dir = tmp_path / "outputs"
    d = _bench(["--dump-outputs", str(out_dir)])
    for k in HEADLINE:
        assert k in d, k
    assert d["unit"] == "views/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-2
    assert len(d["windows_ms_per_step"]) == 3 and d["config"]["timed_steps"] == 9
    assert not [k for k in FULL_ONLY if k in d]
    assert "per_view" not in d["config"]
    for name in ("transforms", "sh_coeffs", "raw_opacities", "loss", "num_visible", "num_intersections"):
        assert (out_dir / (name + ".npy")).is_file(), name


def test_full_run_adds_the_stage_table_and_rooflines():
    d = _bench(["--full", "--no-pmc", "--no-cpu-baseline"])
    for k in HEADLINE + ("stages", "roofline", "roofline_valu", "forward_only", "ms_per_step_without_kernel_events"):
        assert k in d, k
    assert d["stages"] and d["stages"]["RasterizeBackwards"]["ms"] > 0
    assert d["roofline"]["intersections_blended"] > 0
    assert len(d["config"]["per_view"]) == 2 and d["config"]["num_visible"] > 0
