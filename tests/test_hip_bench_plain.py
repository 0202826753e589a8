"""A plain `bench.py --gpus 1 --steps N --warmup W` run on the GPU: it prints the one result line and spends at most 30 s outside its steps --
the time of the whole run, from process start to exit, in a fresh home directory (nothing an earlier run cached), less (N + W) x ms_per_step, so
the first step's start-up (MIOpen find mode, code-object loads) counts."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTSIDE_STEPS_LIMIT_S = 30.0


def test_plain_run_is_lean(tmp_path):
    n, w = 3, 2
    env = dict(os.environ, HOME=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MIOPEN_USER_DB_PATH"):
        env.pop(k, None)
    t0 = time.perf_counter()
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(n), "--warmup", str(w)],
                        capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [ln for ln in pr.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines            # the result line alone: no full record in front of it
    rec = json.loads(lines[-1])
    assert rec["metric"].startswith("stereo-pairs/sec") and rec["unit"] == "stereo-pairs/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["steps"] == n and rec["warmup"] == w and rec["full"] is False and rec["config"]["workload"] == "4k-dav2b-dibr"
    assert abs(rec["value"] - 16 * 1e3 / rec["ms_per_step"]) < 0.01 * rec["value"]       # 16 frames per step
    assert not any(k.startswith(("roofline", "cpu_baseline", "sub_records")) for k in rec)
    outside = wall - (n + w) * rec["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.1f} s wall, {rec['ms_per_step']:.2f} ms per step, {outside:.1f} s outside its steps; {rec['wall_s']}")
    assert outside <= OUTSIDE_STEPS_LIMIT_S, (wall, rec["ms_per_step"], rec["wall_s"])
