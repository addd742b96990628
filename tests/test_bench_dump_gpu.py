"""bench.py --dump-outputs: after the timed steps the headline path's last PPO iteration is written as .npy files (float32 /
float64, a bounded sample of the rollout buffer), and --steps sets the number of timed steps the result line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_of_the_last_timed_step(tmp_path):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0", "--envs-per-gpu", "1024",
           "--configs", "none", "--no-cpu-baseline", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and len(d["update_adam_steps"]) == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 480 * 1024) < 1.0
    files = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert all(f.endswith(".npy") for f in os.listdir(out_dir))
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(out_dir / f) for f in os.listdir(out_dir)) <= 64 << 20
    # 512 of the 1024 env columns, the whole epoch
    assert files["buf_obs"].shape == (480, 512, 1, 11) and files["buf_act"].shape == (480, 512, 1)
    for k in ("logp", "val", "rew", "last_val", "cut", "adv", "ret"):
        assert files["buf_" + k].shape == (480, 512, 1) and np.all(np.isfinite(files["buf_" + k])), k
    assert set(np.unique(files["buf_act"])) <= set(range(8))
    assert int(files["update_stop_iteration"]) == d["update_adam_steps"][-1]
    assert any(k.startswith("param_actor") for k in files) and any(k.startswith("param_critic") for k in files)
    assert all(np.all(np.isfinite(a)) for k, a in files.items() if k.startswith("param_"))
