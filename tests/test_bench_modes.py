"""bench.py's two modes: a plain run reports the headline and what its timed steps measured on their own; --full adds what takes
runs of its own after them (the gradient pass and the env-step kernel re-timed, the 2^20-env step, the CPU baseline, the extra
configs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline_env_step", "roofline_env_step_large_n", "cpu_baseline", "configs")


def _line(cmd):
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_extra_configs_need_full():
    """--configs names work that only --full does: without it the command is refused before anything runs."""
    out = subprocess.run([sys.executable, BENCH, "--steps", "1", "--configs", "3"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--full" in out.stderr, out.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_and_full_run():
    base = [sys.executable, BENCH, "--gpus", "1", "--steps", "1", "--warmup", "0", "--envs-per-gpu", "1024"]
    plain = _line(base)
    assert plain["steps"] == 1 and plain["warmup"] == 0 and plain["ms_per_step"] > 0 and plain["higher_is_better"] is True
    assert abs(plain["value"] * plain["ms_per_step"] * 1e-3 - 480 * 1024) < 1.0
    assert not set(FULL_ONLY) & set(plain), sorted(plain)
    assert plain["roofline"]["launches_timed"] == sum(plain["update_adam_steps"])     # from the timed steps' own HIP events
    assert "avg_launch_ms_isolated" not in plain["roofline"]

    full = _line(base + ["--full", "--cpu-seconds", "1"])
    assert abs(full["value"] * full["ms_per_step"] * 1e-3 - 480 * 1024) < 1.0
    assert full["roofline"]["avg_launch_ms_isolated"] > 0
    assert full["roofline_env_step"]["avg_launch_ms"] > 0
    assert full["roofline_env_step_large_n"]["envs"] == 1 << 20, full["roofline_env_step_large_n"]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["kind"] == "port"
    assert "configs" not in full                    # below 4096 envs per GPU the extra configs default to none
