#!/usr/bin/env python3
"""Time the RID-FIM evaluation lock-step (radiation_ppo_amd/bpf.py, csrc/rs_bpf.hip): ms per lock-step of the filter's track, of the
controller round and of the whole lock-step (rs_action_uniforms, track, controller, rs_step), fused (rs_bpf_track,
rs_ridfim_eval_step) against composed (rs_bpf_draws, rs_peek and float64 torch ops), at NP = 6000 particles.

    python scripts/time_eval_ridfim.py [--lanes 1000 16000] [--agents 1 2 4] [--obst 0 3] [--particles 6000] [--append]

writes profiles/eval_ridfim_timing.txt.  Per configuration: one warm-up lock-step, then REPEATS timed repeats of the fused form and
COMPOSED_REPEATS of the composed one (two: it takes seconds per lock-step, so its rows give min and max and no median), each repeat one lock-step between device synchronises (wall time); the verdict compares the
fused form's SLOWEST repeat with the composed form's FASTEST, as profiles/eval_gs_timing.txt does, and a row where the fused form loses
is marked SLOWER.  The lanes are fresh envs under the inverse-square falloff (the law the filter models), every filter one step past
its prior, thresh = 1 (a resampling at every step), the latch up (the Renyi round, the expensive one)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from radiation_ppo_amd.bpf import BootstrapParticleFilter  # noqa: E402
from radiation_ppo_amd.envs import RadSearchVec  # noqa: E402

REPEATS, COMPOSED_REPEATS = 5, 2


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(N, A, obst, NP, fused, repeats):
    vec = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=7, falloff="inverse_square")
    vec.reset()
    bpf = BootstrapParticleFilter(vec, nParticles=NP)
    track, act = (bpf.track, bpf.act) if fused else (bpf.track_composed, bpf.act_composed)
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    a8 = torch.zeros(N, A, dtype=torch.int8, device="cuda")
    u = torch.empty(N, A, device="cuda")
    track(vec.obs, alive, True)
    out = {"track": [], "round": [], "lock-step": []}
    for r in range(repeats + 1):
        bpf.rdiv.fill_(1)
        t_track = timed(lambda: track(vec.obs, alive, False))
        t_round = timed(lambda: act(vec.obs, alive, a8))
        bpf.rdiv.fill_(1)

        def lock_step():
            vec.action_uniforms(u)
            track(vec.obs, alive, False)
            act(vec.obs, alive, a8)
            vec.step(a8)
        t_step = timed(lock_step)
        if r:                                                      # the first pass is the warm-up
            out["track"].append(t_track); out["round"].append(t_round); out["lock-step"].append(t_step)
    del bpf, vec
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[1000, 16000])
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--obst", type=int, nargs="+", default=[0, 3])
    ap.add_argument("--particles", type=int, default=6000)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_ridfim_timing.txt"))
    args = ap.parse_args()
    with open(args.out, "a" if args.append else "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if not args.append:
            say(f"# lanes x agents filters of {args.particles} particles; wall ms per call between device synchronises; 1 warm-up, {REPEATS} fused and "
                f"{COMPOSED_REPEATS} composed repeats; min median max (composed: min - max)")
            say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
        for obst in args.obst:
            for N in args.lanes:
                for A in args.agents:
                    res = {form: measure(N, A, obst, args.particles, form == "fused", REPEATS if form == "fused" else COMPOSED_REPEATS)
                           for form in ("fused", "composed")}
                    for what in ("track", "round", "lock-step"):
                        head = f"lanes {N:6d} agents {A} obstruction_count {obst} {what:9s}"
                        for form in ("fused", "composed"):
                            v = sorted(res[form][what])
                            mid = f"{v[len(v) // 2]:12.3f}" if len(v) >= 3 else f"{'-':>12s}"       # no median of two repeats
                            say(f"{head} {form:9s} | ms {v[0]:12.3f} {mid} {v[-1]:12.3f}")
                        slow, fast = max(res["fused"][what]), min(res["composed"][what])
                        say(f"{head}: fused slowest {slow:.3f} ms, composed fastest {fast:.3f} ms -> {'faster' if slow < fast else 'SLOWER'}; "
                            f"{fast / slow:.2f} x")


if __name__ == "__main__":
    main()
