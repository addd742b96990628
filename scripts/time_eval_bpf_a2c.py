#!/usr/bin/env python3
"""Time the BPF-A2C evaluation lock-step (radiation_ppo_amd/evaluate.py: _bpf_a2c_rounds; csrc/rs_bpf.hip, csrc/rs_rnn_policy.hip): ms
per call of rs_bpf_fim against fim_composed, of rs_bpf_a2c_eval_step against its composition (the standardisation, clip and scaling
in torch, rs_rnn_team_eval_step, the idle rule and the table in torch), and of the whole lock-step with the Fisher analysis on
(rs_action_uniforms, track, the matrix at the detector, the policy step, the matrix at the predicted position, rs_step), fused against
composed, at NP = 6000 particles.

    python scripts/time_eval_bpf_a2c.py [--lanes 1000 16000] [--agents 1 2 4] [--obst 0 3] [--particles 6000] [--append]

writes profiles/eval_bpf_a2c_timing.txt.  The method is scripts/time_eval_ridfim.py's: per configuration one warm-up pass, then REPEATS
timed repeats of the fused form and COMPOSED_REPEATS of the composed one (two: its track takes a second per lock-step, so its rows give
min and max and no median), each repeat one call between device synchronises (wall time); the verdict compares the fused form's SLOWEST
repeat with the composed form's FASTEST, and a row where the fused form loses is marked SLOWER.  The lanes are fresh envs under the
inverse-square falloff (the law the filter models), every filter one step past its prior, thresh = 1 (a resampling at every step),
untrained default-width actors (the arithmetic does not depend on the weights' values)."""
import argparse
import ctypes as C
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from radiation_ppo_amd import _lib, evaluate  # noqa: E402
from radiation_ppo_amd.envs import RadSearchVec  # noqa: E402
from radiation_ppo_amd.ppo import DeviceWelford  # noqa: E402
from radiation_ppo_amd.rada2c import RNNAgentPPO  # noqa: E402

REPEATS, COMPOSED_REPEATS = 5, 2


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(agents, N, A, obst, NP, fused, repeats):
    dev = torch.device("cuda:0")
    vec = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=7, falloff="inverse_square")
    vec.reset()
    obs = vec.obs.clone()
    stat = DeviceWelford((N, A), dev)
    stat.update(obs[..., 0])
    alive = torch.ones(N, dtype=torch.bool, device=dev)
    run = SimpleNamespace(lib=_lib.load(), vec=vec, obs=obs, stat=stat, N=N, A=A, L=4, seed=7, dev=dev,
                          st=C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), u=torch.empty(N, A, device=dev), alive=alive,
                          alive8=alive.view(torch.uint8))
    rec = dict(fisher=True)
    before, policy_round = evaluate._bpf_a2c_rounds(run, fused, {a: agents[a] for a in range(A)}, dict(nParticles=NP), rec, 0)
    bpf = run.bpf
    fim = bpf.fim if fused else bpf.fim_composed
    a8 = torch.zeros(N, A, dtype=torch.int8, device=dev)
    F = torch.zeros(N, A, 3, 3, dtype=torch.float64, device=dev)
    before()                                                       # the prior; every later call is the process model
    policy_round(a8)
    p = lambda t: t.data_ptr()
    wts = [agents[a].policy_weights() for a in range(A)]
    wp = (C.c_void_p * A)(*[p(w) for w in wts])
    x, loc, k8 = torch.empty_like(obs), torch.empty(N, A, 2, device=dev), torch.full((N, A), 8, dtype=torch.int8, device=dev)
    table = torch.tensor(evaluate.BPF_A2C_ACTION, dtype=torch.float64, device=dev)

    def step_alone():                                              # the policy step without its Fisher matrix
        if fused:
            _lib.check(run.lib.rs_bpf_a2c_eval_step(vec._h, wp, A, p(obs), p(stat.mean), p(stat.std), p(bpf.estimate), 2200.0, p(run.hid), p(run.u),
                                                    p(run.alive8), p(a8), p(run.sim_pos), None, None, run.st), "rs_bpf_a2c_eval_step")
        else:
            x.copy_(obs)
            x[..., 0] = ((obs[..., 0].double() - stat.mean) / stat.std).float().clamp(-8.0, 8.0)
            loc.copy_((bpf.estimate[..., 1:] / 2200.0).float())
            _lib.check(run.lib.rs_rnn_team_eval_step(wp, A, p(x), p(loc), p(run.hid), p(run.u), p(run.alive8), p(k8), N, run.st),
                       "rs_rnn_team_eval_step")
            a8.copy_(torch.where(alive.view(N, 1), k8, torch.full_like(k8, 8)))
            pos = torch.stack([vec.state("x").t(), vec.state("y").t()], dim=-1).double()
            run.sim_pos.copy_(torch.where(alive.view(N, 1, 1), pos + table[a8.long().clamp(0, 7)], run.sim_pos))

    def lock_step():
        rec["it"] = 1                                              # row 1 of the matrix buffer every time
        vec.action_uniforms(run.u)
        before()
        policy_round(a8)
        vec.step(a8)
    out = {"fim": [], "step": [], "lock-step": []}
    for r in range(repeats + 1):
        vec.action_uniforms(run.u)
        t_fim = timed(lambda: fim(run.alive8, pos=run.sim_pos, F=F))
        t_pol = timed(step_alone)
        t_step = timed(lock_step)
        if r:                                                      # the first pass is the warm-up
            out["fim"].append(t_fim); out["step"].append(t_pol); out["lock-step"].append(t_step)
    del bpf, vec, run
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[1000, 16000])
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--obst", type=int, nargs="+", default=[0, 3])
    ap.add_argument("--particles", type=int, default=6000)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bpf_a2c_timing.txt"))
    args = ap.parse_args()
    agents = {}
    for a in range(max(args.agents)):
        torch.manual_seed(a)
        agents[a] = RNNAgentPPO(id=a)
    with open(args.out, "a" if args.append else "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if not args.append:
            say(f"# lanes x agents filters of {args.particles} particles; wall ms per call between device synchronises; 1 warm-up, {REPEATS} fused and "
                f"{COMPOSED_REPEATS} composed repeats; min median max (composed: min - max)")
            say("# fim: rs_bpf_fim | fim_composed at a given position; step: rs_bpf_a2c_eval_step | its composition; lock-step: uniforms, track, "
                "matrix, step, matrix, rs_step")
            say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
        for obst in args.obst:
            for N in args.lanes:
                for A in args.agents:
                    res = {form: measure(agents, N, A, obst, args.particles, form == "fused", REPEATS if form == "fused" else COMPOSED_REPEATS)
                           for form in ("fused", "composed")}
                    for what in ("fim", "step", "lock-step"):
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
