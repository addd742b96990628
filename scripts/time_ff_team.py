"""Feed-forward teams at the workload's size: ppo.Collector (library ops, the baseline) against ppo.TeamCollector (rs_ff_team_step
between the rs_collect_* glue), and the K7 update behind either.

--envs envs x each of --agents agents, --steps-per-epoch / --steps-per-episode steps, once obstacle-free and once with
obstruction_count = -1 (a random count per episode).  Both collectors get the same env seed and the same initial parameters; each runs
--warmup epochs (collect + update) untimed, then --epochs timed ones, the device synchronised around every timed region:
  collect   wall seconds of collect(), and `issue`: the part of it the host spent issuing launches (collect() returns before the device
            has finished; where issue ~ collect the lock-step is bound by the host's launch rate, not by the kernels)
  update    wall seconds of update() (the same K7 path for both: A x 40 Adam steps)
min / median / max over the timed epochs, one line per (configuration, collector); then, per configuration, TeamCollector's slowest
collect against Collector's fastest.  Plain text on stdout (profiles/ff_team_timing.txt keeps a copy)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def run(cls, N, A, T, L, obst, warmup, epochs, seed):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.ppo import VecAgentPPO
    torch.manual_seed(seed)
    env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=seed)
    agents = {a: VecAgentPPO(id=a, steps_per_epoch=T, steps_per_episode=L, number_of_agents=A, alpha=0.1) for a in range(A)}
    col = cls(env, agents, T, L)
    sync = lambda: torch.cuda.synchronize(env.device)
    for _ in range(warmup):
        col.collect(); col.update()
    collect, issue, update = [], [], []
    for _ in range(epochs):
        sync()
        t0 = time.perf_counter()
        col.collect()
        t1 = time.perf_counter()
        sync()
        t2 = time.perf_counter()
        col.update()
        sync()
        t3 = time.perf_counter()
        collect.append(t2 - t0); issue.append(t1 - t0); update.append(t3 - t2)
    assert env.error_flags() == 0
    return collect, issue, update


def mmm(v):
    return f"{min(v):8.4f} {statistics.median(v):8.4f} {max(v):8.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--steps-per-epoch", type=int, default=480)
    ap.add_argument("--steps-per-episode", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    from radiation_ppo_amd.ppo import Collector, TeamCollector
    N, T, L = args.envs, args.steps_per_epoch, args.steps_per_episode
    print(f"# {N} envs, T = {T}, L = {L}, {args.warmup} warm-up + {args.epochs} timed epochs, seed {args.seed}; seconds: min median max")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for A in args.agents:
        for obst in (0, -1):
            res = {}
            for cls in (Collector, TeamCollector):
                c, i, u = res[cls.__name__] = run(cls, N, A, T, L, obst, args.warmup, max(3, args.epochs), args.seed)
                rate = N * T / (statistics.median(c) + statistics.median(u))
                print(f"agents {A} obstruction_count {obst:2d} {cls.__name__:13s} | collect {mmm(c)} | issue {mmm(i)} | update {mmm(u)} | "
                      f"{rate / 1e6:6.3f} M env steps/s (median collect + median update)", flush=True)
            base, team = res["Collector"][0], res["TeamCollector"][0]
            print(f"agents {A} obstruction_count {obst:2d} collect: TeamCollector slowest {max(team):.4f} s, Collector fastest {min(base):.4f} s "
                  f"-> {'faster' if max(team) < min(base) else 'NOT faster'}; median / median = {statistics.median(base) / statistics.median(team):.2f} x",
                  flush=True)


if __name__ == "__main__":
    main()
