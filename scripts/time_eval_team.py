"""Monte-Carlo evaluation of feed-forward agents and teams at the reference's size: the cost of ONE lock-step of
evaluate.run_test_environments_team with fused=True (rs_action_uniforms, rs_ff_eval_step, rs_step, rs_eval_post_step) against
fused=False (DeviceWelford, rs_ff_team_step's step round and torch bookkeeping), and for one agent also of today's
evaluate.run_test_environments (library ops throughout).

--envs saved environments x --runs Monte-Carlo runs = lanes (1000 x 100 = 100 000), --agents agents each, once obstacle-free and once
with --obstructions obstructions.  The policies are untrained, so no run of this length ends early.  A whole run also packs the set,
creates the environment and sorts 100 000 records on the host; to leave that out, the clock is read inside the run: every form draws
its uniforms (RadSearchVec.action_uniforms) exactly once, at the start of each lock-step, and the script wraps that method for the
time of the measurement -- at lock-step --skip it synchronises the device and starts the clock, at lock-step --skip + --steps it
synchronises and stops it.  Wall milliseconds per lock-step = that span / --steps, host issue time and the periodic host read
included.  --warmup untimed runs, then --repeats timed ones: min / median / max, one line per (configuration, form); then, per
configuration, the fused form's slowest against each baseline's fastest.  Plain text on stdout and in profiles/eval_team_timing.txt."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def per_step_ms(run, skip, steps, warmup, repeats):
    from radiation_ppo_amd.envs import RadSearchVec
    real = RadSearchVec.action_uniforms
    out = []
    for i in range(warmup + repeats):
        seen, stamps = [0], []

        def stamped(self, u):
            if seen[0] in (skip, skip + steps):
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
            seen[0] += 1
            return real(self, u)
        RadSearchVec.action_uniforms = stamped
        try:
            run(skip + steps + 1)
        finally:
            RadSearchVec.action_uniforms = real
        assert len(stamps) == 2 and seen[0] == skip + steps + 1, (seen, stamps)      # nothing ended early
        if i >= warmup:
            out.append((stamps[1] - stamps[0]) / steps * 1e3)
    return out


def mmm(v):
    return f"{min(v):8.4f} {statistics.median(v):8.4f} {max(v):8.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--skip", type=int, default=8)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_team_timing.txt"))
    args = ap.parse_args()
    from radiation_ppo_amd.evaluate import run_test_environments, run_test_environments_team, sample_test_environments
    from radiation_ppo_amd.ppo import VecAgentPPO
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# {args.envs} saved environments x {args.runs} runs = {args.envs * args.runs} lanes; wall ms per lock-step over lock-steps {args.skip}.."
        f"{args.skip + args.steps - 1} of a run; {args.warmup} warm-up + {args.repeats} timed repeats, seed {args.seed}; min median max")
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for obst in (0, args.obstructions):
        sets = sample_test_environments(args.envs, obstruction_count=obst, seed=args.seed)
        for A in args.agents:
            torch.manual_seed(args.seed)
            agents = {a: VecAgentPPO(id=a, steps_per_episode=args.skip + args.steps + 1, number_of_agents=A) for a in range(A)}
            common = dict(montecarlo_runs=args.runs, obstruction_count=obst, seed=args.seed)
            forms = {"fused": lambda L: run_test_environments_team(agents, sets, steps_per_episode=L, fused=True, **common),
                     "composed": lambda L: run_test_environments_team(agents, sets, steps_per_episode=L, fused=False, **common)}
            if A == 1:
                forms["run_test_environments"] = lambda L: run_test_environments(agents[0], sets, steps_per_episode=L, **common)
            res = {}
            for name, run in forms.items():
                res[name] = per_step_ms(run, args.skip, args.steps, args.warmup, args.repeats)
                say(f"agents {A} obstruction_count {obst} {name:21s} | ms per lock-step {mmm(res[name])} | "
                    f"{args.envs * args.runs / statistics.median(res[name]) / 1e3:8.2f} M lane steps/s (median)")
            for name in forms:
                if name != "fused":
                    f, b = res["fused"], res[name]
                    say(f"agents {A} obstruction_count {obst} fused slowest {max(f):.4f} ms, {name} fastest {min(b):.4f} ms -> "
                        f"{'faster' if max(f) < min(b) else 'NOT faster'}; median / median = {statistics.median(b) / statistics.median(f):.2f} x")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
