"""Monte-Carlo evaluation of the recurrent agent (RAD-A2C) at the reference's size: the cost of ONE lock-step of
evaluate.run_test_environments_rnn -- the team runner (run_test_environments_rnn_team) with one agent -- with fused=True
(rs_action_uniforms, the PFGRU step, the policy round, rs_step, rs_rnn_team_eval_post_step and, with carried hidden states, rs_refresh
and rs_rnn_team_eval_post_refresh) against fused=False, the team runner's composed lock-step, which is also what
evaluate.run_test_environments runs for a recurrent agent (the same three big kernels inside ~20-35 torch ops).

--envs saved environments x --runs Monte-Carlo runs of --steps-per-episode steps, at the default widths, in both modes -- sequential
(carry_hidden_across_runs=True: one lane per environment, 1000 lanes, its runs one after the other) and lane-per-run (100 000 lanes)
-- once obstacle-free and once with --obstructions obstructions.  The policy is untrained, so hardly any run ends before the step
limit.  A whole run also packs the set, creates the environment and sorts the records on the host, and a sequential run at this size
is 12 000 lock-steps; to time the lock-step alone the clock is read inside the run: every form draws its uniforms
(RadSearchVec.action_uniforms) exactly once, at the start of each lock-step, and the script wraps that method for the time of the
measurement -- at lock-step --skip it synchronises the device and starts the clock, at lock-step --skip + window it synchronises,
stops it and ends the run there.  The window is --steps-seq lock-steps in sequential mode (by default it crosses the end of the first
run at lock-step 120, where every lane is refreshed) and --steps-lane in lane-per-run mode.  Wall milliseconds per lock-step = that
span / window, host issue time and the periodic host read included.  --warmup untimed runs, then --repeats timed ones: min / median /
max, one line per (configuration, form); then, per configuration, the fused form's slowest against the composed form's fastest.  Plain
text on stdout and in profiles/eval_rnn_timing.txt."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


class _WindowDone(Exception):
    """raised by the wrapped action_uniforms once the clock has stopped: the rest of the run is not needed"""


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
                if len(stamps) == 2:
                    raise _WindowDone
            seen[0] += 1
            return real(self, u)
        RadSearchVec.action_uniforms = stamped
        try:
            run()
        except _WindowDone:
            pass
        finally:
            RadSearchVec.action_uniforms = real
        assert len(stamps) == 2 and seen[0] == skip + steps, (seen, stamps)           # the run did not end before the window did
        if i >= warmup:
            out.append((stamps[1] - stamps[0]) / steps * 1e3)
    return out


def mmm(v):
    return f"{min(v):8.4f} {statistics.median(v):8.4f} {max(v):8.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--steps-per-episode", type=int, default=120)
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--skip", type=int, default=8)
    ap.add_argument("--steps-seq", type=int, default=128)
    ap.add_argument("--steps-lane", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rnn_timing.txt"))
    args = ap.parse_args()
    from radiation_ppo_amd.evaluate import run_test_environments_rnn, sample_test_environments
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    L = args.steps_per_episode
    assert args.skip + args.steps_lane < L and args.skip + args.steps_seq < L * args.runs
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# {args.envs} saved environments x {args.runs} runs of {L} steps; wall ms per lock-step over lock-steps {args.skip}.."
        f"{args.skip + args.steps_seq - 1} (sequential) / {args.skip}..{args.skip + args.steps_lane - 1} (lane-per-run) of a run; "
        f"{args.warmup} warm-up + {args.repeats} timed repeats, seed {args.seed}; min median max")
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    torch.manual_seed(args.seed)
    agent = RNNAgentPPO(id=0, steps_per_episode=L)
    for obst in (0, args.obstructions):
        sets = sample_test_environments(args.envs, obstruction_count=obst, seed=args.seed)
        for mode, carry, lanes, window in (("sequential", True, args.envs, args.steps_seq),
                                           ("lane-per-run", False, args.envs * args.runs, args.steps_lane)):
            res = {}
            for name, fused in (("fused", True), ("composed", False)):
                run = lambda: run_test_environments_rnn(agent, sets, montecarlo_runs=args.runs, steps_per_episode=L, obstruction_count=obst,
                                                        seed=args.seed, carry_hidden_across_runs=carry, fused=fused)
                res[name] = per_step_ms(run, args.skip, window, args.warmup, args.repeats)
                say(f"{mode:12s} lanes {lanes:6d} obstruction_count {obst} {name:8s} | ms per lock-step {mmm(res[name])} | "
                    f"{lanes / statistics.median(res[name]) / 1e3:8.2f} M lane steps/s (median)")
            f, b = res["fused"], res["composed"]
            say(f"{mode:12s} lanes {lanes:6d} obstruction_count {obst} fused slowest {max(f):.4f} ms, composed fastest {min(b):.4f} ms -> "
                f"{'faster' if max(f) < min(b) else 'NOT faster'}; median / median = {statistics.median(b) / statistics.median(f):.2f} x")
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
