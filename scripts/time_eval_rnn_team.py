"""Monte-Carlo evaluation of RAD-A2C teams (evaluate.run_test_environments_rnn_team) at the reference's size.  Two measurements, plain
text on stdout and in profiles/eval_rnn_team_timing.txt.

1. The policy round alone: one rs_rnn_team_eval_step launch for the whole team against A back-to-back rs_rnn_policy_step_rows launches
   (K14 on agent a's rows: what the lock-step would do without the team kernel), at N = --kernel-lanes lanes and A = 2, 4, 8 agents,
   all lanes active.  --kernel-rounds policy rounds are issued back to back on one stream between two device synchronisations and the
   wall span is divided by the rounds, host issue time included -- at 1000 lanes the round is launch-bound and that is the cost the
   lock-step pays.  --warmup untimed repeats, then --repeats timed ones: min / median / max; condition at the smallest size: the team
   launch's slowest repeat below the per-agent form's fastest.

2. The lock-step of the whole runner, fused against composed, by scripts/time_eval_rnn.py's method (the clock is read inside the run,
   in the wrapped RadSearchVec.action_uniforms, over a window of lock-steps behind --skip): --envs saved environments x --runs runs of
   --steps-per-episode steps, A = 2 and 4 untrained default-width agents, both hidden-state lifetimes, obstacle-free and with
   --obstructions obstructions.  Per configuration the fused form's slowest repeat against the composed form's fastest; and, with
   carried hidden states, the A-agent fused median against A times the one-agent fused median (run_test_environments_rnn, the same runner with
   one agent, timed here the same way): evaluating the agents one by one is what was possible before.

sized_rows() (--sized HID POL VAL REC; scripts/time_rnn_team_collect.py calls it): both measurements at a sized width, where the fused
runner's policy round is rs_rnn_sized_team_step -- against the fused form it had before, one rs_rnn_sized_step launch per agent."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from time_eval_rnn import mmm, per_step_ms


def kernel_ab(N, A, rounds, warmup, repeats, widths=None):
    """{form: [wall ms per policy round]} for the team launch and for A launches of K14; widths = (hid, pol, val): the same for
    rs_rnn_sized_team_step (the evaluation's use: no value, no log-probability) and A launches of rs_rnn_sized_step"""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N + A)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)
    hid = widths[0] if widths else 24
    W = [(rnd(lib.rs_rnn_sized_weight_floats(*widths) if widths else 5296) - 0.5) * 0.5 for _ in range(A)]
    x, loc, u, h = rnd(N, A, 11), rnd(N, A, 2), rnd(N, A), rnd(A, N, hid) - 0.5
    active = torch.ones(N, dtype=torch.uint8, device=dev)
    act8 = torch.zeros(N, A, dtype=torch.int8, device=dev)
    scratch = torch.empty(N, dtype=torch.int64, device=dev)
    p = lambda t: t.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    wp = (C.c_void_p * A)(*[p(w) for w in W])

    def team():
        if widths:
            _lib.check(lib.rs_rnn_sized_team_step(wp, A, *widths, p(x), p(loc), p(h), p(u), None, None, p(act8), p(active), N, st),
                       "rs_rnn_sized_team_step")
            return
        _lib.check(lib.rs_rnn_team_eval_step(wp, A, p(x), p(loc), p(h), p(u), p(active), p(act8), N, st), "rs_rnn_team_eval_step")

    def per_agent():
        for a in range(A):
            ha = p(h) + 4 * a * N * hid
            if widths:
                _lib.check(lib.rs_rnn_sized_step(p(W[a]), *widths, p(x) + 44 * a, 11 * A, p(loc) + 8 * a, 2 * A, ha, p(u) + 4 * a, A, ha, None,
                                                 None, p(scratch), None, p(act8) + a, A, p(active), N, st), "rs_rnn_sized_step")
                continue
            _lib.check(lib.rs_rnn_policy_step_rows(p(W[a]), p(x) + 44 * a, 11 * A, p(loc) + 8 * a, 2 * A, ha, p(u) + 4 * a, A, ha, None, p(scratch),
                                                   None, p(act8) + a, A, p(active), N, st), "rs_rnn_policy_step_rows")
    out = {}
    for name, fn in (("team", team), ("per-agent", per_agent)):
        v = []
        for i in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(rounds):
                fn()
            torch.cuda.synchronize()
            if i >= warmup:
                v.append((time.perf_counter() - t0) / rounds * 1e3)
        out[name] = v
    return out


class per_agent_sized_round:
    """Inside this context the fused runner's sized-width policy round is what it was before rs_rnn_sized_team_step: one
    rs_rnn_sized_step launch per agent on its rows (mask = active, h in place, the action to act8 and to an int64 scratch).  The
    library object's entry is shadowed by a Python function of the same signature; the runner itself is not touched."""

    def __enter__(self):
        from radiation_ppo_amd import _lib
        lib = self.lib = _lib.load()
        self.real = lib.rs_rnn_sized_team_step
        step = lib.rs_rnn_sized_step
        scratch = {}

        def per_agent(wp, A, hid, pol, val, x, loc, h, u, act, f, act8, mask, N, st):
            assert act is None and f is None
            if N not in scratch:
                scratch[N] = torch.empty(N, dtype=torch.int64, device="cuda:0")
            s = scratch[N].data_ptr()
            for a in range(A):
                ha = h + 4 * a * N * hid
                rc = step(wp[a], hid, pol, val, x + 44 * a, 11 * A, loc + 8 * a, 2 * A, ha, u + 4 * a, A, ha, None, None, s, None, act8 + a, A,
                          mask, N, st)
                if rc:
                    return rc
            return 0
        lib.rs_rnn_sized_team_step = per_agent
        return self

    def __exit__(self, *exc):
        self.lib.rs_rnn_sized_team_step = self.real
        return False


def sized_rows(say, widths, rec, agents, envs, runs, L, obstructions, skip, steps_seq, warmup, repeats, seed, kernel_lanes, kernel_agents,
               kernel_rounds):
    """The two measurements of this script at a sized width, the fused form before (one rs_rnn_sized_step per agent) and after
    (rs_rnn_sized_team_step): the policy round alone, and the sequential runner's lock-step for A in `agents` (1 included: whether one
    agent's lock-step pays for the team kernel's grid).  The two forms' repeats alternate."""
    from radiation_ppo_amd.evaluate import run_test_environments_rnn_team, sample_test_environments
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    say(f"# sized widths GRU {widths[0]} / heads {widths[1]} / {widths[2]} / PFGRU {rec}: the policy round, wall ms per round over "
        f"{kernel_rounds} rounds issued back to back, all lanes active")
    for N in kernel_lanes:
        for A in kernel_agents:
            r = kernel_ab(N, A, kernel_rounds, warmup, repeats, widths)
            for name in ("team", "per-agent"):
                say(f"sized policy round lanes {N:6d} agents {A} {name:9s} | ms per round {mmm(r[name])}")
            t, b = r["team"], r["per-agent"]
            say(f"sized policy round lanes {N:6d} agents {A} team slowest {max(t):.4f} ms, per-agent fastest {min(b):.4f} ms -> "
                f"{'faster' if max(t) < min(b) else 'NOT faster'}; median / median = {statistics.median(b) / statistics.median(t):.2f} x")
    say(f"# sized widths, the fused runner: {envs} saved environments x {runs} runs of {L} steps, carried hidden states; wall ms per "
        f"lock-step over lock-steps {skip}..{skip + steps_seq - 1}")
    args = dict(hidden=((widths[0],),), hidden_sizes_pol=((widths[1],),), hidden_sizes_val=((widths[2],),), hidden_sizes_rec=(rec,))
    team = {}
    for a in range(max(agents)):
        torch.manual_seed(seed + a)
        team[a] = RNNAgentPPO(id=a, steps_per_episode=L, actor_critic_args=args)
    for obst in (0, obstructions):
        sets = sample_test_environments(envs, obstruction_count=obst, seed=seed)
        for A in agents:
            run = lambda: run_test_environments_rnn_team({a: team[a] for a in range(A)}, sets, montecarlo_runs=runs, steps_per_episode=L,
                                                         obstruction_count=obst, seed=seed, carry_hidden_across_runs=True, fused=True)
            res = {"team launch": [], "per-agent launches": []}
            for i in range(warmup + repeats):
                for name in res:
                    if name == "team launch":
                        v = per_step_ms(run, skip, steps_seq, 0, 1)
                    else:
                        with per_agent_sized_round():
                            v = per_step_ms(run, skip, steps_seq, 0, 1)
                    if i >= warmup:
                        res[name] += v
            for name, v in res.items():
                say(f"sized sequential lanes {envs:6d} agents {A} obstruction_count {obst} fused, {name:18s} | ms per lock-step {mmm(v)}")
            t, b = res["team launch"], res["per-agent launches"]
            say(f"sized sequential lanes {envs:6d} agents {A} obstruction_count {obst} team launch slowest {max(t):.4f} ms, per-agent launches "
                f"fastest {min(b):.4f} ms -> {'faster' if max(t) < min(b) else 'NOT faster'}; median / median = "
                f"{statistics.median(b) / statistics.median(t):.2f} x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=100)
    ap.add_argument("--steps-per-episode", type=int, default=120)
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--agents", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--kernel-lanes", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--kernel-agents", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--kernel-rounds", type=int, default=200)
    ap.add_argument("--skip", type=int, default=8)
    ap.add_argument("--steps-seq", type=int, default=128)
    ap.add_argument("--steps-lane", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rnn_team_timing.txt"))
    ap.add_argument("--sized", type=int, nargs=4, default=None, metavar=("HID", "POL", "VAL", "REC"),
                    help="also the rows of sized_rows() at these widths (scripts/time_rnn_team_collect.py records them at 32 64 64 16)")
    args = ap.parse_args()
    from radiation_ppo_amd.evaluate import run_test_environments_rnn, run_test_environments_rnn_team, sample_test_environments
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    L = args.steps_per_episode
    assert args.skip + args.steps_lane < L and args.skip + args.steps_seq < L * args.runs
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.warmup} warm-up + {args.repeats} timed repeats, seed {args.seed}; "
        "min median max")
    say(f"# 1. the policy round: wall ms per round over {args.kernel_rounds} rounds issued back to back, all lanes active")
    for N in args.kernel_lanes:
        for A in args.kernel_agents:
            r = kernel_ab(N, A, args.kernel_rounds, args.warmup, args.repeats)
            for name in ("team", "per-agent"):
                say(f"policy round lanes {N:6d} agents {A} {name:9s} | ms per round {mmm(r[name])}")
            t, b = r["team"], r["per-agent"]
            say(f"policy round lanes {N:6d} agents {A} team slowest {max(t):.4f} ms, per-agent fastest {min(b):.4f} ms -> "
                f"{'faster' if max(t) < min(b) else 'NOT faster'}; median / median = {statistics.median(b) / statistics.median(t):.2f} x")
    say(f"# 2. the runner: {args.envs} saved environments x {args.runs} runs of {L} steps; wall ms per lock-step over lock-steps {args.skip}.."
        f"{args.skip + args.steps_seq - 1} (sequential) / {args.skip}..{args.skip + args.steps_lane - 1} (lane-per-run) of a run")
    team = {}
    for a in range(max(args.agents)):
        torch.manual_seed(args.seed + a)
        team[a] = RNNAgentPPO(id=a, steps_per_episode=L)
    for obst in (0, args.obstructions):
        sets = sample_test_environments(args.envs, obstruction_count=obst, seed=args.seed)
        common = dict(montecarlo_runs=args.runs, steps_per_episode=L, obstruction_count=obst, seed=args.seed)
        one = per_step_ms(lambda: run_test_environments_rnn(team[0], sets, carry_hidden_across_runs=True, fused=True, **common),
                          args.skip, args.steps_seq, args.warmup, args.repeats)
        say(f"sequential   lanes {args.envs:6d} agents 1 obstruction_count {obst} fused    | ms per lock-step {mmm(one)} | run_test_environments_rnn")
        for A in args.agents:
            agents = {a: team[a] for a in range(A)}
            for mode, carry, lanes, window in (("sequential", True, args.envs, args.steps_seq),
                                               ("lane-per-run", False, args.envs * args.runs, args.steps_lane)):
                res = {}
                for name, fused in (("fused", True), ("composed", False)):
                    run = lambda: run_test_environments_rnn_team(agents, sets, carry_hidden_across_runs=carry, fused=fused, **common)
                    res[name] = per_step_ms(run, args.skip, window, args.warmup, args.repeats)
                    say(f"{mode:12s} lanes {lanes:6d} agents {A} obstruction_count {obst} {name:8s} | ms per lock-step {mmm(res[name])} | "
                        f"{lanes * A / statistics.median(res[name]) / 1e3:8.2f} M agent steps/s (median)")
                f, b = res["fused"], res["composed"]
                say(f"{mode:12s} lanes {lanes:6d} agents {A} obstruction_count {obst} fused slowest {max(f):.4f} ms, composed fastest {min(b):.4f} ms"
                    f" -> {'faster' if max(f) < min(b) else 'NOT faster'}; median / median = {statistics.median(b) / statistics.median(f):.2f} x")
                if carry:
                    fm, om = statistics.median(f), statistics.median(one)
                    say(f"{mode:12s} lanes {lanes:6d} agents {A} obstruction_count {obst} fused median {fm:.4f} ms against {A} x the one-agent "
                        f"fused median {om:.4f} ms = {A * om:.4f} ms -> {'within' if fm <= A * om else 'NOT within'} ({fm / om:.2f} x one agent)")
    if args.sized:
        sized_rows(say, tuple(args.sized[:3]), args.sized[3], [1] + args.agents, args.envs, args.runs, L, args.obstructions, args.skip,
                   args.steps_seq, args.warmup, args.repeats, args.seed, args.kernel_lanes, args.kernel_agents, args.kernel_rounds)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
