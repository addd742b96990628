"""A recurrent (RAD-A2C) team's policy round as one launch (rs_rnn_team_step / rs_rnn_sized_team_step) against one K14 / sized-step
launch per agent, at the workload's size: --envs envs, A = 1, 2, 4, 8 agents, the default widths (GRU 24, heads 32 / 32, PFGRU 24) and
--sized (32 64 64, PFGRU 16).  Plain text on stdout and in profiles/rnn_team_collect_timing.txt.  Three measurements:

1. The policy round alone, as the collector issues it: the step round (act, act8, log-probability and value, no mask) and the
   bootstrap round (mask: one env in --episode-steps, what a steady collector cuts per lock-step).  --rounds rounds are issued back to
   back on one stream between two device synchronisations; wall span over rounds, host issue time included.
2. One collector epoch (RNNCollector.collect: --steps lock-steps, episodes of --episode-steps steps, through the captured graph, GAE
   included), use_team_step on against off -- off is the per-agent form, the code before the team step.  Two collectors in one
   process, their epochs alternated; obstacle-free and with --obstructions obstructions.  With one agent `on` is forced (the default
   for one agent is off: bench.py's RAD-A2C leg).
3. scripts/time_eval_rnn_team.py's sized_rows(): the evaluation's policy round and fused lock-step at the sized width, before and after.

--warmup untimed repeats, then --repeats timed ones of each form: min median max, and the team form's slowest repeat against the
per-agent form's fastest."""
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

from time_eval_rnn import mmm
from time_eval_rnn_team import sized_rows


def verdict(team, per_agent):
    return (f"team slowest {max(team):.4f} ms, per-agent fastest {min(per_agent):.4f} ms -> {'faster' if max(team) < min(per_agent) else 'NOT faster'}; "
            f"median / median = {statistics.median(per_agent) / statistics.median(team):.2f} x")


def round_ab(N, A, widths, boot_every, rounds, warmup, repeats):
    """{(round, form): [wall ms per policy round]}: the collector's step and bootstrap rounds, team launch and A per-agent launches"""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N + A)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)
    hid = widths[0] if widths else 24
    W = [(rnd(lib.rs_rnn_sized_weight_floats(*widths) if widths else 5296) - 0.5) * 0.5 for _ in range(A)]
    x, loc, u, h = rnd(N, A, 11), rnd(N, A, 2), rnd(N, A), rnd(A, N, hid) - 0.5
    boot = (torch.arange(N, device=dev) % boot_every == 0).to(torch.uint8)
    act8 = torch.zeros(N, A, dtype=torch.int8, device=dev)
    act = torch.zeros(A, N, dtype=torch.int64, device=dev)
    f = torch.zeros(A, 3, N, device=dev)
    p = lambda t: t.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    wp = (C.c_void_p * A)(*[p(w) for w in W])
    sized = (lambda fn, w, *tail: fn(w, *widths, *tail)) if widths else (lambda fn, w, *tail: fn(w, *tail))
    team_fn = lib.rs_rnn_sized_team_step if widths else lib.rs_rnn_team_step

    def team(step):
        if step:
            _lib.check(team_fn(wp, A, *(widths or ()), p(x), p(loc), p(h), p(u), p(act), p(f), p(act8), None, N, st), "team step round")
        else:
            _lib.check(team_fn(wp, A, *(widths or ()), p(x), p(loc), p(h), None, None, p(f), None, p(boot), N, st), "team bootstrap round")

    def per_agent(step):
        for a in range(A):
            ha, fa = p(h) + 4 * a * N * hid, p(f) + 4 * a * 3 * N
            rows = (p(x) + 44 * a, 11 * A, p(loc) + 8 * a, 2 * A, ha)
            logits = (None,) if widths else ()
            fn = lib.rs_rnn_sized_step if widths else lib.rs_rnn_policy_step_rows
            if step:
                _lib.check(sized(fn, p(W[a]), *rows, p(u) + 4 * a, A, ha, *logits, fa + 4 * N, p(act) + 8 * a * N, fa, p(act8) + a, A, None, N, st),
                           "per-agent step round")
            else:
                _lib.check(sized(fn, p(W[a]), *rows, None, A, None, *logits, fa + 8 * N, None, None, None, A, p(boot), N, st),
                           "per-agent bootstrap round")
    out = {}
    for rname, step in (("step", True), ("bootstrap", False)):
        res = {"team": [], "per-agent": []}
        for i in range(warmup + repeats):
            for name, fn in (("team", team), ("per-agent", per_agent)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(rounds):
                    fn(step)
                torch.cuda.synchronize()
                if i >= warmup:
                    res[name].append((time.perf_counter() - t0) / rounds * 1e3)
        for name, v in res.items():
            out[rname, name] = v
    return out


def epoch_ab(N, A, T, L, obst, ac_args, warmup, repeats, seed):
    """{form: [wall ms per collector epoch]}, the two forms' epochs alternated"""
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector
    cols = {}
    for name, on in (("team", True), ("per-agent", False)):
        torch.manual_seed(seed)
        env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=seed)
        agents = {a: RNNAgentPPO(id=a, steps_per_epoch=T, steps_per_episode=L, seed=seed + a, actor_critic_args=ac_args) for a in range(A)}
        cols[name] = RNNCollector(env, agents, T, L)
        assert cols[name].use_glue and cols[name].use_team_step == (A >= 2)
        cols[name].use_team_step = on
    res = {name: [] for name in cols}
    for i in range(warmup + repeats):
        for name, col in cols.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            col.collect()
            torch.cuda.synchronize()
            if i >= warmup:
                res[name].append((time.perf_counter() - t0) * 1e3)
    assert all(col.env.error_flags() == 0 for col in cols.values())
    assert torch.equal(cols["team"].buf.act, cols["per-agent"].buf.act) and torch.equal(cols["team"].buf.val, cols["per-agent"].buf.val)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--sized", type=int, nargs=4, default=[32, 64, 64, 16], metavar=("HID", "POL", "VAL", "REC"))
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--steps", type=int, default=480)
    ap.add_argument("--episode-steps", type=int, default=120)
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--eval-envs", type=int, default=1000)
    ap.add_argument("--eval-runs", type=int, default=100)
    ap.add_argument("--eval-agents", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnn_team_collect_timing.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    hid, pol, val, rec = args.sized
    families = (("default", None, None),
                ("sized", (hid, pol, val), dict(hidden=((hid,),), hidden_sizes_pol=((pol,),), hidden_sizes_val=((val,),), hidden_sizes_rec=(rec,))))
    N, T, L = args.envs, args.steps, args.episode_steps
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.warmup} warm-up + {args.repeats} timed repeats of each form, "
        f"alternated, seed {args.seed}; min median max; default = GRU 24 / heads 32 / 32 / PFGRU 24, sized = GRU {hid} / heads {pol} / {val} / "
        f"PFGRU {rec}")
    say(f"# 1. the collector's policy round alone at {N} envs: wall ms per round over {args.rounds} rounds issued back to back; bootstrap "
        f"mask: one env in {L}")
    for fam, widths, _ in families:
        for A in args.agents:
            r = round_ab(N, A, widths, L, args.rounds, args.warmup, args.repeats)
            for rname in ("step", "bootstrap"):
                for name in ("team", "per-agent"):
                    say(f"{fam:7s} {rname:9s} round envs {N} agents {A} {name:9s} | ms per round {mmm(r[rname, name])}")
                say(f"{fam:7s} {rname:9s} round envs {N} agents {A} {verdict(r[rname, 'team'], r[rname, 'per-agent'])}")
    say(f"# 2. one collector epoch (RNNCollector.collect, captured lock-step): {N} envs, {T} lock-steps, episodes of {L} steps; wall ms per epoch")
    for fam, _, ac_args in families:
        for obst in (0, args.obstructions):
            for A in args.agents:
                r = epoch_ab(N, A, T, L, obst, ac_args, args.warmup, args.repeats, args.seed)
                for name in ("team", "per-agent"):
                    say(f"{fam:7s} epoch envs {N} agents {A} obstruction_count {obst} {name:9s} | ms per epoch {mmm(r[name])} | "
                        f"{N * T * A / statistics.median(r[name]) / 1e3:8.2f} M agent steps/s (median)")
                say(f"{fam:7s} epoch envs {N} agents {A} obstruction_count {obst} {verdict(r['team'], r['per-agent'])}")
    say("# 3. the evaluation at the sized widths (scripts/time_eval_rnn_team.py: sized_rows)")
    sized_rows(say, (hid, pol, val), rec, args.eval_agents, args.eval_envs, args.eval_runs, L, args.obstructions, 8, 128, args.warmup,
               args.repeats, args.seed, [args.eval_envs], [a for a in args.agents if a > 1], args.rounds)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
