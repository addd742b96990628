"""The gradient-search evaluation (evaluate.run_test_environments_gradient_search) at the reference's sizes: what the look-ahead over
8 moves costs per lock-step in three forms, on the same envs in the same session:

  fused     rs_gs_eval_step: look-ahead, gradient, draw and idle rows in one launch
  composed  rs_peek, then the gradient, log-softmax, cumsum, compare and idle rule in torch
  parent    the look-ahead as the API before rs_peek allows it: RadSearchVec.snapshot(), eight rs_step with the action rows
            16 + k, after each a copy of x, y, aflags and the readings (what a controller needs of the move), RadSearchVec.restore()
            -- no gradient and no draw, so this form is charged less than a controller built on it would pay

--lanes lanes (1000 and 100 000: 1000 saved environments x 1 / x 100 runs), --agents agents each, obstacle-free and with
--obstructions obstructions.  Every lane is mid-episode and running (all eight moves are looked at on every lane), the forms are
timed in turn within each repeat -- a device synchronise, --iters rounds, a device synchronise; wall milliseconds per round = span /
iters, host issue time included -- with --warmup untimed turns and --repeats timed ones: min / median / max.  Then, through the
runner itself with q = 1e30 (a random walk: the look-ahead costs the same and hardly a lane finishes), the wall time of a whole
lock-step (rs_action_uniforms, the round, rs_step, the bookkeeping) fused and composed, clocked as scripts/time_eval_team.py does.
Per configuration the fused form's slowest repeat is held against each other form's fastest.  Plain text on stdout and in
profiles/eval_gs_timing.txt."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from time_eval_team import mmm, per_step_ms


def rounds(vec, obs, q):
    """the three forms of one policy round on vec's present state, as callables"""
    from radiation_ppo_amd import _lib
    N, A, dev = vec.num_envs, vec.number_agents, vec.device
    p = lambda t: t.data_ptr()
    u = vec.action_uniforms(torch.empty(N, A, device=dev))
    alive = torch.ones(N, dtype=torch.bool, device=dev)
    alive8, a8 = alive.view(torch.uint8), torch.empty(N, A, dtype=torch.int8, device=dev)
    st, q_rec = vec._stream(), 1 / q

    def fused():
        _lib.check(vec.lib.rs_gs_eval_step(vec._h, p(obs), q_rec, p(u), p(alive8), p(a8), None, st), "rs_gs_eval_step")

    def composed():
        _, moved, _, meas = vec.peek(lam=False)
        g = ((meas.double() - obs[..., 0:1].double()) * 0.01 * q_rec).float()
        g = torch.where(moved.bool(), g, torch.zeros_like(g))
        cdf = torch.cumsum(torch.exp(torch.log_softmax(g, dim=-1)), dim=-1)
        act = (cdf[..., :-1] <= u.unsqueeze(-1)).sum(dim=-1)
        a8.copy_(torch.where(alive.view(N, 1), act, torch.full_like(act, 8)).to(torch.int8))
    rows = [torch.full((N, A), 16 + k, dtype=torch.int8, device=dev) for k in range(8)]
    cx, cy = torch.empty(8, A, N, dtype=torch.int32, device=dev), torch.empty(8, A, N, dtype=torch.int32, device=dev)
    cf, cm = torch.empty(8, A, N, dtype=torch.uint8, device=dev), torch.empty(8, N, A, device=dev)

    def parent():
        snap = vec.snapshot()
        for k in range(8):
            vec.step(rows[k])
            cx[k].copy_(vec.state("x")); cy[k].copy_(vec.state("y")); cf[k].copy_(vec.state("aflags")); cm[k].copy_(vec.obs[..., 0])
            vec.restore(snap)
    return {"fused": fused, "composed": composed, "parent": parent}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--runs", type=int, nargs="+", default=[1, 100])
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_gs_timing.txt"))
    args = ap.parse_args()
    from radiation_ppo_amd import evaluate
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    say(f"# {args.envs} saved environments x runs = lanes; wall ms per policy round over {args.iters} rounds between device synchronises, and per "
        f"whole lock-step over lock-steps {args.skip}..{args.skip + args.steps - 1} of a run at q = 1e30; {args.warmup} warm-up + {args.repeats} "
        f"timed repeats, the forms in turn within a repeat; seed {args.seed}; min median max")
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for obst in (0, args.obstructions):
        sets = evaluate.sample_test_environments(args.envs, obstruction_count=obst, seed=args.seed)
        for R in args.runs:
            for A in args.agents:
                lanes = args.envs * R
                tag = f"lanes {lanes:6d} agents {A} obstruction_count {obst}"
                vec, _, _, obs, _ = evaluate._open(sets, R, A, obst, True, args.seed, "cuda:0", welford=False)
                g = torch.Generator(device="cuda").manual_seed(args.seed)
                for _ in range(3):                                 # mid-episode: the agents of a team apart, past the first step
                    obs = vec.step(torch.randint(0, 8, (lanes, A), generator=g, device="cuda").to(torch.int8))[0]
                forms = rounds(vec, obs.clone(), 1.0)
                res = {name: [] for name in forms}
                for i in range(args.warmup + args.repeats):
                    for name, fn in forms.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.iters):
                            fn()
                        torch.cuda.synchronize()
                        if i >= args.warmup:
                            res[name].append((time.perf_counter() - t0) / args.iters * 1e3)
                for name in forms:
                    say(f"{tag} round {name:9s} | ms per round {mmm(res[name])}")
                for name in ("composed", "parent"):
                    f, b = res["fused"], res[name]
                    say(f"{tag} round: fused slowest {max(f):.4f} ms, {name} fastest {min(b):.4f} ms -> "
                        f"{'faster' if max(f) < min(b) else 'SLOWER' if min(f) > max(b) else 'NOT faster'}; median / median = "
                        f"{statistics.median(b) / statistics.median(f):.2f} x")
                del vec, forms
                common = dict(number_of_agents=A, q=1e30, montecarlo_runs=R, obstruction_count=obst, seed=args.seed)
                step = {name: per_step_ms(lambda L, fz=fz: evaluate.run_test_environments_gradient_search(sets, steps_per_episode=L, fused=fz, **common),
                                          args.skip, args.steps, args.warmup, args.repeats) for name, fz in (("fused", True), ("composed", False))}
                for name in step:
                    say(f"{tag} lock-step {name:9s} | ms per lock-step {mmm(step[name])} | "
                        f"{lanes / statistics.median(step[name]) / 1e3:8.2f} M lane steps/s (median)")
                f, b = step["fused"], step["composed"]
                say(f"{tag} lock-step: fused slowest {max(f):.4f} ms, composed fastest {min(b):.4f} ms -> "
                    f"{'faster' if max(f) < min(b) else 'SLOWER' if min(f) > max(b) else 'NOT faster'}; median / median = "
                    f"{statistics.median(b) / statistics.median(f):.2f} x")
                flush()
    flush()


if __name__ == "__main__":
    main()
