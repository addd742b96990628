"""Monte-Carlo evaluation of RAD-TEAM (CNN) teams at the reference's size: the cost of ONE lock-step of
evaluate.run_test_environments_cnn_team with fused=True (rs_action_uniforms, the PFGRU step, rs_maps_update, rs_maps_stack,
rs_cnn_team_trunk_infer, rs_cnn_team_eval_head, rs_step, rs_eval_post_step) against fused=False (per agent rs_cnn_trunk_infer, BLAS
linear, rs_cnn_head and the idle rule; torch bookkeeping) and against today's evaluate.run_test_environments_cnn (library ops
throughout, a host read every lock-step).

--envs saved environments x --runs Monte-Carlo runs = lanes (1000 x 100 = 100 000 and 1000 x 1), --agents agents each, once
obstacle-free and once with --obstructions obstructions.  The clock is read inside the run, as scripts/time_eval_team.py does: every
form draws its uniforms (RadSearchVec.action_uniforms) exactly once per lock-step, and the script wraps that method for the time of the
measurement -- at lock-step --skip it synchronises the device and starts the clock, at lock-step --skip + --steps it synchronises and
stops it.  Wall milliseconds per lock-step = that span / --steps, host issue time and the periodic host read included.  --warmup
untimed runs, then --repeats timed ones: min / median / max, one line per (configuration, form); then the fused form's slowest
against each baseline's fastest.

Then the two new kernels alone at the largest lane count, by device events over --kernel-reps launches after an untimed pass: the team
trunk against A x rs_cnn_trunk_infer, the team head against A x (BLAS linear + rs_cnn_head).  Plain text on stdout and in
profiles/eval_cnn_timing.txt."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from time_eval_team import mmm, per_step_ms


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def kernels_alone(N, A, reps, say):
    """the policy round's two kernels on random maps, N lanes, A agents"""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import CNNActor, cnn_head_params, cnn_trunk_prepare
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()
    torch.manual_seed(A)
    seqs = [CNNActor().cuda().actor for _ in range(A)]
    maps = torch.rand(N, 4, 27, 27, device="cuda") * (torch.rand(N, 4, 27, 27, device="cuda") < 0.1)
    cells = torch.randint(0, 729, (N, A), device="cuda")
    pcells = torch.randint(-1, 729, (N, A), device="cuda")
    c32, p32 = cells.int().contiguous(), pcells.int().contiguous()
    u = torch.rand(N, A, device="cuda")
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    act8 = torch.empty(N, A, dtype=torch.int8, device="cuda")
    wt = torch.empty(A, lib.rs_cnn_trunk_scratch_floats(6), dtype=torch.float32, device="cuda")
    for a, s in enumerate(seqs):
        cnn_trunk_prepare(s, 6, wt[a], st)
    a2 = torch.empty(A, N, 2704, device="cuda")
    heads = (_lib.RsCnnHeadParams * A)(*[cnn_head_params(s) for s in seqs])

    def team_trunk():
        _lib.check(lib.rs_cnn_team_trunk_infer(p(maps), p(c32), p(p32), A, N, p(wt), p(a2), st), "rs_cnn_team_trunk_infer")

    def per_agent_trunk():
        for a in range(A):
            _lib.check(lib.rs_cnn_trunk_infer(p(maps), p(cells), p(pcells), A, a, N, p(wt[a]), p(a2[a]), st), "rs_cnn_trunk_infer")

    def team_head():
        _lib.check(lib.rs_cnn_team_eval_head(heads, A, p(a2), p(u), p(alive), p(act8), None, None, None, N, st), "rs_cnn_team_eval_head")

    def per_agent_head():
        with torch.no_grad():
            for a, s in enumerate(seqs):
                y1 = torch.nn.functional.linear(a2[a], s[6].weight, s[6].bias)
                _lib.check(lib.rs_cnn_head(p(y1), p(s[8].weight), p(s[8].bias), p(s[10].weight), p(s[10].bias), 8, p(u) + 4 * a, A, None, None,
                                           p(act8) + a, A, None, 1, 0, None, N, st), "rs_cnn_head")
    res = {}
    forms = (("rs_cnn_team_trunk_infer", team_trunk), (f"{A} x rs_cnn_trunk_infer", per_agent_trunk),
             ("rs_cnn_team_eval_head", team_head), (f"{A} x (BLAS linear + rs_cnn_head)", per_agent_head))
    for _, fn in forms:                                  # one untimed pass over all four: whichever is timed first would otherwise pay
        event_ms(fn, reps)                               # for the clocks and caches the allocations above left cold
    for name, fn in forms:
        res[name] = event_ms(fn, reps)
        say(f"kernels alone lanes {N} agents {A} {name:32s} | ms {mmm(res[name])}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--runs", type=int, nargs="+", default=[100, 1])
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--skip", type=int, default=8)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_cnn_timing.txt"))
    args = ap.parse_args()
    from radiation_ppo_amd.evaluate import run_test_environments_cnn, run_test_environments_cnn_team, sample_test_environments
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    say(f"# {args.envs} saved environments x {args.runs} runs; wall ms per lock-step over lock-steps {args.skip}..{args.skip + args.steps - 1} of a "
        f"run; {args.warmup} warm-up + {args.repeats} timed repeats, seed {args.seed}; min median max")
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for runs in args.runs:
        for obst in (0, args.obstructions):
            sets = sample_test_environments(args.envs, obstruction_count=obst, seed=args.seed)
            for A in args.agents:
                torch.manual_seed(args.seed)
                agents = {a: CNNAgentPPO(id=a) for a in range(A)}
                common = dict(montecarlo_runs=runs, obstruction_count=obst, seed=args.seed)
                forms = {"fused": lambda L: run_test_environments_cnn_team(agents, sets, steps_per_episode=L, fused=True, **common),
                         "composed": lambda L: run_test_environments_cnn_team(agents, sets, steps_per_episode=L, fused=False, **common),
                         "run_test_environments_cnn": lambda L: run_test_environments_cnn(agents, sets, steps_per_episode=L, **common)}
                res = {}
                tag = f"lanes {args.envs * runs} agents {A} obstruction_count {obst}"
                for name, run in forms.items():
                    res[name] = per_step_ms(run, args.skip, args.steps, args.warmup, args.repeats)
                    say(f"{tag} {name:25s} | ms per lock-step {mmm(res[name])} | "
                        f"{args.envs * runs / statistics.median(res[name]) / 1e3:8.2f} M lane steps/s (median)")
                for name in forms:
                    if name != "fused":
                        f, b = res["fused"], res[name]
                        say(f"{tag} fused slowest {max(f):.4f} ms, {name} fastest {min(b):.4f} ms -> "
                            f"{'faster' if max(f) < min(b) else 'NOT faster'}; median / median = {statistics.median(b) / statistics.median(f):.2f} x")
                flush()
                torch.cuda.empty_cache()
    for A in args.agents:
        res = kernels_alone(args.envs * max(args.runs), A, args.kernel_reps, say)
        names = list(res)
        for new, old in ((names[0], names[1]), (names[2], names[3])):
            say(f"kernels alone agents {A} {new} slowest {max(res[new]):.4f} ms, {old} fastest {min(res[old]):.4f} ms -> "
                f"{'faster' if max(res[new]) < min(res[old]) else 'NOT faster'}; median / median = "
                f"{statistics.median(res[old]) / statistics.median(res[new]):.2f} x")
        flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
