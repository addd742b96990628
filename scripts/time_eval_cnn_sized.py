"""Monte-Carlo evaluation of RAD-TEAM (CNN) teams WITHOUT enforced walls (147 x 147 heat maps for 120-step episodes): the cost of ONE
lock-step of evaluate.run_test_environments_cnn_team_sized with fused=True (rs_action_uniforms, the PFGRU step, rs_maps_update,
rs_maps_stack, rs_cnn_sized_team_infer, rs_cnn_sized_team_eval_head, rs_step, rs_eval_post_step) against fused=False (per agent
rs_cnn_sized_infer, BLAS linear, rs_cnn_head and the idle rule; torch bookkeeping) and against evaluate.run_test_environments_cnn
(library ops throughout, a host read every lock-step), the method of scripts/time_eval_cnn.py: the clock is read inside the run, at
lock-steps --skip and --steps-per-episode - 1, wall milliseconds per lock-step in between, --warmup untimed runs, then --repeats timed
ones: min / median / max per (configuration, form), then the fused form's slowest against each baseline's fastest.

--lanes saved environments x 1 run each, --agents agents each, once obstacle-free and once with --obstructions obstructions; the first
lane count is the reference's 1000, the last one (--big-lanes; 0 = computed) the largest that fits next to the heat maps' own state: the
script prints that state's bytes per lane (rs_maps_state_bytes, HeatMaps' two stack buffers, the composed forms' a2) and the count
that fits into --memory-share of the free device memory.

Then the two kernels alone, by device events over --kernel-reps launches after an untimed pass:
  * rs_cnn_sized_team_infer against A x rs_cnn_sized_infer on the maps of a walls-off run (--trunk-lanes lanes, uniformly random
    actions) at lock-steps 1, 30 and 120, with the share of (agent, image, tile) units whose input window is empty (counted on the host
    from the same maps: the units that skip conv1), and on dense random maps, where no unit does;
  * rs_cnn_sized_team_eval_head against A x (BLAS linear + rs_cnn_head) at depth 85 264.
Plain text on stdout and in profiles/eval_cnn_sized_timing.txt."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from time_eval_cnn import event_ms
from time_eval_team import mmm, per_step_ms


def empty_window_share(maps, cells, pcells):
    """the share of (agent, image, tile) units that skip conv1: every element of the tile's 38 x 38 x 4 input window == 0 and neither of
    the agent's cells inside it (the rule of rs_cnn_sized_team_infer, on the host)"""
    N, _, M, _ = maps.shape
    A = cells.shape[1]
    nt = (M // 2 + 15) // 16
    nz = (maps != 0).any(dim=1)
    skipped = 0
    for ty in range(nt):
        for tx in range(nt):
            r0, c0 = 32 * ty - 3, 32 * tx - 3
            empty = ~nz[:, max(r0, 0):r0 + 38, max(c0, 0):c0 + 38].flatten(1).any(dim=1)
            for a in range(A):
                hit = torch.zeros(N, dtype=torch.bool, device=maps.device)
                for at in (cells[:, a], pcells[:, a]):
                    r, c = torch.div(at, M, rounding_mode="floor") - r0, at % M - c0
                    hit |= (at >= 0) & (r >= 0) & (r < 38) & (c >= 0) & (c < 38)
                skipped += int((empty & ~hit).sum())
    return skipped / (N * A * nt * nt)


def run_maps(N, A, L, obst, seed, at_steps):
    """{lock-step: (shared maps, cells, pcells)} of a walls-off run of N lanes under uniformly random actions, as the runner sees them
    at that lock-step (1 = the first policy round)"""
    from radiation_ppo_amd.evaluate import _open, sample_test_environments
    from radiation_ppo_amd.maps import HeatMaps
    from radiation_ppo_amd.pfgru import PredictorBank
    sets = sample_test_environments(N, obstruction_count=obst, enforce_grid_boundaries=False, seed=seed)
    vec, _, _, obs, _ = _open(sets, 1, A, obst, False, seed, "cuda:0", welford=False)
    maps = HeatMaps(vec, L, enforce_boundaries=False)
    bank = PredictorBank(N, A, seed=seed, device=torch.device("cuda:0"))
    bank.reset()
    u = torch.empty(N, A, dtype=torch.float32, device="cuda")
    out = {}
    for t in range(1, L + 1):
        pred = bank.predict_kernel(obs)
        bank.calls.add_(1)
        maps.update(obs, pred=pred)
        if t in at_steps:
            out[t] = (maps.shared_maps().clone(), maps.field("cell").clone(), maps.field("pred_cell").clone())
        vec.action_uniforms(u)
        obs = vec.step((u * 8).clamp_(max=7).to(torch.int8))[0].clone()
    return out


def trunk_alone(A, snaps, reps, say):
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import CNNActor, cnn_conv_params
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()
    torch.manual_seed(A)
    for name, (maps, c32, p32) in snaps.items():
        N, _, M, _ = maps.shape
        seqs = [CNNActor(map_dim=(M, M)).cuda().actor for _ in range(A)]
        convs = (_lib.RsCnnConvParams * A)(*[cnn_conv_params(s) for s in seqs])
        c64, p64 = c32.long().contiguous(), p32.long().contiguous()
        a2 = torch.empty(A, N, 16 * (M // 2) ** 2, device="cuda")

        def team():
            _lib.check(lib.rs_cnn_sized_team_infer(p(maps), p(c32), p(p32), A, N, M, convs, p(a2), st), "rs_cnn_sized_team_infer")

        def per_agent():
            for a, s in enumerate(seqs):
                _lib.check(lib.rs_cnn_sized_infer(p(maps), p(c64), p(p64), A, a, N, M, p(s[0].weight), p(s[0].bias), p(s[3].weight), p(s[3].bias),
                                                  p(a2[a]), st), "rs_cnn_sized_infer")
        share = empty_window_share(maps, c32.long(), p32.long())
        for fn in (team, per_agent):
            event_ms(fn, reps)
        t, o = event_ms(team, reps), event_ms(per_agent, reps)
        say(f"trunk alone lanes {N} agents {A} side {M} {name:18s} empty-window units {100 * share:5.1f} % | rs_cnn_sized_team_infer ms {mmm(t)} | "
            f"{A} x rs_cnn_sized_infer ms {mmm(o)} | slowest {max(t):.4f} against fastest {min(o):.4f} -> "
            f"{'faster' if max(t) < min(o) else 'NOT faster'}; median / median = {statistics.median(o) / statistics.median(t):.2f} x")


def head_alone(N, A, M, reps, say):
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import CNNActor, cnn_head_params
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()
    torch.manual_seed(A)
    flat = 16 * (M // 2) ** 2
    seqs = [CNNActor(map_dim=(M, M)).cuda().actor for _ in range(A)]
    heads = (_lib.RsCnnHeadParams * A)(*[cnn_head_params(s) for s in seqs])
    a2 = torch.rand(A, N, flat, device="cuda") * (torch.rand(A, N, flat, device="cuda") < 0.3)
    u = torch.rand(N, A, device="cuda")
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    act8 = torch.empty(N, A, dtype=torch.int8, device="cuda")

    def team():
        _lib.check(lib.rs_cnn_sized_team_eval_head(heads, A, flat, p(a2), p(u), p(alive), p(act8), None, None, None, N, st),
                   "rs_cnn_sized_team_eval_head")

    def per_agent():
        with torch.no_grad():
            for a, s in enumerate(seqs):
                y1 = torch.nn.functional.linear(a2[a], s[6].weight, s[6].bias)
                _lib.check(lib.rs_cnn_head(p(y1), p(s[8].weight), p(s[8].bias), p(s[10].weight), p(s[10].bias), 8, p(u) + 4 * a, A, None, None,
                                           p(act8) + a, A, None, 1, 0, None, N, st), "rs_cnn_head")
    for fn in (team, per_agent):
        event_ms(fn, reps)
    t, o = event_ms(team, reps), event_ms(per_agent, reps)
    say(f"head alone lanes {N} agents {A} depth {flat} | rs_cnn_sized_team_eval_head ms {mmm(t)} | {A} x (BLAS linear + rs_cnn_head) ms {mmm(o)} | "
        f"slowest {max(t):.4f} against fastest {min(o):.4f} -> {'faster' if max(t) < min(o) else 'NOT faster'}; median / median = "
        f"{statistics.median(o) / statistics.median(t):.2f} x")


def lanes_that_fit(A, L, M, share):
    """(bytes per lane, lanes): the heat maps' state, HeatMaps' actor and critic stack buffers and one agent's a2 of all lanes (what the
    composed runner allocates) per lane, and the count that fits into `share` of the free device memory, in whole thousands"""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    per_lane = lib.rs_maps_state_bytes(1000, A, L, M, M) / 1000 + 4 * M * M * (6 * A + 4) + 4 * 16 * (M // 2) ** 2
    free, _ = torch.cuda.mem_get_info()
    return per_lane, int(free * share / per_lane) // 1000 * 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1000)
    ap.add_argument("--big-lanes", type=int, default=0)
    ap.add_argument("--memory-share", type=float, default=0.8)
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--steps-per-episode", type=int, default=120)
    ap.add_argument("--skip", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--trunk-lanes", type=int, default=256)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--only", choices=("runs", "kernels"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_cnn_sized_timing.txt"))
    args = ap.parse_args()
    from radiation_ppo_amd.evaluate import run_test_environments_cnn, run_test_environments_cnn_team_sized, sample_test_environments
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO
    L, M = args.steps_per_episode, 27 + args.steps_per_episode
    steps = L - 1 - args.skip
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    written = [0]

    def flush():                                             # --only kernels adds to the file that --only runs wrote
        with open(args.out, "a" if written[0] or args.only == "kernels" else "w") as fh:
            fh.write("\n".join(lines[written[0]:]) + "\n")
        written[0] = len(lines)
    say(f"# walls off, {L}-step episodes: {M} x {M} heat maps; wall ms per lock-step over lock-steps {args.skip}..{L - 2} of a run; "
        f"{args.warmup} warm-up + {args.repeats} timed repeats, seed {args.seed}; min median max")
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for A in args.agents:
        per_lane, fit = lanes_that_fit(A, L, M, args.memory_share)
        say(f"# {A} agents: {per_lane / 1e6:.2f} MB per lane (maps state, stack buffers, one a2 row); {fit} lanes fit into "
            f"{args.memory_share:.0%} of the free device memory")
    if args.only != "kernels":
        big = args.big_lanes or min(lanes_that_fit(max(args.agents), L, M, args.memory_share)[1], 100000)
        for lanes in dict.fromkeys((args.lanes, big)):        # (once where both counts are the same)
            for obst in (0, args.obstructions):
                sets = sample_test_environments(lanes, obstruction_count=obst, enforce_grid_boundaries=False, seed=args.seed)
                for A in args.agents:
                    torch.manual_seed(args.seed)
                    agents = {a: CNNAgentPPO(id=a, map_dim=(M, M)) for a in range(A)}
                    common = dict(montecarlo_runs=1, obstruction_count=obst, enforce_grid_boundaries=False, seed=args.seed)
                    forms = {"fused": lambda _: run_test_environments_cnn_team_sized(agents, sets, steps_per_episode=L, fused=True, **common),
                             "composed": lambda _: run_test_environments_cnn_team_sized(agents, sets, steps_per_episode=L, fused=False, **common),
                             "run_test_environments_cnn": lambda _: run_test_environments_cnn(agents, sets, steps_per_episode=L, **common)}
                    res = {}
                    tag = f"lanes {lanes} agents {A} obstruction_count {obst}"
                    for name, run in forms.items():
                        res[name] = per_step_ms(run, args.skip, steps, args.warmup, args.repeats)
                        say(f"{tag} {name:25s} | ms per lock-step {mmm(res[name])} | "
                            f"{lanes / statistics.median(res[name]) / 1e3:8.2f} M lane steps/s (median)")
                    for name in forms:
                        if name != "fused":
                            f, b = res["fused"], res[name]
                            say(f"{tag} fused slowest {max(f):.4f} ms, {name} fastest {min(b):.4f} ms -> "
                                f"{'faster' if max(f) < min(b) else 'NOT faster'}; median / median = {statistics.median(b) / statistics.median(f):.2f} x")
                    flush()
                    del agents
                    torch.cuda.empty_cache()
    if args.only != "runs":
        for A in args.agents:
            snaps = {f"run, lock-step {t}": (m, c.int().contiguous(), q.int().contiguous())
                     for t, (m, c, q) in run_maps(args.trunk_lanes, A, L, 0, args.seed, (1, 30, L)).items()}
            N = args.trunk_lanes
            snaps["dense random"] = (torch.rand(N, 4, M, M, device="cuda") - 0.3, torch.randint(0, M * M, (N, A), dtype=torch.int32, device="cuda"),
                                     torch.randint(-1, M * M, (N, A), dtype=torch.int32, device="cuda"))
            trunk_alone(A, snaps, args.kernel_reps, say)
            head_alone(args.lanes, A, M, args.kernel_reps, say)
            flush()
            del snaps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
