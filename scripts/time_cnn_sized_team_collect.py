"""A walls-off RAD-TEAM (CNN) team's training round in four launches (rs_cnn_sized_team_infer, the critic trunk(s),
rs_cnn_sized_team_step_head's two stages) against the per-agent round (per agent rs_cnn_sized_infer + BLAS Linear(16 P P, 32) +
rs_cnn_head, then the same per critic), at the walls-off workload's size: --envs envs (512), --side x --side maps (147: episodes of 120
steps), A = 1, 2, 4, 8 agents, a global critic and one critic per agent.  Plain text on stdout and in
profiles/cnn_sized_team_collect_timing.txt (--append: behind what is there, so that the parts can run as separate processes, each under
its own time limit).  Every line names the first layer's slice length (rs_cnn_sized_team_head_slice_floats(); RS_LIB_PATH selects a
library built with -DRS_SK_SLICE=n for the A/B of slice lengths).  --part selects:

kernels  the launches alone, --rounds of them back to back on one stream between two device synchronisations (wall span over rounds,
         host issue time included): the head call of a step round against A x (GEMM + rs_cnn_head) + C x (GEMM + rs_cnn_head), of a
         bootstrap round (mask: one env in --episode-steps) against C x (GEMM + masked rs_cnn_head), and the critic team trunk against C
         launches of rs_cnn_sized_infer(agent = -1).
epochs   one collector epoch (CNNCollector.collect: --steps lock-steps through the captured graph, episodes of --episode-steps steps, GAE
         included), sized_team_round on against off -- off is the per-agent round, the code before the team round.  Two collectors in
         one process, their epochs alternated.  The epoch's stored maps are steps x envs x 4 x side x side x 4 bytes per collector:
         21.2 GB at 120 x 512 x 147 x 147, 42.5 GB for the two (the a2 rows and the scratch add 2.8 GB at 8 agents with own critics).

--warmup untimed repeats, then --repeats timed ones of each form: min median max, and the team form's slowest repeat against the
per-agent form's fastest."""
import argparse
import ctypes as C
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from time_cnn_team_collect import ab, verdict
from time_eval_rnn import mmm


def kernels_ab(N, M, A, nc, boot_every, rounds, warmup, repeats):
    """{(what, form): [wall ms per call]} for the step heads, the bootstrap heads and the critic trunks of A agents and nc critics"""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import CNNActor, CNNCritic, cnn_conv_params, cnn_head_params
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(N + 10 * A + nc)
    flat = 16 * (M // 2) ** 2
    actors = [CNNActor(map_dim=(M, M)).to(dev).actor for _ in range(A)]
    critics = [CNNCritic(map_dim=(M, M)).to(dev).critic for _ in range(nc)]
    p = lambda t: t.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    hpa, hpc = (_lib.RsCnnHeadParams * A)(*map(cnn_head_params, actors)), (_lib.RsCnnHeadParams * nc)(*map(cnn_head_params, critics))
    cvc = (_lib.RsCnnConvParams * nc)(*map(cnn_conv_params, critics))

    def sparse(*s):                                                 # a trunk's output: non-negative, sparse
        t = torch.rand(*s, device=dev)
        return t.mul_(torch.rand(*s, device=dev) < 0.3)
    a2a, a2c, u = sparse(A, N, flat), sparse(nc, N, flat), torch.rand(N, A, device=dev)
    maps = torch.rand(N, 4, M * M, device=dev) * (torch.rand(N, 4, M * M, device=dev) < 0.02)
    boot = (torch.arange(N, device=dev) % boot_every == 0).to(torch.uint8)
    act, f, act8 = torch.zeros(A, N, dtype=torch.int64, device=dev), torch.zeros(A, 3, N, device=dev), torch.zeros(N, A, dtype=torch.int8, device=dev)
    scratch = torch.empty(lib.rs_cnn_sized_team_head_scratch_floats(flat, A + nc, N), device=dev)
    copies = A if nc == 1 else 1

    def value(c, slot, mask):
        m = critics[c]
        y1 = torch.nn.functional.linear(a2c[c], m[6].weight, m[6].bias)
        _lib.check(lib.rs_cnn_head(p(y1), p(m[8].weight), p(m[8].bias), p(m[10].weight), p(m[10].bias), 1, None, 1, None, None, None, 1,
                                   p(f[c, slot]), copies, 3 * N, mask, N, st), "rs_cnn_head")

    def step_team():
        _lib.check(lib.rs_cnn_sized_team_step_head(hpa, A, hpc, nc, flat, p(a2a), p(a2c), p(u), p(act), p(f), p(act8), None, None, p(scratch),
                                                   scratch.numel(), N, st), "step round")

    def step_per_agent():
        for a, m in enumerate(actors):
            y1 = torch.nn.functional.linear(a2a[a], m[6].weight, m[6].bias)
            _lib.check(lib.rs_cnn_head(p(y1), p(m[8].weight), p(m[8].bias), p(m[10].weight), p(m[10].bias), 8, p(u) + 4 * a, A, p(act[a]),
                                       p(f[a, 0]), p(act8) + a, A, None, 1, 0, None, N, st), "rs_cnn_head")
        for c in range(nc):
            value(c, 1, None)

    def boot_team():
        _lib.check(lib.rs_cnn_sized_team_step_head(None, A, hpc, nc, flat, None, p(a2c), None, None, p(f), None, p(boot), None, p(scratch),
                                                   scratch.numel(), N, st), "bootstrap round")

    def boot_per_agent():
        for c in range(nc):
            value(c, 2, p(boot))

    def trunk_team():
        _lib.check(lib.rs_cnn_sized_team_critic_infer(p(maps), nc, N, M, cvc, p(a2c), st), "rs_cnn_sized_team_critic_infer")

    def trunk_per_agent():
        for c in range(nc):
            cv = cvc[c]
            _lib.check(lib.rs_cnn_sized_infer(p(maps), None, None, 0, -1, N, M, cv.w1, cv.b1, cv.w2, cv.b2, p(a2c[c]), st), "rs_cnn_sized_infer")
    with torch.no_grad():
        out = {}
        for what, team, per in (("step heads", step_team, step_per_agent), ("bootstrap heads", boot_team, boot_per_agent),
                                ("critic trunks", trunk_team, trunk_per_agent)):
            if what == "critic trunks" and nc == 1:
                continue                                        # a global critic's trunk is rs_cnn_sized_infer in both forms
            for name, v in ab({"team": team, "per-agent": per}, rounds, warmup, repeats).items():
                out[what, name] = v
    return out


def epoch_ab(N, A, T, L, obst, global_critic, warmup, repeats, seed):
    """{form: [wall ms per collector epoch]}, the two forms' epochs alternated; and the maps' side"""
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic, heat_map_geometry
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    cols = {}
    for name, on in (("team", True), ("per-agent", False)):
        torch.manual_seed(seed)
        env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=False, seed=seed)
        kw = dict(map_dim=tuple(heat_map_geometry(env, L, False)[2]))
        gcr = CNNCritic(**kw).cuda() if global_critic else None
        agents = {i: CNNAgentPPO(id=i, GlobalCritic=gcr, GlobalCriticOptimizer=torch.optim.Adam(gcr.parameters(), lr=1e-3) if gcr is not None else None,
                                 **kw) for i in range(A)}
        col = CNNCollector(env, agents, T, L, global_critic_flag=global_critic)
        col.sized_team_round = on
        assert col.use_heads and col.use_sized_team_round == on and not col.use_team_round
        cols[name] = col
    res = {name: [] for name in cols}
    for i in range(warmup + repeats):
        for name, col in cols.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            col.collect()
            torch.cuda.synchronize()
            if i >= warmup:
                res[name].append((time.perf_counter() - t0) * 1e3)
    assert all(col.env.error_flags() == 0 and col._graph is not None for col in cols.values())
    side = cols["team"].maps.map_dimensions[0]
    cols.clear()
    del col
    gc.collect()
    torch.cuda.empty_cache()
    return res, side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "epochs"], required=True)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--side", type=int, default=147, help="kernels: the maps' side (epochs: 27 + --episode-steps)")
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--episode-steps", type=int, default=120)
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_sized_team_collect_timing.txt"))
    args = ap.parse_args()
    from radiation_ppo_amd import _lib
    sl = _lib.load().rs_cnn_sized_team_head_slice_floats()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    N, T, L, M = args.envs, args.steps, args.episode_steps, args.side
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; part {args.part}, agents {args.agents}; slice {sl} floats; {args.warmup} warm-up + "
        f"{args.repeats} timed repeats of each form, alternated, seed {args.seed}; min median max")
    if args.part == "kernels":
        flat = 16 * (M // 2) ** 2
        say(f"# the launches alone at {N} envs, {M} x {M} maps (depth {flat}, {-(-flat // sl)} slices): wall ms per call over {args.rounds} calls "
            f"issued back to back; bootstrap mask: one env in {L}")
        for A in args.agents:
            for nc in sorted({1, A}):
                mode = "global critic" if nc == 1 and A > 1 else ("one critic" if A == 1 else "critic per agent")
                r = kernels_ab(N, M, A, nc, L, args.rounds, args.warmup, args.repeats)
                for what in ("step heads", "bootstrap heads", "critic trunks"):
                    if (what, "team") not in r:
                        continue
                    for name in ("team", "per-agent"):
                        say(f"{what:15s} slice {sl} envs {N} agents {A} {mode:16s} {name:9s} | ms per call {mmm(r[what, name])}")
                    v = verdict(r[what, "team"], r[what, "per-agent"])
                    say(f"{what:15s} slice {sl} envs {N} agents {A} {mode:16s} {v}{'  SLOWER' if 'NOT faster' in v else ''}")
                gc.collect()
                torch.cuda.empty_cache()
    else:
        side = 27 + L
        say(f"# one collector epoch (CNNCollector.collect, captured lock-step), walls off: {N} envs, T = {T} lock-steps, episodes of {L} steps; "
            f"wall ms per epoch; stored maps {T * N * 4 * side * side * 4 / 1e9:.1f} GB per collector")
        for A in args.agents:
            for gcf in ((True,) if A == 1 else (True, False)):
                mode = "one critic" if A == 1 else ("global critic" if gcf else "critic per agent")
                r, got_side = epoch_ab(N, A, T, L, args.obstructions, gcf, args.warmup, args.repeats, args.seed)
                assert got_side == side, (got_side, side)
                for name in ("team", "per-agent"):
                    say(f"epoch slice {sl} envs {N} side {side} agents {A} {mode:16s} obstruction_count {args.obstructions} {name:9s} | ms per epoch "
                        f"{mmm(r[name])} | {N * T * A / statistics.median(r[name]) / 1e3:8.2f} M agent steps/s (median)")
                v = verdict(r["team"], r["per-agent"])
                say(f"epoch slice {sl} envs {N} side {side} agents {A} {mode:16s} obstruction_count {args.obstructions} {v}"
                    f"{'  SLOWER' if 'NOT faster' in v else ''}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
