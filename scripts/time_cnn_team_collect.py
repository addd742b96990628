"""A RAD-TEAM (CNN) team's training round in three launches (rs_cnn_team_trunk_infer, the critic trunk(s), rs_cnn_team_step_head) against
the per-agent round (per agent rs_cnn_trunk_infer + BLAS Linear(2704, 32) + rs_cnn_head, then the same per critic), at the workload's
size: --envs envs, 27 x 27 maps, A = 1, 2, 4, 8 agents, a global critic and one critic per agent.  Plain text on stdout and in
profiles/cnn_team_collect_timing.txt (--append: behind what is there, so that the parts can run as separate processes, each under its
own time limit).  --part selects:

kernels  the launches alone, --rounds of them back to back on one stream between two device synchronisations (wall span over rounds,
         host issue time included): the head launch of a step round against A x (GEMM + rs_cnn_head) + C x (GEMM + rs_cnn_head), of a
         bootstrap round (mask: one env in --episode-steps) against C x (GEMM + masked rs_cnn_head), and the critic team trunk against C
         launches of rs_cnn_trunk_infer(agent = -1).
epochs   one collector epoch (CNNCollector.collect: --steps lock-steps through the captured graph, episodes of --episode-steps steps, GAE
         included), team_round on against off -- off is the per-agent round, the code before the team round.  Two collectors in one
         process, their epochs alternated; obstacle-free and with --obstructions obstructions.  The epoch's stored maps are
         steps x envs x 4 x 729 x 4 bytes per collector (11.5 GB at 240 x 4096).

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

FLAT = 2704


def verdict(team, per_agent):
    return (f"team slowest {max(team):.4f} ms, per-agent fastest {min(per_agent):.4f} ms -> {'faster' if max(team) < min(per_agent) else 'NOT faster'}; "
            f"median / median = {statistics.median(per_agent) / statistics.median(team):.2f} x")


def ab(forms, rounds, warmup, repeats):
    res = {name: [] for name in forms}
    for i in range(warmup + repeats):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(rounds):
                fn()
            torch.cuda.synchronize()
            if i >= warmup:
                res[name].append((time.perf_counter() - t0) / rounds * 1e3)
    return res


def kernels_ab(N, A, nc, boot_every, rounds, warmup, repeats):
    """{(what, form): [wall ms per call]} for the step heads, the bootstrap heads and the critic trunks of A agents and nc critics"""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import CNNActor, CNNCritic, cnn_head_params, cnn_trunk_prepare
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(N + 10 * A + nc)
    actors = [CNNActor().to(dev).actor for _ in range(A)]
    critics = [CNNCritic().to(dev).critic for _ in range(nc)]
    p = lambda t: t.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    hpa, hpc = (_lib.RsCnnHeadParams * A)(*map(cnn_head_params, actors)), (_lib.RsCnnHeadParams * nc)(*map(cnn_head_params, critics))
    sparse = lambda *s: torch.rand(*s, device=dev) * (torch.rand(*s, device=dev) < 0.3)            # a trunk's output: non-negative, sparse
    a2a, a2c, u = sparse(A, N, FLAT), sparse(nc, N, FLAT), torch.rand(N, A, device=dev)
    maps = torch.rand(N, 4, 729, device=dev) * (torch.rand(N, 4, 729, device=dev) < 0.1)
    boot = (torch.arange(N, device=dev) % boot_every == 0).to(torch.uint8)
    act, f, act8 = torch.zeros(A, N, dtype=torch.int64, device=dev), torch.zeros(A, 3, N, device=dev), torch.zeros(N, A, dtype=torch.int8, device=dev)
    wt_c = torch.empty(nc, lib.rs_cnn_trunk_scratch_floats(4), device=dev)
    for c, m in enumerate(critics):
        cnn_trunk_prepare(m, 4, wt_c[c], st)
    copies = A if nc == 1 else 1

    def value(c, slot, mask):
        m = critics[c]
        y1 = torch.nn.functional.linear(a2c[c], m[6].weight, m[6].bias)
        _lib.check(lib.rs_cnn_head(p(y1), p(m[8].weight), p(m[8].bias), p(m[10].weight), p(m[10].bias), 1, None, 1, None, None, None, 1,
                                   p(f[c, slot]), copies, 3 * N, mask, N, st), "rs_cnn_head")

    def step_team():
        _lib.check(lib.rs_cnn_team_step_head(hpa, A, hpc, nc, p(a2a), p(a2c), p(u), p(act), p(f), p(act8), None, None, N, st), "step round")

    def step_per_agent():
        for a, m in enumerate(actors):
            y1 = torch.nn.functional.linear(a2a[a], m[6].weight, m[6].bias)
            _lib.check(lib.rs_cnn_head(p(y1), p(m[8].weight), p(m[8].bias), p(m[10].weight), p(m[10].bias), 8, p(u) + 4 * a, A, p(act[a]),
                                       p(f[a, 0]), p(act8) + a, A, None, 1, 0, None, N, st), "rs_cnn_head")
        for c in range(nc):
            value(c, 1, None)

    def boot_team():
        _lib.check(lib.rs_cnn_team_step_head(None, A, hpc, nc, None, p(a2c), None, None, p(f), None, p(boot), None, N, st), "bootstrap round")

    def boot_per_agent():
        for c in range(nc):
            value(c, 2, p(boot))

    def trunk_team():
        _lib.check(lib.rs_cnn_team_critic_trunk_infer(p(maps), nc, N, p(wt_c), p(a2c), st), "rs_cnn_team_critic_trunk_infer")

    def trunk_per_agent():
        for c in range(nc):
            _lib.check(lib.rs_cnn_trunk_infer(p(maps), None, None, 0, -1, N, p(wt_c[c]), p(a2c[c]), st), "rs_cnn_trunk_infer")
    with torch.no_grad():
        out = {}
        for what, team, per in (("step heads", step_team, step_per_agent), ("bootstrap heads", boot_team, boot_per_agent),
                                ("critic trunks", trunk_team, trunk_per_agent)):
            if what == "critic trunks" and nc == 1:
                continue                                        # a global critic's trunk is rs_cnn_trunk_infer in both forms
            for name, v in ab({"team": team, "per-agent": per}, rounds, warmup, repeats).items():
                out[what, name] = v
    return out


def epoch_ab(N, A, T, L, obst, global_critic, warmup, repeats, seed):
    """{form: [wall ms per collector epoch]}, the two forms' epochs alternated"""
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    cols = {}
    for name, on in (("team", True), ("per-agent", False)):
        torch.manual_seed(seed)
        env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=seed)
        gc = CNNCritic().cuda() if global_critic else None
        agents = {i: CNNAgentPPO(id=i, GlobalCritic=gc, GlobalCriticOptimizer=torch.optim.Adam(gc.parameters(), lr=1e-3) if gc is not None else None)
                  for i in range(A)}
        col = CNNCollector(env, agents, T, L, global_critic_flag=global_critic)
        col.team_round = on
        assert col.use_heads and col.use_team_round == on
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
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "epochs"], required=True)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--episode-steps", type=int, default=120)
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_team_collect_timing.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    N, T, L = args.envs, args.steps, args.episode_steps
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; part {args.part}, agents {args.agents}; {args.warmup} warm-up + "
        f"{args.repeats} timed repeats of each form, alternated, seed {args.seed}; min median max")
    if args.part == "kernels":
        say(f"# the launches alone at {N} envs: wall ms per call over {args.rounds} calls issued back to back; bootstrap mask: one env in {L}")
        for A in args.agents:
            for nc in sorted({1, A}):
                mode = "global critic" if nc == 1 and A > 1 else ("one critic" if A == 1 else "critic per agent")
                r = kernels_ab(N, A, nc, L, args.rounds, args.warmup, args.repeats)
                for what in ("step heads", "bootstrap heads", "critic trunks"):
                    if (what, "team") not in r:
                        continue
                    for name in ("team", "per-agent"):
                        say(f"{what:15s} envs {N} agents {A} {mode:16s} {name:9s} | ms per call {mmm(r[what, name])}")
                    say(f"{what:15s} envs {N} agents {A} {mode:16s} {verdict(r[what, 'team'], r[what, 'per-agent'])}")
    else:
        say(f"# one collector epoch (CNNCollector.collect, captured lock-step): {N} envs, T = {T} lock-steps, episodes of {L} steps; wall ms "
            f"per epoch; stored maps {T * N * 4 * 729 * 4 / 1e9:.1f} GB per collector")
        for A in args.agents:
            for gc in ((True,) if A == 1 else (True, False)):
                mode = "one critic" if A == 1 else ("global critic" if gc else "critic per agent")
                for obst in (0, args.obstructions):
                    r = epoch_ab(N, A, T, L, obst, gc, args.warmup, args.repeats, args.seed)
                    for name in ("team", "per-agent"):
                        say(f"epoch envs {N} agents {A} {mode:16s} obstruction_count {obst} {name:9s} | ms per epoch {mmm(r[name])} | "
                            f"{N * T * A / statistics.median(r[name]) / 1e3:8.2f} M agent steps/s (median)")
                    say(f"epoch envs {N} agents {A} {mode:16s} obstruction_count {obst} {verdict(r['team'], r['per-agent'])}")
    with open(args.out, "a" if args.append else "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
