"""The occupancy-aware training passes of the tiled CNN trunk (rs_cnn_sized_occupancy, rs_cnn_sized_forward_occ / _backward_occ:
SizedConvTrunk with occ) against the dense passes (rs_cnn_sized_forward / _backward: occ = None) at 147 x 147, in one session.  Plain
text on stdout and in profiles/cnn_sized_occ_timing.txt (--append: behind what is there, so that the parts can run as separate
processes, each under its own time limit).  --part selects:

kernels  the training forward and the backward alone (HIP kernels only: the trunk's autograd function, no head), actor and critic,
         (a) on a run's own maps -- --envs envs, one collected epoch of --steps lock-steps, the chunk of the update in the middle of the
         epoch, of the size maps.sized_trunk_sample_bytes gives -- and (b) on as many random maps of which 10 % of the elements are
         non-zero (tests/test_cnn_sized_trunk_gpu.py::_random_inputs' density), where no unit is empty.  Wall ms per call over --rounds
         calls between two device synchronisations.  Also the occupancy pass over the epoch and the share of units found empty.
update   (c) CNNCollector.update() on one collected epoch with use_occupancy on against off: the same collector, the forms alternated.
         target_kl is lifted so that every update runs all of its --pi-iters + --v-iters iterations whatever the parameters have become
         (the repeats update the same networks again and again); 40 + 40 is the training default.

--warmup untimed repeats, then --repeats timed ones of each form, alternated: min median max; the verdict is the new form's slowest
repeat against the dense form's fastest, and for (b) the dense form's own spread (max / min - 1) is the allowance."""
import argparse
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def mmm(v):
    return f"{min(v):9.3f} {statistics.median(v):9.3f} {max(v):9.3f}"


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


def verdict(occ, dense, allowance=False):
    spread = max(dense) / min(dense) - 1
    s = (f"occ slowest {max(occ):.3f} ms, dense fastest {min(dense):.3f} ms (dense spread {100 * spread:.2f} %) -> "
         f"median / median = {statistics.median(dense) / statistics.median(occ):.2f} x")
    if max(occ) < min(dense):
        return s + "; faster"
    if allowance and max(occ) <= min(dense) * (1 + spread):
        return s + "; within the dense form's spread"
    return s + "; NOT faster  SLOWER"


def collector(N, A, T, L, obst, seed, pi_iters, v_iters):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic, heat_map_geometry
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    torch.manual_seed(seed)
    env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=False, seed=seed)
    kw = dict(map_dim=tuple(heat_map_geometry(env, L, False)[2]), steps_per_epoch=T, steps_per_episode=L, train_pi_iters=pi_iters,
              train_v_iters=v_iters)
    gcr = CNNCritic(map_dim=kw["map_dim"]).cuda()
    agents = {i: CNNAgentPPO(id=i, GlobalCritic=gcr, GlobalCriticOptimizer=torch.optim.Adam(gcr.parameters(), lr=1e-3), **kw) for i in range(A)}
    col = CNNCollector(env, agents, T, L, global_critic_flag=True)
    col.collect()
    torch.cuda.synchronize()
    assert col.env.error_flags() == 0
    return col, agents


def trunk_forms(seq, maps, cells, pcells, agent, flags):
    """{(pass, form): fn} of the trunk's training forward and backward with and without the flags"""
    from radiation_ppo_amd.maps import SizedConvTrunk
    conv = [seq[0].weight, seq[0].bias, seq[3].weight, seq[3].bias]
    P = maps.shape[-1] // 2
    da2 = torch.randn(maps.shape[0], 16 * P * P, device="cuda")
    out, saved = {}, {}
    for form, occ in (("occ", flags), ("dense", None)):
        def fwd(form=form, occ=occ):
            saved[form] = SizedConvTrunk.apply(maps, cells, pcells, agent, *conv, True, occ)

        def bwd(form=form):
            torch.autograd.backward(saved[form], da2, retain_graph=True, inputs=conv)
        out["forward", form], out["backward", form] = fwd, bwd
    return out, saved


def part_kernels(args, say):
    from radiation_ppo_amd.maps import CNNActor, CNNCritic, sized_occupancy
    N, T, L = args.envs, args.steps, args.episode_steps
    col, agents = collector(N, 1, T, L, args.obstructions, args.seed, 1, 1)
    M = col.maps.map_dimensions[0]
    chunk = agents[0].chunk
    shared = col.shared.view(T * N, 4, M, M)
    r = ab({"occupancy": lambda: sized_occupancy(shared)}, 1, args.warmup, args.repeats)["occupancy"]
    flags_all = sized_occupancy(shared)
    say(f"occupancy pass   envs {N} side {M} images {T * N} ({shared.numel() * 4 / 1e9:.1f} GB) | ms per call {mmm(r)} | "
        f"{shared.numel() * 4 / statistics.median(r) / 1e9:.2f} TB/s (median) | flags zero: {100 * float((flags_all == 0).float().mean()):.2f} % of {flags_all.numel()} units")
    lo = max(0, (T * N - chunk) // 2)
    own = (shared[lo:lo + chunk], col.cells.view(T * N, 1)[lo:lo + chunk], col.pcells.view(T * N, 1)[lo:lo + chunk])
    S = own[0].shape[0]
    g = torch.Generator(device="cuda"); g.manual_seed(args.seed)
    rnd = (torch.rand(S, 4, M, M, device="cuda", generator=g) * (torch.rand(S, 4, M, M, device="cuda", generator=g) < 0.1)).contiguous()
    random = (rnd, torch.randint(0, M * M, (S, 1), device="cuda", generator=g), torch.randint(0, M * M, (S, 1), device="cuda", generator=g))
    torch.manual_seed(args.seed)
    nets = (("actor", CNNActor(map_dim=(M, M)).cuda().actor, 0), ("critic", CNNCritic(map_dim=(M, M)).cuda().critic, -1))
    for label, (maps, cells, pcells), allowance in (("(a) own maps", own, False), ("(b) random 10 %", random, True)):
        flags = sized_occupancy(maps)
        say(f"{label:16s} envs {N} side {M} images {S} (samples {lo}..{lo + S} of the epoch) | flags zero: {100 * float((flags == 0).float().mean()):.2f} % of units")
        for kind, seq, agent in nets:
            forms, saved = trunk_forms(seq, maps, cells if agent >= 0 else None, pcells if agent >= 0 else None, agent, flags)
            for what in ("forward", "backward"):
                if what == "backward":
                    forms["forward", "occ"](); forms["forward", "dense"]()
                res = ab({f: forms[what, f] for f in ("occ", "dense")}, args.rounds, args.warmup, args.repeats)
                for f in ("occ", "dense"):
                    say(f"{label:16s} {kind:6s} {what:8s} {f:5s} | ms per call {mmm(res[f])}")
                say(f"{label:16s} {kind:6s} {what:8s} {verdict(res['occ'], res['dense'], allowance)}")
            saved.clear()
            gc.collect()
            torch.cuda.empty_cache()


def part_update(args, say):
    N, T, L = args.envs, args.steps, args.episode_steps
    for A in args.agents:
        col, agents = collector(N, A, T, L, args.obstructions, args.seed, args.pi_iters, args.v_iters)
        for ag in agents.values():
            ag.target_kl = 1e9
        M = col.maps.map_dimensions[0]
        res = {"occ": [], "dense": []}
        for i in range(args.warmup + args.repeats):
            for form in ("occ", "dense"):
                col.use_occupancy = form == "occ"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = col.update()
                torch.cuda.synchronize()
                assert all(r.stop_iteration == args.pi_iters for r in out.values())
                if i >= args.warmup:
                    res[form].append((time.perf_counter() - t0) * 1e3)
        mode = "one critic" if A == 1 else "global critic"
        for f in ("occ", "dense"):
            say(f"(c) update       envs {N} side {M} T {T} agents {A} {mode:13s} iters {args.pi_iters}+{args.v_iters} chunk {agents[0].chunk} {f:5s} | "
                f"ms per update {mmm(res[f])}")
        say(f"(c) update       envs {N} side {M} T {T} agents {A} {mode:13s} {verdict(res['occ'], res['dense'])}")
        del col, agents
        gc.collect()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "update"], required=True)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--steps", type=int, default=120, help="lock-steps of the collected epoch")
    ap.add_argument("--episode-steps", type=int, default=120, help="the maps' side is 27 + this")
    ap.add_argument("--obstructions", type=int, default=3)
    ap.add_argument("--agents", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--pi-iters", type=int, default=40)
    ap.add_argument("--v-iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_sized_occ_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_cnn_sized_occ.py measures the MI355X"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; part {args.part}; {args.warmup} warm-up + {args.repeats} timed repeats of "
        f"each form, alternated, seed {args.seed}; min median max; obstruction_count {args.obstructions}")
    (part_kernels if args.part == "kernels" else part_update)(args, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
