"""The walls-off RAD-TEAM CNN at 147 x 147 (maps without enforced walls, 120-step episodes):
  1. the tiled HIP trunk (maps.SizedConvTrunk: rs_cnn_sized_forward / _infer / _backward) against the library path it replaces
     (dense stack from maps.actor_stack_from + the nn.Sequential's native convolutions, MIOpen off, autograd) on the same 4096 images,
     actor and critic: forward (inference and training) and backward, HIP events, with the HIP trunk's FLOP, HBM bytes and roofline
     fraction;
  2. one RAD-TEAM iteration shaped like the authors' walls-off run (1 agent, 0 obstacles, 120-step episodes, 480 steps per epoch) at
     --envs envs: collect and update seconds, env steps / s.
One JSON object per line on stdout."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

PEAK_FLOPS = 157.3e12          # MI355X FP32 vector, spec
PEAK_BW = 6.29e12              # measured float4 copy (8.0 TB/s spec)


def trunk_cost(M: int, cin: int, train: bool, backward: bool):
    """(FLOP, HBM bytes) per image of the tiled trunk: conv1 over the 2P x 2P pixels the pool reads, conv2 over P x P; bytes = the 4
    map planes in and a2 out (training adds p1, amax, mask); backward reads maps, da2, p1, amax, mask and runs dW2, dP1 and dW1 (one
    pixel per pooled cell)."""
    P, dense = M // 2, 4 * 9
    maps_b, a2_b, saved_b = 4 * M * M * 4, 16 * P * P * 4, P * P * (32 + 8 + 2)
    if backward:
        return 2 * P * P * (16 * 72 + 16 * 72 + 8 * dense), maps_b + a2_b + saved_b
    return 2 * (4 * P * P) * 8 * dense + 2 * P * P * 16 * 72, maps_b + a2_b + (saved_b if train else 0)


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def trunks(M: int, S: int, reps: int):
    from radiation_ppo_amd.maps import CNNActor, CNNCritic, SizedConvTrunk, actor_stack_from
    torch.manual_seed(0)
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    maps = (torch.rand(S, 4, M, M, device="cuda", generator=g) * (torch.rand(S, 4, M, M, device="cuda", generator=g) < 0.1)).contiguous()
    cells = torch.randint(0, M * M, (S, 1), device="cuda", generator=g)
    pcells = torch.randint(0, M * M, (S, 1), device="cuda", generator=g)
    for kind, seq in (("actor", CNNActor(map_dim=(M, M)).cuda().actor), ("critic", CNNCritic(map_dim=(M, M)).cuda().critic)):
        agent, cin = (0, 6) if kind == "actor" else (-1, 4)
        conv = [seq[0].weight, seq[0].bias, seq[3].weight, seq[3].bias]
        c, pc = (cells, pcells) if agent >= 0 else (None, None)
        da2 = torch.randn(S, 16 * (M // 2) ** 2, device="cuda")
        dense_in = lambda: actor_stack_from(maps, cells, pcells, 0) if agent >= 0 else maps
        lib_trunk = lambda x: seq[5](seq[4](seq[3](seq[2](seq[1](seq[0](x))))))
        saved = {}

        def hip_fwd(train):
            with torch.set_grad_enabled(train):
                saved["a2"] = SizedConvTrunk.apply(maps, c, pc, agent, *conv, train)

        def lib_fwd(train):
            with torch.set_grad_enabled(train), torch.backends.cudnn.flags(enabled=False):
                saved["a2"] = lib_trunk(dense_in())

        def bwd():
            with torch.backends.cudnn.flags(enabled=False):
                torch.autograd.backward(saved["a2"], da2, retain_graph=True, inputs=conv)

        for path, fwd in (("hip", hip_fwd), ("library", lib_fwd)):
            res = {}
            res["fwd_infer_s"] = timed(lambda: fwd(False), reps)
            res["fwd_train_s"] = timed(lambda: fwd(True), reps)
            fwd(True)
            res["bwd_s"] = timed(bwd, reps)
            saved.clear(); torch.cuda.empty_cache()
            out = dict(what="trunk", path=path, net=kind, M=M, images=S, **{k: round(v, 6) for k, v in res.items()})
            if path == "hip":
                for key, train, back in (("fwd_infer", False, False), ("fwd_train", True, False), ("bwd", True, True)):
                    fl, by = trunk_cost(M, cin, train, back)
                    t = res[key + "_s"]
                    out[key + "_tflops"] = round(fl * S / t / 1e12, 2)
                    out[key + "_tbps"] = round(by * S / t / 1e12, 2)
                    floor = max(fl * S / PEAK_FLOPS, by * S / PEAK_BW)
                    out[key + "_roofline"] = round(floor / t, 3)
                    out[key + "_bound"] = "memory" if by * S / PEAK_BW > fl * S / PEAK_FLOPS else "compute"
            print(json.dumps(out), flush=True)


def iteration(N: int, T: int, L: int, iters: int):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import heat_map_geometry
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    torch.manual_seed(0)
    env = RadSearchVec(N, number_agents=1, obstruction_count=0, enforce_grid_boundaries=False, seed=289714752)
    dims = heat_map_geometry(env, L, False)[2]
    agents = {0: CNNAgentPPO(id=0, map_dim=dims, steps_per_epoch=T, steps_per_episode=L)}
    col = CNNCollector(env, agents, T, L, global_critic_flag=True)
    for it in range(iters):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        col.collect()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        res = col.update()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        print(json.dumps(dict(what="iteration", iteration=it, envs=N, maps=list(dims), steps_per_epoch=T, steps_per_episode=L,
                              chunk=agents[0].chunk, use_heads=col.use_heads, collect_s=round(t1 - t0, 3), update_s=round(t2 - t1, 3),
                              pi_iters=res[0].stop_iteration, env_steps_per_s=round(T * N / (t2 - t0), 1),
                              peak_gb=round(torch.cuda.max_memory_allocated() / 1e9, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=147)
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--steps-per-epoch", type=int, default=480)
    ap.add_argument("--steps-per-episode", type=int, default=120)
    ap.add_argument("--iterations", type=int, default=2, help="the first one includes graph capture and library warm-up")
    ap.add_argument("--skip-trunk", action="store_true")
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_cnn_sized.py measures the MI355X"
    if not a.skip_trunk:
        trunks(a.side, a.images, a.reps)
    if not a.skip_iteration:
        iteration(a.envs, a.steps_per_epoch, a.steps_per_episode, a.iterations)


if __name__ == "__main__":
    main()
