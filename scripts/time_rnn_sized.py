"""The RAD-A2C actor-critic at non-default widths (csrc/rs_rnn_sized.hip) for each --sizes entry hid,pol,val:
  1. each sized kernel alone -- the policy step over --envs envs, the GRU sequence forward / backward over --episodes episodes of
     --steps-per-episode steps, the heads-loss over all of their samples -- HIP events, with FLOP, HBM bytes and roofline fraction;
  2. RAD-A2C iterations (--envs envs, 1 agent, rec 24, --steps-per-episode steps per episode, --steps-per-epoch steps per epoch) on the
     sized path and on the library-op path at the same widths (and on K12 / K14 / K15 at the default widths), --runs of each, alternated:
     collect and update seconds, env steps / s.
One JSON object per line on stdout.  Kernel times in a run of their own: rocprofv3 --kernel-trace --stats -- python
scripts/time_rnn_sized.py --skip-iteration."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

PEAK_FLOPS = 157.3e12          # MI355X FP32 vector, spec
PEAK_BW = 6.29e12              # measured float4 copy (8.0 TB/s spec)


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def report(name, hid, pol, val, items, t, flop, byts):
    floor = max(flop * items / PEAK_FLOPS, byts * items / PEAK_BW)
    print(json.dumps(dict(what="kernel", kernel=name, hid=hid, pol=pol, val=val, items=items, s=round(t, 6),
                          tflops=round(flop * items / t / 1e12, 3), tbps=round(byts * items / t / 1e12, 3), roofline=round(floor / t, 3),
                          bound="memory" if byts * items / PEAK_BW > flop * items / PEAK_FLOPS else "compute")), flush=True)


def kernels(hid, pol, val, N, L, E, reps):
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.rada2c import RNNAgentPPO, pack_sized_gru_weights, pack_sized_policy_weights
    torch.manual_seed(0)
    ag = RNNAgentPPO(id=0, actor_critic_args=dict(hidden=((hid,),), hidden_sizes_pol=((pol,),), hidden_sizes_val=((val,),)))
    ac = ag.agent
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    HT = (hid + 15) // 16 * 16
    P8, V8 = (pol + 7) // 8 * 8, (val + 7) // 8 * 8
    w = pack_sized_policy_weights(ac)
    x, loc, u = torch.randn(N, 11, device="cuda"), torch.rand(N, 2, device="cuda"), torch.rand(N, device="cuda")
    h = torch.rand(N, hid, device="cuda") * 0.4 - 0.2
    v, lp = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    a = torch.empty(N, dtype=torch.int64, device="cuda")

    def step():
        _lib.check(lib.rs_rnn_sized_step(w.data_ptr(), hid, pol, val, x.data_ptr(), 11, loc.data_ptr(), 2, h.data_ptr(), u.data_ptr(), 1,
                                         h.data_ptr(), None, v.data_ptr(), a.data_ptr(), lp.data_ptr(), None, 1, None, N, st), "step")
    heads_mac = hid * pol + pol * 8 + hid * val + val
    report("rs_rnn_sized_step", hid, pol, val, N, timed(step, reps), 2 * (13 * 3 * hid + hid * 3 * hid + heads_mac),
           4 * (11 + 2 + 1 + 2 * hid + 3) + 8)
    g = ac.pi.logits_net.v_net.seq_model
    gi = torch.randn(L, E, 3 * hid, device="cuda")
    h0 = torch.rand(E, hid, device="cuda") * 0.4 - 0.2
    wg = pack_sized_gru_weights(g.weight_hh_l0.detach(), g.bias_hh_l0.detach())
    hs = torch.empty(L, E, hid, device="cuda")
    gates = torch.empty(L, E, lib.rs_gru_sized_gate_floats(hid), device="cuda")
    dhs = torch.randn(L, E, hid, device="cuda")
    dgi, dgh = torch.empty(L, E, 3 * hid, device="cuda"), torch.empty(L, E, 3 * hid, device="cuda")
    fwd = lambda: _lib.check(lib.rs_gru_sized_forward(gi.data_ptr(), h0.data_ptr(), wg.data_ptr(), hs.data_ptr(), gates.data_ptr(), hid, L, E, st), "fwd")
    bwd = lambda: _lib.check(lib.rs_gru_sized_backward(dhs.data_ptr(), hs.data_ptr(), gates.data_ptr(), h0.data_ptr(), wg.data_ptr(),
                                                       dgi.data_ptr(), dgh.data_ptr(), hid, L, E, st), "bwd")
    report("rs_gru_sized_forward", hid, pol, val, L * E, timed(fwd, reps), 2 * 3 * hid * hid, 4 * (3 * hid + hid + 4 * HT))
    report("rs_gru_sized_backward", hid, pol, val, L * E, timed(bwd, reps), 2 * 3 * hid * hid, 4 * (2 * hid + 4 * HT + 6 * hid))
    S = L * E
    hsf = hs.view(S, hid)
    act = torch.randint(0, 8, (S,), device="cuda")
    adv, ret, lpo, wt = torch.randn(S, device="cuda"), torch.randn(S, device="cuda"), torch.randn(S, device="cuda") * 0.1 - 2.0, torch.rand(S, device="cuda")
    dh2, dfac, tfac = torch.empty(S, hid, device="cuda"), torch.empty(S, P8 + V8 + 16, device="cuda"), torch.empty(S, P8 + V8, device="cuda")
    stats = torch.empty((S + 63) // 64, 8, device="cuda")
    heads = lambda: _lib.check(lib.rs_a2c_sized_heads_loss(w.data_ptr(), hid, pol, val, hsf.data_ptr(), act.data_ptr(), adv.data_ptr(),
                                                           ret.data_ptr(), lpo.data_ptr(), wt.data_ptr(), dh2.data_ptr(), dfac.data_ptr(),
                                                           tfac.data_ptr(), stats.data_ptr(), S, 0.2, 0.01, st), "heads")
    report("rs_a2c_sized_heads_loss", hid, pol, val, S, timed(heads, reps), 2 * (2 * heads_mac + 8 * pol + pol * hid + val * hid),
           4 * (hid + 5) + 8 + 4 * (hid + 2 * (P8 + V8) + 16))


def make(hid, pol, val, N, T, L, sized):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector
    torch.manual_seed(0)
    env = RadSearchVec(N, number_agents=1, obstruction_count=0, enforce_grid_boundaries=True, seed=289714752)
    args = dict(hidden=((hid,),), hidden_sizes_pol=((pol,),), hidden_sizes_val=((val,),))
    agents = {0: RNNAgentPPO(id=0, steps_per_epoch=T, steps_per_episode=L, actor_critic_args=args)}
    if not sized:
        agents[0].agent.sized_policy = False                        # the library-op composition at the same widths
    col = RNNCollector(env, agents, T, L)
    return col, agents


def iterations(sizes, N, T, L, runs):
    """One widths entry at a time (each path's update keeps tens of GB of scratch): its paths alternated, run 0 (graph capture and
    library warm-up) not reported."""
    for hid, pol, val in sizes:
        default = (hid, pol, val) == (24, 32, 32)
        cols = {path: make(hid, pol, val, N, T, L, path != "library") for path in (("default",) if default else ("sized", "library"))}
        for r in range(runs + 1):
            for path, (col, agents) in cols.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                col.collect()
                torch.cuda.synchronize(); t1 = time.perf_counter()
                res = col.update()
                torch.cuda.synchronize(); t2 = time.perf_counter()
                if r == 0:
                    continue
                print(json.dumps(dict(what="iteration", run=r, hid=hid, pol=pol, val=val, path=path, use_sized=col.use_sized,
                                      use_glue=col.use_glue, envs=N, steps_per_epoch=T, steps_per_episode=L, collect_s=round(t1 - t0, 3),
                                      update_s=round(t2 - t1, 3), pi_iters=res[0].stop_iteration,
                                      env_steps_per_s=round(T * N / (t2 - t0), 1))), flush=True)
        del cols, col, agents
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="24,32,32;32,64,64;64,64,64")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=16384, help="episodes of the GRU / heads-loss kernel timings")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps-per-epoch", type=int, default=480)
    ap.add_argument("--steps-per-episode", type=int, default=120)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_rnn_sized.py measures the MI355X"
    sizes = [tuple(int(v) for v in s.split(",")) for s in a.sizes.split(";")]
    if not a.skip_kernels:
        for hid, pol, val in sizes:
            kernels(hid, pol, val, a.envs, a.steps_per_episode, a.episodes, a.reps)
    if not a.skip_iteration:
        iterations(sizes, a.envs, a.steps_per_epoch, a.steps_per_episode, a.runs)


if __name__ == "__main__":
    main()
