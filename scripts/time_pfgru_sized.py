"""The PFGRU location predictor at hidden widths other than 24 (csrc/rs_pfgru_sized.hip):
  1. one predictor step over --envs envs x --agents owners (config 4's shape: 4096 x 4), carried particle sets: the sized kernels
     against PredictorBank(impl="torch") for each --widths entry, and the sized kernels forced at 24 units against K11; A and B
     alternated rep by rep in one process, HIP events, with the algorithmic work 2 (H + 3) 2H + (H + 3) multiply-adds per particle-step;
  2. the no-grad pass (rs_pfgru_sized_pass) over --episodes episodes of --steps-per-episode steps at 64 units;
  3. RAD-A2C iterations at rec 64 (default policy widths, --iter-envs envs): the sized PFGRU path, the same with the PFGRU training pass
     on library ops (use_k13 = False) and the library-op path, alternated, run 0 (graph capture, warm-up) not reported; the sized path
     also reports the training pass on its own (rs_pfgru_sized_train, HIP events); --iteration-rec 64,16 runs this leg alone at those widths;
  4. a short RAD-TEAM iteration (collect + update, --iter-envs envs, 2 agents) with a 64-unit predictor, against 24 units (K11).
One JSON object per line on stdout.  Kernel times in a run of their own: rocprofv3 --kernel-trace --stats -- python
scripts/time_pfgru_sized.py --skip-iteration."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

PEAK_FLOPS = 157.3e12          # MI355X FP32 vector, spec


def _ev():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def ab(fa, fb, reps):
    """A and B alternated; median seconds of each."""
    fa(); fb(); torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, acc in ((fa, ta), (fb, tb)):
            e0, e1 = _ev()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e-3)
    return sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]


def macs(H):
    return 2 * (H + 3) * 2 * H + (H + 3)


def step_pair(H, N, A, reps, b_impl):
    from radiation_ppo_amd.pfgru import PredictorBank
    torch.manual_seed(0)
    a = PredictorBank(N, A, hidden_size=H, seed=1, carry_hidden=True, device="cuda", impl="hip", sized=True)
    b = PredictorBank(N, A, hidden_size=H, seed=1, carry_hidden=True, device="cuda", impl=b_impl, sized=False if b_impl == "hip" else None)
    for i in range(A):
        b.load_state_dict(i, a.state_dict(i))
    a.reset(); b.reset()
    obs = torch.rand(N, A, 11, device="cuda")
    ta, tb = ab(lambda: a.predict(obs), lambda: b.predict(obs), reps)
    work = macs(H) * 40 * N * A
    for name, t in (("rs_pfgru_sized_step", ta), ("rs_pfgru_step (K11)" if b_impl == "hip" else "PredictorBank(impl='torch')", tb)):
        print(json.dumps(dict(what="step", impl=name, hidden=H, envs=N, owners=A, us=round(t * 1e6, 1),
                              tflops=round(2 * work / t / 1e12, 2), of_peak=round(2 * work / t / PEAK_FLOPS, 3))), flush=True)
    print(json.dumps(dict(what="step_ratio", hidden=H, b=b_impl, speedup=round(tb / ta, 2))), flush=True)


def pass_time(H, E, L, reps):
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.pfgru import PFGRUCell, pack_sized_weights
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = pack_sized_weights([PFGRUCell(hidden_size=H).cuda()])
    X = torch.rand(L, E, 11, device="cuda")
    base = torch.randint(0, 2 ** 52, (1, E), dtype=torch.int64, device="cuda")
    episode = torch.ones(E, dtype=torch.int64, device="cuda")
    calls = torch.arange(L, dtype=torch.int64, device="cuda").view(L, 1).expand(L, E).contiguous()
    h = torch.empty(1, E, H // 4, 40, 4, device="cuda"); p = torch.empty(1, E, 40, device="cuda")
    loc = torch.empty(L, E, 2, device="cuda")
    alive = (C.c_int32 * L)(*([E] * L))

    def run():
        _lib.check(lib.rs_pfgru_sized_pass(w.data_ptr(), X.data_ptr(), h.data_ptr(), p.data_ptr(), base.data_ptr(), episode.data_ptr(),
                                           calls.data_ptr(), 0.7, loc.data_ptr(), alive, L, E, H, st))
    t, _ = ab(run, lambda: None, reps)
    print(json.dumps(dict(what="pass", hidden=H, episodes=E, steps=L, ms=round(t * 1e3, 2), us_per_step=round(t / L * 1e6, 1),
                          tflops=round(2 * macs(H) * 40 * E * L / t / 1e12, 2))), flush=True)


def rada2c_iterations(N, T, L, runs, rec=64):
    """Whole RAD-A2C iterations at PFGRU width rec, alternated: every kernel sized ("sized"), the sized kernels with the PFGRU training
    pass on library ops (use_k13 = False: what ran before rs_pfgru_sized_train existed), and library ops throughout.  The sized path also
    reports the training pass on its own (HIP events around rs_pfgru_sized_train) per particle-step."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector

    def make(sized, hip_train):
        torch.manual_seed(0)
        env = RadSearchVec(N, number_agents=1, obstruction_count=1, enforce_grid_boundaries=True, seed=5)
        agents = {0: RNNAgentPPO(id=0, steps_per_epoch=T, steps_per_episode=L, seed=3, actor_critic_args=dict(hidden_sizes_rec=(rec,)))}
        agents[0].agent.sized_pfgru = sized
        agents[0].use_k13 = hip_train
        return RNNCollector(env, agents, T, L), agents[0]
    cols = {"sized": make(True, True), "sized_library_training_pass": make(True, False), "library": make(False, False)}
    for r in range(runs + 1):
        for path, (col, ag) in cols.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            col.collect()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if path == "sized":
                _lib.EVENTS = {}
            col.update()
            torch.cuda.synchronize(); t2 = time.perf_counter()
            extra = {}
            if path == "sized":
                ev, _lib.EVENTS = _lib.EVENTS, None
                ms = sum(a.elapsed_time(b) for a, b in ev.get("rs_pfgru_sized_train", []))
                ps = sum(ag.k13_particle_steps)
                extra = dict(train_pass_calls=len(ev.get("rs_pfgru_sized_train", [])), train_pass_ms=round(ms, 2), particle_steps=ps,
                             ns_per_particle_step=round(1e6 * ms / max(ps, 1), 3))
            if r:
                print(json.dumps(dict(what="rada2c_iteration", rec=rec, path=path, bank=col.bank.impl, use_glue=col.use_glue, run=r, envs=N,
                                      steps_per_epoch=T, collect_s=round(t1 - t0, 3), update_s=round(t2 - t1, 3),
                                      env_steps_per_s=round(T * N / (t2 - t0), 1), **extra)), flush=True)
    del cols
    torch.cuda.empty_cache()


def radteam_iterations(N, T, L, runs):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector

    def make(H):
        torch.manual_seed(0)
        env = RadSearchVec(N, number_agents=2, obstruction_count=1, enforce_grid_boundaries=True, seed=5)
        gc = CNNCritic().cuda()
        agents = {i: CNNAgentPPO(id=i, GlobalCritic=gc, GlobalCriticOptimizer=torch.optim.Adam(gc.parameters(), lr=1e-3), train_pi_iters=4,
                                 train_v_iters=4) for i in range(2)}
        return CNNCollector(env, agents, T, L, global_critic_flag=True, predictor_hidden_size=H)
    cols = {64: make(64), 24: make(24)}
    for r in range(runs + 1):
        for H, col in cols.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            col.collect()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            col.update()
            torch.cuda.synchronize(); t2 = time.perf_counter()
            if r:
                print(json.dumps(dict(what="radteam_iteration", predictor_hidden=H, sized=col.predictor.sized, run=r, envs=N, agents=2,
                                      steps_per_epoch=T, collect_s=round(t1 - t0, 3), update_s=round(t2 - t1, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="16,32,64")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--episodes", type=int, default=16384)
    ap.add_argument("--steps-per-episode", type=int, default=120)
    ap.add_argument("--iter-envs", type=int, default=1024)
    ap.add_argument("--steps-per-epoch", type=int, default=240)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--iteration-rec", default="", help="only the RAD-A2C iterations, at these PFGRU widths (e.g. 64,16)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_pfgru_sized.py measures the MI355X"
    if a.iteration_rec:
        for rec in (int(v) for v in a.iteration_rec.split(",")):
            rada2c_iterations(a.iter_envs, a.steps_per_epoch, a.steps_per_episode, a.runs, rec)
        return
    with torch.no_grad():
        for H in (int(v) for v in a.widths.split(",")):
            step_pair(H, a.envs, a.agents, a.reps, "torch")
        step_pair(24, a.envs, a.agents, a.reps, "hip")
        pass_time(64, a.episodes, a.steps_per_episode, max(2, a.reps // 3))
    if not a.skip_iteration:
        rada2c_iterations(a.iter_envs, a.steps_per_epoch, a.steps_per_episode, a.runs)
        radteam_iterations(a.iter_envs // 4, a.steps_per_epoch // 4, a.steps_per_episode // 4, a.runs)


if __name__ == "__main__":
    main()
