"""rs_pfgru_sized (csrc/rs_pfgru_sized.hip): the PFGRU location predictor at hidden widths 8, 16, .., 64 through PredictorBank,
the RAD-A2C collector / update / evaluation and the RAD-TEAM collector.  Tolerances and the near-tie rule are test_pfgru_gpu.py's:
a row that differs beyond rtol 1e-4 / atol 2e-5 must have a resampling uniform within 2e-6 of a CDF value (the torch composition
reports the distance), and there may be no more such rows than near-ties."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_ppo_gpu import SEED, _replay_check  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL, TIE = 1e-4, 2e-5, 2e-6
SIZED = (8, 16, 32, 40, 48, 56, 64)


def _banks(N, A, carry, H, seed=7, base=96, sized=None, ref_impl="torch"):
    from radiation_ppo_amd.pfgru import PredictorBank
    torch.manual_seed(3 + H)
    hip = PredictorBank(N, A, hidden_size=H, seed=seed, env_id_base=base, carry_hidden=carry, device="cuda", impl="hip", sized=sized)
    ref = PredictorBank(N, A, hidden_size=H, seed=seed, env_id_base=base, carry_hidden=carry, device="cuda", impl=ref_impl,
                        sized=False if ref_impl == "hip" else None)
    for a in range(A):
        with torch.no_grad():
            for p in hip.cells[a].parameters():
                p.mul_(2.0)                                            # livelier gates than the default initialisation
        ref.load_state_dict(a, hip.state_dict(a))
    return hip, ref


def _bad_rows(x, y):
    bad = ~torch.isclose(x, y, rtol=RTOL, atol=ATOL)
    return bad.reshape(bad.shape[0], bad.shape[1], -1).any(dim=2)


def _obs(N, A, g):
    obs = torch.rand(N, A, 11, device="cuda", generator=g)
    obs[..., 0] = torch.randint(0, 4000, (N, A), device="cuda", generator=g).float() / 100.0 - 10.0
    return obs


@pytest.mark.parametrize("H", SIZED)
def test_sized_reset_is_bit_exact_and_masked(H):
    hip, ref = _banks(200, 3, True, H)
    assert hip.sized and hip._hq.shape == (3, 200, H // 4, 40, 4)
    hip.reset(); ref.reset()
    assert torch.equal(hip.h, ref.h) and torch.equal(hip.p, ref.p)
    mask = torch.rand(200, device="cuda") < 0.3
    before = hip.h.clone()
    hip.reset(mask=mask); ref.reset(mask=mask)
    assert torch.equal(hip.h, ref.h) and torch.equal(hip.p, ref.p)
    assert torch.equal(hip.h[:, ~mask], before[:, ~mask]) and not torch.equal(hip.h[:, mask], before[:, mask])


def _compare(hip, ref, carry, N, A, steps=5, seed=11):
    """Steps of both banks (masked rounds on odd steps), the near-tie rule; returns (moved rows, near-ties)."""
    ref.record_margin = True
    g = torch.Generator(device="cuda").manual_seed(seed)
    moved = ties = 0
    for t in range(steps):
        obs = _obs(N, A, g)
        mask = None if t % 2 == 0 else (torch.rand(N, device="cuda", generator=g) < 0.6)
        ph, pr = hip.predict(obs, mask), ref.predict(obs, mask)
        assert torch.isfinite(ph).all() and float(ph.min()) >= 0.0
        counted = torch.ones(N, dtype=torch.bool, device="cuda") if mask is None else mask
        near_tie = ref.last_margin < TIE if ref.impl == "torch" else torch.ones(A, N, dtype=torch.bool, device="cuda")
        bad = _bad_rows(ph.permute(1, 0, 2), pr.permute(1, 0, 2)) & counted.view(1, N)
        if carry:
            bad |= (_bad_rows(hip.h, ref.h) | _bad_rows(hip.p.unsqueeze(-1), ref.p.unsqueeze(-1))) & counted.view(1, N)
            ref.h, ref.p = hip.h.clone(), hip.p.clone()
        else:
            assert torch.equal(hip.h, ref.h)
        assert not bool((bad & ~near_tie).any()), (t, int((bad & ~near_tie).sum()))
        moved += int(bad.sum()); ties += int((near_tie & counted.view(1, N)).sum())
        assert torch.equal(hip.calls, ref.calls)
        if t == 2:
            cut = torch.rand(N, device="cuda", generator=g) < 0.25
            hip.reset(mask=cut); ref.reset(mask=cut)
    return moved, ties


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("H", SIZED)
def test_sized_step_matches_torch_composition(H, carry):
    N, A = 384, 3
    hip, ref = _banks(N, A, carry, H)
    hip.reset(); ref.reset()
    moved, ties = _compare(hip, ref, carry, N, A)
    print(f"H {H}: {moved} rows with a moved index of {ties} near-ties")
    assert moved <= ties


def test_sized_kernels_at_24_units_agree_with_k11():
    """The sized kernels forced at 24 units against K11: the same draws; rows may differ only where the torch composition finds a
    near-tie (both kernels are held to it with the same rule), so the count of differing rows is bounded by the near-ties."""
    N, A = 512, 2
    sized, k11 = _banks(N, A, True, 24, sized=True, ref_impl="hip")
    _, tor = _banks(N, A, True, 24)
    tor.record_margin = True
    for a in range(A):
        tor.load_state_dict(a, sized.state_dict(a))
    assert sized.sized and not k11.sized
    sized.reset(); k11.reset(); tor.reset()
    assert torch.equal(sized.h, k11.h) and torch.equal(sized.p, k11.p)
    g = torch.Generator(device="cuda").manual_seed(5)
    moved = ties = 0
    for t in range(5):
        obs = _obs(N, A, g)
        tor.h, tor.p = k11.h.clone(), k11.p.clone()                   # the three banks step from the same particle sets
        ps, pk = sized.predict(obs), k11.predict(obs)
        tor.predict(obs)
        near_tie = tor.last_margin < TIE
        bad = _bad_rows(ps.permute(1, 0, 2), pk.permute(1, 0, 2)) | _bad_rows(sized.h, k11.h) | _bad_rows(sized.p.unsqueeze(-1), k11.p.unsqueeze(-1))
        assert not bool((bad & ~near_tie).any()), t
        moved += int(bad.sum()); ties += int(near_tie.sum())
        sized.h, sized.p = k11.h.clone(), k11.p.clone()
    assert moved <= ties


@pytest.mark.parametrize("H", [64, 16])
def test_recorded_draws_reproduce_the_reference(golden_dir, H):
    """rs_pfgru_sized_step_recorded with the reference's own recorded draws (tests/golden/pfgru_sized.npz, RADTEAM_core.PFGRUCell at
    hidden_size H)."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.pfgru import PFGRUCell, PredictorBank, pack_sized_weights
    g = np.load(os.path.join(golden_dir, "pfgru_sized.npz"))
    pre = f"h{H}_"
    cell = PFGRUCell(hidden_size=H)
    cell.load_state_dict({k[len(pre) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre + "sd_")})
    cell = cell.cuda()
    w = pack_sized_weights([cell])
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    T = g[pre + "obs"].shape[0]
    for tag, carry in (("carry", True), ("fresh", False)):
        h0 = torch.from_numpy(g[f"{pre}{tag}_h0"]).view(1, 1, 40, H).cuda()
        hq = PredictorBank.to_quads(h0).contiguous()
        p = torch.full((1, 1, 40), float(np.log(1 / 40)), dtype=torch.float32, device="cuda")
        for t in range(T):
            obs = torch.zeros(1, 1, 11, device="cuda")
            obs[0, 0, :3] = torch.from_numpy(g[pre + "obs"][t]).cuda()
            eps = torch.from_numpy(g[f"{pre}{tag}_eps"][t]).reshape(1, 1, 40, H).cuda().contiguous()
            idx = torch.from_numpy(g[f"{pre}{tag}_idx"][t].astype(np.int32)).reshape(1, 1, 40).cuda()
            pred = torch.zeros(1, 1, 2, device="cuda")
            h_in, p_in = (hq, p) if carry else (PredictorBank.to_quads(h0).contiguous(), torch.full_like(p, float(np.log(1 / 40))))
            _lib.check(lib.rs_pfgru_sized_step_recorded(w.data_ptr(), obs.data_ptr(), h_in.data_ptr(), p_in.data_ptr(), eps.data_ptr(),
                                                        idx.data_ptr(), None, 1, 0.7, pred.data_ptr(), 1, 1, H, st))
            torch.cuda.synchronize()
            assert np.allclose(pred.cpu().numpy().reshape(-1), g[f"{pre}{tag}_loc"][t].reshape(-1), rtol=1e-4, atol=2e-5), (tag, t)
            assert np.allclose(PredictorBank.from_quads(h_in).cpu().numpy()[0, 0], g[f"{pre}{tag}_h"][t], rtol=1e-4, atol=2e-5), (tag, t)
            assert np.allclose(p_in.cpu().numpy().reshape(-1), g[f"{pre}{tag}_p"][t], rtol=1e-4, atol=2e-5), (tag, t)


@pytest.mark.parametrize("H", [16, 64])
def test_sized_pass_equals_reset_plus_per_step_launches(H):
    """rs_pfgru_sized_pass (up to 8 steps per launch, ragged descending episode lengths) against rs_pfgru_sized_reset + one
    rs_pfgru_sized_step per step: bit for bit, and nothing written for steps past an episode's end."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.pfgru import PFGRUCell, pack_sized_weights
    torch.manual_seed(2)
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cell = PFGRUCell(hidden_size=H).cuda()
    w = pack_sized_weights([cell])
    E, L = 70, 21
    lens = sorted((int(x) for x in torch.randint(1, L + 1, (E,))), reverse=True)
    lens[0] = L
    alive = [sum(1 for n in lens if n > t) for t in range(L)]
    X = torch.rand(L, E, 11, device="cuda")
    base = torch.randint(0, 2 ** 52, (1, E), dtype=torch.int64, device="cuda")
    episode = torch.ones(E, dtype=torch.int64, device="cuda")
    calls = torch.arange(L, dtype=torch.int64, device="cuda").view(L, 1).expand(L, E).contiguous()
    h = torch.empty(1, E, H // 4, 40, 4, device="cuda"); p = torch.empty(1, E, 40, device="cuda")
    loc = torch.full((L, E, 2), -1.0, device="cuda")
    _lib.check(lib.rs_pfgru_sized_pass(w.data_ptr(), X.data_ptr(), h.data_ptr(), p.data_ptr(), base.data_ptr(), episode.data_ptr(),
                                       calls.data_ptr(), 0.7, loc.data_ptr(), (C.c_int32 * L)(*alive), L, E, H, st))
    h2 = torch.empty_like(h); p2 = torch.empty_like(p)
    ref = torch.full((L, E, 2), -1.0, device="cuda")
    _lib.check(lib.rs_pfgru_sized_reset(h2.data_ptr(), p2.data_ptr(), base.data_ptr(), episode.data_ptr(), calls.data_ptr(), None, E, 1, H, st))
    for t in range(L):
        _lib.check(lib.rs_pfgru_sized_step(w.data_ptr(), X[t].data_ptr(), h2.data_ptr(), p2.data_ptr(), base.data_ptr(), episode.data_ptr(),
                                           calls[t].data_ptr(), None, 1, 0.7, ref[t].data_ptr(), alive[t], 1, H, st))
    torch.cuda.synchronize()
    for t in range(L):
        assert torch.equal(loc[t, :alive[t]], ref[t, :alive[t]]), t
        assert bool((loc[t, alive[t]:] == -1.0).all()), t


def test_sized_predictions_do_not_depend_on_sharding():
    from radiation_ppo_amd.pfgru import PredictorBank
    N, A, H = 96, 2, 64
    torch.manual_seed(9)
    full = PredictorBank(N, A, hidden_size=H, seed=5, env_id_base=0, carry_hidden=True, device="cuda")
    halves = [PredictorBank(N // 2, A, hidden_size=H, seed=5, env_id_base=b, carry_hidden=True, device="cuda") for b in (0, N // 2)]
    for hb in halves:
        for a in range(A):
            hb.load_state_dict(a, full.state_dict(a))
    full.reset(); [hb.reset() for hb in halves]
    g = torch.Generator(device="cuda").manual_seed(1)
    for t in range(4):
        obs = _obs(N, A, g)
        pf = full.predict(obs)
        ph = torch.cat([halves[0].predict(obs[:N // 2].contiguous()), halves[1].predict(obs[N // 2:].contiguous())])
        assert torch.equal(pf, ph), t
    assert torch.equal(full.h, torch.cat([hb.h for hb in halves], dim=1))


def test_sized_bank_resume_round_trip():
    from radiation_ppo_amd.pfgru import PredictorBank
    N, A, H = 64, 2, 64
    a, b = (PredictorBank(N, A, hidden_size=H, seed=3, carry_hidden=True, device="cuda") for _ in range(2))
    for i in range(A):
        b.load_state_dict(i, a.state_dict(i))
    g = torch.Generator(device="cuda").manual_seed(4)
    a.reset()
    a.predict(_obs(N, A, g))
    b.load_resume_state(a.resume_state())
    assert torch.equal(a.h, b.h) and torch.equal(a.p, b.p)
    obs = _obs(N, A, g)
    assert torch.equal(a.predict(obs), b.predict(obs)) and torch.equal(a.h, b.h)


def _cnn_run(use_graph, H=64):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    N, A, T, L = 24, 2, 20, 7
    torch.manual_seed(8)
    env = RadSearchVec(N, number_agents=A, obstruction_count=1, enforce_grid_boundaries=True, seed=SEED, env_id_base=32)
    gc = CNNCritic().cuda()
    agents = {i: CNNAgentPPO(id=i, GlobalCritic=gc, GlobalCriticOptimizer=torch.optim.Adam(gc.parameters(), lr=1e-3)) for i in range(A)}
    col = CNNCollector(env, agents, T, L, global_critic_flag=True, use_graph=use_graph, predictor_hidden_size=H)
    assert col.predictor.impl == "hip" and col.predictor.sized and col.predictor.H == H
    out = []
    for _ in range(2):
        col.collect()
        out.append({k: getattr(col.buf, k).clone() for k in ("obs", "act", "rew", "val", "logp", "cut")} | {"h": col.predictor.h.clone()})
    assert (col._graph is not None) == use_graph
    return out


def test_cnn_collector_graph_replay_equals_eager_steps_at_64_units():
    g, e = _cnn_run(True), _cnn_run(False)
    for ep in range(2):
        for k in e[ep]:
            assert torch.equal(g[ep][k], e[ep][k]), (ep, k)


def _rnn_collector(rec, N=48, T=26, L=8, use_graph=True, base=16):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector
    torch.manual_seed(4)
    env = RadSearchVec(N, number_agents=1, obstruction_count=1, enforce_grid_boundaries=True, seed=SEED, env_id_base=base)
    agents = {0: RNNAgentPPO(id=0, steps_per_epoch=T, steps_per_episode=L, train_pi_iters=2, train_pfgru_iters=2, seed=3,
                             actor_critic_args=dict(hidden_sizes_rec=(rec,)))}
    return env, agents, RNNCollector(env, agents, T, L, use_graph=use_graph)


def test_rnn_collector_at_rec_64_runs_the_sized_bank_glued_and_replays_through_the_oracle():
    N, T, L = 48, 26, 8
    env, agents, col = _rnn_collector(64, N=N, T=T, L=L, base=0)            # the oracle numbers its envs from 0
    assert agents[0].agent.sized_pfgru and not agents[0].agent.fused_pfgru
    assert col.bank.impl == "hip" and col.bank.sized and col.use_glue
    col.collect()
    assert col._graph is not None
    _replay_check(col, agents, N, T, L, 1, stride=4)


def test_rnn_collector_graph_replay_equals_eager_steps_at_rec_64():
    def run(use_graph):
        env, agents, col = _rnn_collector(64, use_graph=use_graph)
        out = []
        for ep in range(2):
            col.collect()
            out.append({k: getattr(col.buf, k).clone() for k in ("obs", "act", "rew", "val", "logp", "last_val", "cut")})
            if ep == 0:                                              # new PFGRU weights: the replayed graph reads the re-packed buffer
                with torch.no_grad():                                # (an update is left out: the library-op PFGRU training pass at
                    for p in agents[0].agent.model.parameters():     # 64 units is not bitwise deterministic)
                        p.mul_(1.25)
        assert (col._graph is not None) == use_graph
        return out
    g, e = run(True), run(False)
    assert not torch.equal(e[0]["val"], e[1]["val"])
    for ep in range(2):
        for k in e[ep]:
            assert torch.equal(g[ep][k], e[ep][k]), (ep, k)


def test_rada2c_update_at_rec_64_matches_the_library_path():
    """update_agent at rec 64.  (1) The policy loop's PFGRU pass on rs_pfgru_sized_pass against the torch composition with the same
    keys (PredictorBank(impl="torch") keyed like the pass: episode 1, step t): on every valid step equal within tolerance, except in
    episodes where a resampling uniform came within a near-tie of a CDF value (a moved index then carries on).  (2) One update on the
    sized path and one on the library path (whose draws follow HashDraws' own counter): the same number of policy iterations, losses
    within 5 %.  The PFGRU's own training pass is library ops on both paths."""
    from radiation_ppo_amd.pfgru import PredictorBank
    from radiation_ppo_amd.rada2c import HashDraws, RNNAgentPPO
    from test_rnn_sized_gpu import _batch
    B = _batch(23, T=48, N=80, spread=0.05)
    torch.manual_seed(31)
    ag = RNNAgentPPO(id=0, seed=1, train_pi_iters=3, train_pfgru_iters=1, actor_critic_args=dict(hidden_sizes_rec=(64,)))
    X = B.X.contiguous()
    L, E = X.shape[0], X.shape[1]
    d = HashDraws(B.key * 64 + 17, H=64, hid=ag.agent.hid)
    bank = PredictorBank(E, 1, hidden_size=64, carry_hidden=True, device="cuda", impl="torch")
    bank.cells[0] = ag.agent.model
    bank._base = d.k.view(1, E).clone()
    bank.record_margin = True
    with torch.no_grad():
        lh = ag._pfgru_pass_hip(X, d, B.lens_host)
        bank.reset()
        lt, tie = [], []
        for t in range(L):
            lt.append(bank.predict(X[t].view(E, 1, 11).contiguous())[:, 0])
            tie.append(bank.last_margin[0] < TIE)
    lt, tie = torch.stack(lt), torch.stack(tie)
    valid = B.valid.bool()
    bad = ((~torch.isclose(lh, lt, rtol=RTOL, atol=ATOL)).any(-1) & valid).any(0)
    near = (tie & valid).any(0)
    assert not bool((bad & ~near).any()), (int(bad.sum()), int(near.sum()))
    assert int(bad.sum()) <= int(near.sum())
    res = []
    for sized in (True, False):
        torch.manual_seed(31)
        ag = RNNAgentPPO(id=0, seed=1, train_pi_iters=3, train_pfgru_iters=1, actor_critic_args=dict(hidden_sizes_rec=(64,)))
        ag.agent.sized_pfgru = sized
        res.append(ag.update_agent(B))
        torch.cuda.synchronize()
    ra, rb = res
    assert ra.stop_iteration == rb.stop_iteration
    for k in ("loss_policy", "loss_critic"):
        assert np.isfinite(getattr(ra, k)) and np.isclose(getattr(ra, k), getattr(rb, k), rtol=5e-2, atol=1e-3), (k, getattr(ra, k), getattr(rb, k))


def test_evaluation_with_a_rec_64_agent_matches_the_library_path():
    from radiation_ppo_amd import evaluate as ev
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    sets = ev.sample_test_environments(6, obstruction_count=1, seed=77)
    ag = RNNAgentPPO(id=0, seed=1, actor_critic_args=dict(hidden_sizes_rec=(64,)))
    runs = []
    for sized in (True, False):
        ag.agent.sized_pfgru = sized
        runs.append(ev.run_test_environments(ag, sets, montecarlo_runs=3, steps_per_episode=30, obstruction_count=1, seed=5,
                                             return_actions=True))
    ag.agent.sized_pfgru = True
    (ra, sa, aa), (rb, sb, ab) = runs
    assert int((aa != ab).any(axis=0).sum()) <= 1 and (aa != 8).sum() > 0
    if (aa == ab).all():
        assert [r.total_episode_length for r in ra] == [r.total_episode_length for r in rb] and sa["success_rate"] == sb["success_rate"]


def test_train_ppo_radteam_with_a_64_unit_predictor_end_to_end(tmp_path):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.pfgru import PFGRUCell
    from radiation_ppo_amd.train import train_PPO
    vec = RadSearchVec(32, number_agents=2, obstruction_count=0, enforce_grid_boundaries=True, seed=SEED)
    sim = train_PPO(env=vec, logger_kwargs=dict(output_dir=str(tmp_path)), seed=2, number_of_agents=2, actor_critic_architecture="cnn",
                    global_critic_flag=True, steps_per_epoch=24, steps_per_episode=8, total_epochs=1, save_freq=1,
                    ppo_kwargs=dict(train_pi_iters=2, train_v_iters=2, predictor_hidden_size=64))
    assert sim.collector.predictor.impl == "hip" and sim.collector.predictor.H == 64
    sim.train()
    found = [os.path.join(r, f) for r, _, fs in os.walk(str(tmp_path)) for f in fs if f == "predictor.pt"]
    assert found
    sd = torch.load(found[0], map_location="cpu", weights_only=True)
    assert sd["fc_z.weight"].shape == (64, 67)
    PFGRUCell(hidden_size=64).load_state_dict(sd)
