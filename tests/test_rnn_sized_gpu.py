"""The RAD-A2C actor-critic at widths other than the CLI default on the sized kernels (csrc/rs_rnn_sized.hip): the policy step, the GRU
sequence and the heads-loss against the torch composition and autograd, the default-size kernels (K12 / K14 / K15) against the sized
ones forced at (24, 32, 32), the GRU-state reset bitwise, and the routing of collector, update and evaluation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_ppo_gpu import SEED, _replay_check  # noqa: E402

pytestmark = pytest.mark.gpu


def _args(hid, pol, val, rec=24):
    return dict(hidden=((hid,),), hidden_sizes_pol=((pol,),), hidden_sizes_val=((val,),), hidden_sizes_rec=(rec,))


def _agent(hid, pol, val, rec=24, **kw):
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    ag = RNNAgentPPO(id=0, seed=1, actor_critic_args=_args(hid, pol, val, rec), **kw)
    with torch.no_grad():
        for p in ag.agent.pi.parameters():
            p.mul_(1.7)
    return ag


def _batch(seed, T=60, N=150, spread=0.25):
    from radiation_ppo_amd.rada2c import pack_episodes
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand(T, N, 11, generator=g).cuda()
    act = torch.randint(0, 8, (T, N), generator=g).cuda()
    adv, ret = torch.randn(T, N, generator=g).cuda(), torch.randn(T, N, generator=g).cuda()
    logp = (float(np.log(1 / 8)) + spread * torch.randn(T, N, generator=g)).cuda()
    src = (torch.rand(T, N, 2, generator=g) * 2000 + 200).cuda()
    cut = (torch.rand(T, N, generator=g) < 0.08).to(torch.uint8)
    cut[-1] = 1
    return pack_episodes(obs, act, adv, ret, logp, src, cut.cuda(), n_total=N, seed=3, sort_by_length=True)


def _torch_step(ag, x, loc, h, u):
    with torch.no_grad():
        logits_t, v_t, h_t = ag.agent.policy_step(x, loc, h)
        lp_all = torch.log_softmax(logits_t, dim=-1)
        cdf = torch.cumsum(lp_all.exp(), dim=-1)
        act_t = (cdf[:, :-1] <= u.unsqueeze(-1)).sum(dim=-1)
    return logits_t, v_t, h_t, lp_all, cdf, act_t


def _check_draw(act, lp, act_t, lp_all, cdf, u):
    edge = (cdf[:, :-1] - u.unsqueeze(-1)).abs().amin(dim=1) < 1e-5      # a uniform within rounding of a CDF step may fall either side
    assert bool(((act == act_t) | edge).all()) and int((act != act_t).sum()) <= 2
    same = act == act_t
    assert torch.allclose(lp[same], lp_all.gather(-1, act_t.unsqueeze(-1)).squeeze(-1)[same], rtol=1e-5, atol=5e-6)


@pytest.mark.parametrize("hid", [1, 8, 13, 24, 32, 48, 64])
def test_sized_step_matches_torch_composition(hid):
    """rs_rnn_sized_step against RNNModelActorCritic.policy_step + the collector's inverse-CDF draw, for odd and tier-boundary widths: the
    plain form (N not a multiple of 64, in-place state), the rows form on agent 1 of [N, 2, .] tensors, the masked value-only form."""
    for pol, val in [(2, 64), (5, 40), (32, 32), (64, 16), (64, 64)]:
        torch.manual_seed(12)
        ag = _agent(hid, pol, val)
        assert ag.agent.sized_policy == ((hid, pol, val) != (24, 32, 32))
        if not ag.agent.sized_policy:
            continue
        N = 1000
        g = torch.Generator().manual_seed(2)
        x = torch.randn(N, 11, generator=g).cuda()
        loc = torch.rand(N, 2, generator=g).cuda()
        h = (torch.rand(N, hid, generator=g) * 0.4 - 0.2).cuda()
        u = torch.rand(N, generator=g).cuda()
        logits_t, v_t, h_t, lp_all, cdf, act_t = _torch_step(ag, x, loc, h, u)
        hk = h.clone()
        logits = torch.empty(N, 8, device="cuda"); v = torch.empty(N, device="cuda"); lp = torch.empty(N, device="cuda")
        act = torch.empty(N, dtype=torch.int64, device="cuda")
        ag.policy_step_hip(x, loc, hk, u=u, h_out=hk, logits=logits, value=v, act=act, logp=lp)
        key = (hid, pol, val)
        assert torch.allclose(hk, h_t, rtol=1e-5, atol=2e-6), (key, float((hk - h_t).abs().max()))
        assert torch.allclose(logits, logits_t, rtol=1e-5, atol=5e-6), (key, float((logits - logits_t).abs().max()))
        assert torch.allclose(v, v_t, rtol=1e-5, atol=5e-6), (key, float((v - v_t).abs().max()))
        _check_draw(act, lp, act_t, lp_all, cdf, u)
        # rows form: agent 1 of [N, 2, .] tensors, state updated in place, int8 action row; then the masked bootstrap form
        A = 2
        xr = torch.randn(N, A, 11, device="cuda"); xr[:, 1] = x
        lr = torch.rand(N, A, 2, device="cuda"); lr[:, 1] = loc
        ur = torch.rand(N, A, device="cuda"); ur[:, 1] = u
        hr = h.clone()
        vr = torch.zeros(N, device="cuda"); lpr = torch.zeros(N, device="cuda")
        ar = torch.zeros(N, dtype=torch.int64, device="cuda")
        a8 = torch.full((N, A), -1, dtype=torch.int8, device="cuda")
        ag.policy_step_rows(xr, lr, hr, ur, 1, value=vr, act=ar, logp=lpr, act8=a8)
        assert torch.allclose(hr, h_t, rtol=1e-5, atol=2e-6) and torch.allclose(vr, v_t, rtol=1e-5, atol=5e-6)
        _check_draw(ar, lpr, act_t, lp_all, cdf, u)
        assert torch.equal(a8[:, 1].long(), ar) and bool((a8[:, 0] == -1).all())
        mask = (torch.rand(N, generator=g) < 0.3).to(torch.uint8).cuda()
        vb = torch.full((N,), 7.0, device="cuda")
        hb = h.clone()
        ag.policy_step_rows(xr, lr, hb, None, 1, value=vb, mask8=mask)
        m = mask.bool()
        assert torch.allclose(vb[m], v_t[m], rtol=1e-5, atol=5e-6) and bool((vb[~m] == 7.0).all()) and torch.equal(hb, h)


@pytest.mark.parametrize("hid", [1, 13, 32, 48, 64])
def test_sized_gru_sequence_matches_torch_gru(hid):
    """rs_gru_sized_forward / _backward (rada2c.GRUSequenceSized) against torch.nn.GRU and its autograd: every state and all four
    parameter gradients (float32, different summation order)."""
    from radiation_ppo_amd.rada2c import GRUSequenceSized
    torch.manual_seed(2)
    L, E = 37, 333
    gru = torch.nn.GRU(13, hid, 1).cuda()
    x = torch.randn(L, E, 13, device="cuda")
    h0 = (torch.rand(E, hid, device="cuda") * 2 - 1) * 0.2
    wgt = torch.randn(L, E, hid, device="cuda") * (torch.rand(L, E, 1, device="cuda") < 0.7)
    with torch.backends.cudnn.flags(enabled=False):
        ref, _ = gru(x, h0.unsqueeze(0))
    (ref * wgt).sum().backward()
    want = {k: p.grad.clone() for k, p in gru.named_parameters()}
    gru.zero_grad()
    got = GRUSequenceSized.apply(x, h0, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
    assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5), float((got - ref).abs().max())
    (got * wgt).sum().backward()
    for k, p in gru.named_parameters():
        assert torch.allclose(p.grad, want[k], rtol=1e-4, atol=1e-3 * float(want[k].abs().max())), (k, float((p.grad - want[k]).abs().max()))


@pytest.mark.parametrize("hid,pol,val", [(32, 64, 64), (13, 5, 40), (64, 48, 16)])
def test_policy_update_on_sized_kernels_equals_the_library_path(hid, pol, val):
    """One update_rada2c pass on the sized GRU sequence + heads-loss against the same pass on torch.nn.GRU, the torch heads and
    autograd: statistics and every pi gradient, with both clip sides hit."""
    from radiation_ppo_amd.rada2c import HashDraws
    B = _batch(19)
    out = []
    for sized in (True, False):
        torch.manual_seed(22)
        ag = _agent(hid, pol, val)
        ag.use_sized = sized
        ag.agent.train()
        ag.pi_optimizer.zero_grad(set_to_none=True)
        loss, st = ag.a2c_losses(B, slice(0, B.lens.shape[0]), HashDraws(B.key * 64 + 17, hid=hid))
        loss.backward()
        out.append((st.clone(), {k: p.grad.clone() for k, p in ag.agent.pi.named_parameters()}))
    assert float(out[1][0][2]) > 0.01
    assert torch.allclose(out[0][0], out[1][0], rtol=2e-5, atol=1e-7), (out[0][0], out[1][0])
    for k in out[0][1]:
        a, b = out[0][1][k], out[1][1][k]
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-4 * float(b.abs().max()) + 1e-9), (k, float((a - b).abs().max()), float(b.abs().max()))


def test_sized_kernels_at_the_default_widths_agree_with_k12_k14_k15():
    """The sized kernels forced at (24, [32], [32]) against K14, K12 and K15 on the same inputs."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.rada2c import GRUSequence, GRUSequenceSized, HeadsLoss, HeadsLossSized, pack_sized_policy_weights
    torch.manual_seed(3)
    ag = _agent(24, 32, 32)
    assert ag.agent.fused_policy and not ag.agent.sized_policy
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N = 777
    x = torch.randn(N, 11, device="cuda"); loc = torch.rand(N, 2, device="cuda"); u = torch.rand(N, device="cuda")
    h = torch.rand(N, 24, device="cuda") * 0.4 - 0.2
    outs = []
    for sized in (True, False):
        hk = h.clone()
        lg = torch.empty(N, 8, device="cuda"); v = torch.empty(N, device="cuda"); lp = torch.empty(N, device="cuda")
        a = torch.empty(N, dtype=torch.int64, device="cuda")
        if sized:
            w = pack_sized_policy_weights(ag.agent)
            _lib.check(lib.rs_rnn_sized_step(w.data_ptr(), 24, 32, 32, x.data_ptr(), 11, loc.data_ptr(), 2, hk.data_ptr(), u.data_ptr(), 1,
                                             hk.data_ptr(), lg.data_ptr(), v.data_ptr(), a.data_ptr(), lp.data_ptr(), None, 1, None, N, st), "step")
        else:
            ag.policy_step_hip(x, loc, hk, u=u, h_out=hk, logits=lg, value=v, act=a, logp=lp)
        outs.append((hk, lg, v, a, lp))
    for s, k in zip(outs[0], outs[1]):
        if s.dtype == torch.int64:
            assert int((s != k).sum()) <= 2
        else:
            assert torch.allclose(s, k, rtol=1e-5, atol=5e-6), float((s - k).abs().max())
    # K12
    gru = ag.agent.pi.logits_net.v_net.seq_model
    L, E = 29, 201
    X = torch.randn(L, E, 13, device="cuda"); h0 = torch.rand(E, 24, device="cuda") * 0.4 - 0.2
    wgt = torch.randn(L, E, 24, device="cuda")
    res = []
    for fn in (GRUSequenceSized, GRUSequence):
        gru.zero_grad()
        hs = fn.apply(X, h0, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
        (hs * wgt).sum().backward()
        res.append((hs.detach().clone(), [p.grad.clone() for p in gru.parameters()]))
    assert torch.allclose(res[0][0], res[1][0], rtol=1e-5, atol=2e-6)
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))
    # K15
    S = 3000
    hs = torch.rand(S, 24, device="cuda") * 2 - 1
    act = torch.randint(0, 8, (S,), device="cuda")
    adv, ret = torch.randn(S, device="cuda"), torch.randn(S, device="cuda")
    lpo = float(np.log(1 / 8)) + 0.25 * torch.randn(S, device="cuda")
    wt = torch.rand(S, device="cuda") / S
    vn = ag.agent.pi.logits_net.v_net
    hres = []
    for fn, w in ((HeadsLossSized, pack_sized_policy_weights(ag.agent)), (HeadsLoss, ag.policy_weights())):
        hx = hs.clone().requires_grad_(True)
        params = [vn.Woms[0].weight, vn.Woms[0].bias, vn.Woms[2].weight, vn.Woms[2].bias, vn.Valms[0].weight, vn.Valms[0].bias,
                  vn.Valms[2].weight, vn.Valms[2].bias]
        loss, stt = fn.apply(hx, *params, w, act, adv, ret, lpo, wt, 0.2, 0.01)
        gr = torch.autograd.grad(loss, [hx] + params)
        hres.append((stt, gr))
    assert torch.allclose(hres[0][0], hres[1][0], rtol=1e-5, atol=1e-8)
    for a, b in zip(hres[0][1], hres[1][1]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()) + 1e-10), float((a - b).abs().max())


def _collector(hid, pol, val, rec=24, N=64, T=30, L=10, use_graph=True, base=0, A=1, obst=1):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector
    torch.manual_seed(4)
    env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=SEED, env_id_base=base)
    agents = {a: RNNAgentPPO(id=a, steps_per_epoch=T, steps_per_episode=L, train_pi_iters=2, train_pfgru_iters=2, seed=3 + a,
                             actor_critic_args=_args(hid, pol, val, rec)) for a in range(A)}
    with torch.no_grad():
        for ag in agents.values():
            for p in ag.agent.pi.parameters():
                p.mul_(2.0)
    return env, agents, RNNCollector(env, agents, T, L, use_graph=use_graph)


@pytest.mark.parametrize("hid", [1, 32, 64])
def test_sized_h0_reset_equals_the_hash_composition(hid):
    env, agents, col = _collector(hid, 16, 16, N=70, T=8, L=4, use_graph=False)
    assert col.use_sized and not col.use_k14
    col.start()
    g = torch.Generator().manual_seed(3)
    for rep in range(3):
        mask = (torch.rand(70, generator=g) < 0.5).cuda() if rep else None
        begun = col.episodes_begun.clone()
        h_before = col.h.clone()
        pf = (col.bank.h.clone(), col.bank.p.clone(), col.bank.episode.clone(), col.bank.calls.clone())
        col._reset_hidden(mask)
        got = col.h.clone()
        col.episodes_begun.copy_(begun); col.h.copy_(h_before)
        col.bank.h = pf[0]; col.bank.p.copy_(pf[1]); col.bank.episode.copy_(pf[2]); col.bank.calls.copy_(pf[3])
        col.use_sized = False
        col._reset_hidden(mask)
        col.use_sized = True
        assert torch.equal(got, col.h), rep
        if mask is not None:
            assert torch.equal(got[:, ~mask], h_before[:, ~mask]) and not torch.equal(got[:, mask], h_before[:, mask])


def test_sized_collector_takes_the_glued_lock_step_and_replays_through_the_oracle(monkeypatch):
    """At (32, [64], [64], rec 24) the collector runs the glued lock-step with the sized step, its buffers replay through the pinned
    train-loop oracle, and the update runs no library GRU."""
    N, T, L = 64, 30, 10
    env, agents, col = _collector(32, 64, 64, N=N, T=T, L=L, use_graph=True)
    assert col.use_glue and col.use_sized and not col.use_k14 and agents[0].agent.fused_pfgru and not agents[0].agent.fused_policy
    col.collect()
    assert col._graph is not None
    _replay_check(col, agents, N, T, L, 1, stride=5)

    def no_library_gru(*a, **k):
        raise AssertionError("library GRU on the sized path")
    monkeypatch.setattr(torch.nn.GRU, "forward", no_library_gru)
    before = torch.cat([p.detach().reshape(-1).clone() for p in agents[0].agent.parameters()])
    r = col.update()[0]
    after = torch.cat([p.detach().reshape(-1) for p in agents[0].agent.parameters()])
    assert np.isfinite([r.loss_policy, r.loss_critic, r.kl_divergence]).all() and not torch.equal(before, after)


def test_sized_glued_lock_step_equals_the_torch_composition():
    """Glued lock-step with the sized step (one and two agents) against the collector's torch composition: bit for bit."""
    for A in (1, 2):
        res = []
        for glue in (True, False):
            env, agents, col = _collector(13, 5, 40, N=80, T=26, L=8, use_graph=False, A=A, base=32)
            assert col.use_glue
            col.use_glue = glue
            out = []
            for ep in range(2):
                col.collect()
                out.append({k: getattr(col.buf, k).clone() for k in ("obs", "act", "rew", "val", "logp", "last_val", "cut")}
                           | {"h": col.h.clone(), "begun": col.episodes_begun.clone()})
            res.append(out)
        for ep in range(2):
            for k in res[0][ep]:
                assert torch.equal(res[0][ep][k], res[1][ep][k]), (A, ep, k)


def test_sized_graph_replay_equals_eager_steps():
    def run(use_graph):
        env, agents, col = _collector(48, 40, 24, N=48, T=26, L=8, use_graph=use_graph, base=16)
        out = []
        for ep in range(2):
            col.collect()
            out.append({k: getattr(col.buf, k).clone() for k in ("obs", "act", "rew", "val", "logp", "last_val", "cut", "adv", "ret")})
            if ep == 0:
                col.update()
                with torch.no_grad():
                    for p in agents[0].agent.pi.parameters():
                        p.mul_(1.5)
        assert (col._graph is not None) == use_graph
        return out
    g, e = run(True), run(False)
    assert not torch.equal(e[0]["val"], e[1]["val"])
    for ep in range(2):
        for k in e[ep]:
            assert torch.equal(g[ep][k], e[ep][k]), (ep, k)


def test_sized_collector_is_sharding_invariant():
    N, T, L = 32, 24, 8
    full = _collector(32, 64, 64, N=N, T=T, L=L, obst=0)[2]
    half = _collector(32, 64, 64, N=N // 2, T=T, L=L, base=N // 2, obst=0)[2]
    full.collect(); half.collect()
    for name in ("obs", "act", "rew", "cut"):
        assert torch.equal(getattr(full.buf, name)[:, N // 2:], getattr(half.buf, name)), name
    assert torch.allclose(full.buf.logp[:, N // 2:], half.buf.logp, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("hid,pol,val", [(32, 64, 64), (64, 48, 16)])
def test_update_agent_on_the_sized_path_equals_the_library_path(hid, pol, val):
    """One update_agent (PFGRU update + policy iterations) on the sized kernels against the library-op path on the same batch."""
    B = _batch(23, T=48, N=80, spread=0.05)
    res = []
    for sized in (True, False):
        torch.manual_seed(31)
        ag = _agent(hid, pol, val, train_pi_iters=3, train_pfgru_iters=1)
        ag.use_sized = sized
        r = ag.update_agent(B)
        torch.cuda.synchronize()
        res.append((r, {k: p.detach().clone() for k, p in ag.agent.pi.named_parameters()}))
    (ra, pa), (rb, pb) = res
    assert ra.stop_iteration == rb.stop_iteration
    for k in pa:
        assert torch.allclose(pa[k], pb[k], rtol=1e-4, atol=1e-5), (k, float((pa[k] - pb[k]).abs().max()))


def test_train_ppo_at_a_non_default_size_end_to_end(tmp_path):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNModelActorCritic
    from radiation_ppo_amd.train import train_PPO
    vec = RadSearchVec(64, number_agents=1, obstruction_count=0, enforce_grid_boundaries=True, seed=SEED)
    args = _args(32, 64, 64)
    sim = train_PPO(env=vec, logger_kwargs=dict(output_dir=str(tmp_path)), seed=2, number_of_agents=1, actor_critic_architecture="rnn",
                    global_critic_flag=False, steps_per_epoch=36, steps_per_episode=12, total_epochs=2, save_freq=1,
                    ppo_kwargs=dict(train_pi_iters=3, train_pfgru_iters=2, alpha=0.1, actor_critic_args=args))
    assert sim.agents[0].agent.sized_policy
    before = torch.cat([p.detach().reshape(-1).clone() for p in sim.agents[0].agent.parameters()])
    sim.train()
    after = torch.cat([p.detach().reshape(-1) for p in sim.agents[0].agent.parameters()])
    assert not torch.equal(before, after) and torch.isfinite(after).all()
    assert len(sim.loggers[0].rows) == 2
    sd = torch.load(os.path.join(str(tmp_path), "0_agent", "pyt_save", "model.pt"), map_location="cpu")
    RNNModelActorCritic(**args).load_state_dict(sd)
    sim.agents[0].save(os.path.join(str(tmp_path), "round_trip"))
    ag = RNNAgentPPO(id=0, actor_critic_args=args)
    ag.load(os.path.join(str(tmp_path), "round_trip"))
    assert ag.agent.sized_policy
    for k, v in ag.agent.state_dict().items():
        assert torch.equal(v, sim.agents[0].agent.state_dict()[k]), k


def test_evaluation_with_a_sized_agent_equals_the_library_path():
    from radiation_ppo_amd import evaluate as ev
    sets = ev.sample_test_environments(6, obstruction_count=1, seed=77)
    ag = _agent(32, 64, 64)
    with torch.no_grad():
        for p in ag.agent.pi.parameters():
            p.mul_(2.0)
    runs = []
    for sized in (True, False):
        ag.agent.sized_policy = sized
        res, summ, acts = ev.run_test_environments(ag, sets, montecarlo_runs=3, steps_per_episode=30, obstruction_count=1, seed=5,
                                                   return_actions=True)
        runs.append((res, summ, acts))
    ag.agent.sized_policy = True
    (ra, sa, aa), (rb, sb, ab) = runs
    # a uniform within rounding of a CDF step may fall either side, and the lane then follows another trajectory: at most one such lane
    assert int((aa != ab).any(axis=0).sum()) <= 1 and (aa != 8).sum() > 0
    if (aa == ab).all():
        assert [r.total_episode_length for r in ra] == [r.total_episode_length for r in rb] and sa["success_rate"] == sb["success_rate"]


def test_out_of_set_widths_route_as_before():
    from radiation_ppo_amd.rada2c import RNNModelActorCritic
    assert not RNNModelActorCritic(**_args(65, 32, 32)).sized_policy
    assert not RNNModelActorCritic(**_args(32, 1, 32)).sized_policy and not RNNModelActorCritic(**_args(32, 32, 65)).sized_policy
    assert not RNNModelActorCritic(hidden=((32,),), hidden_sizes_pol=((20, 12),), hidden_sizes_val=((10,),)).sized_policy
    assert not RNNModelActorCritic().sized_policy and RNNModelActorCritic().fused_policy
    env, agents, col = _collector(65, 32, 32, N=16, T=6, L=3, use_graph=False)
    assert not col.use_sized and not col.use_k14 and not col.use_glue
    col.collect()
    env, agents, col = _collector(32, 64, 64, rec=12, N=16, T=6, L=3, use_graph=False)
    assert col.use_sized and not col.use_glue and col.bank.impl == "torch"        # PFGRU at 12 units: library ops, no glue
    col.collect()
    _replay_check(col, agents, 16, 6, 3, 1, stride=4)
