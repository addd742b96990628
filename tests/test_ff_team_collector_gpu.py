"""ppo.TeamCollector (rs_ff_team_step between the rs_collect_* glue): the rollout of a feed-forward team.

  * replay: the stored actions, driven env by env through oracle/train_loop_oracle.train_loop_trace (number_of_agents = A, the RAD-A2C
    branch), reproduce every agent column of the buffer -- standardised observations within the 1-ulp Welford rule (rtol 2e-7 / atol
    1e-7), rewards, source targets and cut flags exactly, last_val exactly 0 on terminal cuts and non-zero only at cuts; over two
    epochs, so the state a second collect() starts from is covered;
  * stored logp / val / non-zero last_val against the float64 twin of the OWNING agent within R.fwd_tolerance(R.K6_INIT_SCALES)
    (parameters = nn.Linear's initialisation x 3, as the fused collector's test); a bootstrap row gets the input-distance allowance
    of test_ppo_gpu._stored_outputs_match_float64 (its observation is the oracle's, 1 ulp from the kernel's own);
  * R.check_draw on the stored actions with u recomputed from the documented Philox stream (counter (0, 1 + step in episode,
    episode, 32 + agent), key (seed, env id): test_action_uniforms_are_the_documented_philox_stream);
  * the logger statistics collect() returns, rebuilt from the buffer per agent id;
  * sharding: 96 envs in one collector == envs [0, 32) and [32, 96) in two, every buffer field, bit for bit;
  * the team reward (global_critic_flag on the class), and the train_PPO entry: selection, finite rows, resume."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from oracle.radsearch_oracle import PhiloxDraws, RadSearchOracle, philox4x32_10

sys.path.insert(0, os.path.dirname(__file__))
import _f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 289714752
FIELDS = ("obs", "act", "logp", "val", "rew", "cut", "last_val", "source_tar", "adv", "ret")


def _team(N, A, T, L, obst, seed, team=False, env_id_base=0, agents=None):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.ppo import TeamCollector, VecAgentPPO
    env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=SEED, env_id_base=env_id_base)
    if agents is None:
        torch.manual_seed(seed)
        agents = {a: VecAgentPPO(id=a, steps_per_epoch=T, steps_per_episode=L, number_of_agents=A, alpha=0.1) for a in range(A)}
        with torch.no_grad():
            for ag in agents.values():
                for p in ag.agent.parameters():
                    p.mul_(3.0)                                     # visibly non-uniform policies, each agent its own
    return env, agents, TeamCollector(env, agents, T, L, global_critic_flag=team)


def _rows(buf):
    return {k: getattr(buf, k).cpu().numpy().copy() for k in FIELDS}


def _stack(epochs):
    return {k: np.concatenate([e[k] for e in epochs], axis=0) for k in FIELDS}


def _replay_team(B, envs, A, T, L, obst, epochs, team=False, env_id_base=0):
    """test_ppo_gpu._replay_check for A agents and `epochs` consecutive epochs.  B: the buffers of those epochs stacked along time.
    Returns [(t, n, a, x)]: the standardised pre-reset observation the trace hands agent a's critic at a cut by the time limit or the
    epoch's end."""
    from oracle.train_loop_oracle import train_loop_trace
    obs, act, rew, cut, val, logp, lastv, src = (B[k] for k in ("obs", "act", "rew", "cut", "val", "logp", "last_val", "source_tar"))
    boot = []
    for n in envs:
        ref = RadSearchOracle(PhiloxDraws(SEED, env_id_base + n), number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True)
        st = {"t": 0, "after_step": False, "first": True}

        class Env:
            src = property(lambda s: ref.src)

            def reset(s):
                st["after_step"] = False
                if st["first"]:                      # train() opens with env.reset(): the constructor's reset stands for it
                    st["first"] = False
                    return ref._ret
                return ref.reset()

            def step(s, a):
                r = ref.step(a)
                st["t"] += 1
                st["after_step"] = True
                return r

            def __setattr__(s, k, v):
                setattr(ref, k, v)

        def agent_step(i, observations):
            if st["after_step"] and cut[st["t"] - 1, n, 0]:          # bootstrap call (train.py:476-480)
                boot.append((st["t"] - 1, n, i, np.asarray(observations[i], dtype=np.float64)))
                return 0, float(lastv[st["t"] - 1, n, i]), 0.0
            t = st["t"]
            return int(act[t, n, i]), float(val[t, n, i]), float(logp[t, n, i])

        ev, _ = train_loop_trace(Env(), agent_step, A, team, T, L, epochs, arch="mlp")
        stores = [e for e in ev if e[0] == "store"]
        assert len(stores) == epochs * T * A
        for j, e in enumerate(stores):
            t, a = divmod(j, A)
            assert e[1] == a
            x = np.asarray(e[2], dtype=np.float64).astype(np.float32)
            assert np.allclose(obs[t, n, a], x, rtol=2e-7, atol=1e-7), (n, t, a, obs[t, n, a], x)
            assert tuple(float(v) for v in src[t, n]) == tuple(e[7]), (n, t)
            assert rew[t, n, a] == np.float32(e[3]), (n, t, a)
            assert bool(cut[t, n, a]) == e[8], (n, t, a)
        gae = [e for e in ev if e[0] == "gae"]
        cuts_t = [t for t in range(epochs * T) if cut[t, n, 0]]
        assert len(gae) == len(cuts_t) * A
        for j, e in enumerate(gae):
            t, a = cuts_t[j // A], j % A
            assert e[1] == a and float(lastv[t, n, a]) == e[2], (n, t, a)          # 0.0 where the trace ended on a terminal
        assert ref.err == 0
    return boot


def _uniforms(B, N, A, env_id_base=0):
    """u [T, N, A] of the documented stream, the episode and step counters rebuilt from the stored cut flags."""
    cut = B["cut"]
    u = np.empty(cut.shape, dtype=np.float32)
    for n in range(N):
        ep, k = 0, 0
        for t in range(cut.shape[0]):
            for a in range(A):
                o = philox4x32_10(0, 1 + k, ep, 32 + a, SEED, env_id_base + n)
                u[t, n, a] = np.float32((o[0] >> 8) / 16777216.0)
            k += 1
            if cut[t, n, 0]:
                ep, k = ep + 1, 0
    return u


def _outputs_match_float64(B, agents, boot, envs, name, u):
    """test_ppo_gpu._stored_outputs_match_float64 per agent column, plus check_draw on the stored actions."""
    t_out, t_lp = R.fwd_tolerance(R.K6_INIT_SCALES)
    lastv_all, cut = torch.from_numpy(B["last_val"]), torch.from_numpy(B["cut"]).bool()
    assert not bool((lastv_all != 0)[~cut].any())                  # a bootstrap value exists at cuts only
    assert bool((lastv_all != 0).any())
    for a, ag in agents.items():
        ac64 = R.f64(ag.agent)
        X = torch.from_numpy(B["obs"][:, :, a]).reshape(-1, 11)
        act = torch.from_numpy(B["act"][:, :, a]).reshape(-1)
        logp, val = torch.from_numpy(B["logp"][:, :, a]).reshape(-1), torch.from_numpy(B["val"][:, :, a]).reshape(-1)
        lg64, v64 = R.ff_forward_f64(ac64, X)
        act64, lp_all, cdf64 = R.draw_f64(lg64, torch.from_numpy(u[:, :, a]).reshape(-1))
        lp64 = lp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1)
        rows_a = [(t, n, x) for t, n, i, x in boot if i == a]
        rows = {(t, n) for t, n, _ in rows_a}
        assert len(rows) == len(rows_a) >= 1
        lastv = lastv_all[:, :, a]
        for n in envs:                                              # every non-zero last_val of a replayed env is compared below
            assert all((int(t), n) in rows for t in torch.nonzero(lastv[:, n]).reshape(-1)), (a, n)
        xb = torch.tensor(np.stack([x for _, _, x in rows_a]).astype(np.float32)).double().requires_grad_(True)
        vb64 = ac64.critic(xb).squeeze(-1)
        vb64.sum().backward()
        dx = 2e-7 * xb.detach().abs() + 1e-7
        t_boot = dict(t_out, tiny=t_out["tiny"] + (xb.grad.abs() * dx).sum(-1))
        got_b = torch.stack([lastv[t, n] for t, n, _ in rows_a])
        print(f"TeamCollector stored outputs {name} agent {a} | logp {R.close_ratio(logp, lp64, **t_lp):.4f} "
              f"val {R.close_ratio(val, v64, **t_out):.4f} last_val ({len(rows_a)} rows) {R.close_ratio(got_b, vb64.detach(), **t_boot):.4f} "
              f"draws differing {int((act != act64).sum())}")
        R.close(logp, lp64, f"logp {name} agent {a}", **t_lp)
        R.close(val, v64, f"val {name} agent {a}", **t_out)
        R.close(got_b, vb64.detach(), f"last_val {name} agent {a}", **t_boot)
        R.check_draw(act, logp, act64, lp_all, cdf64, torch.from_numpy(u[:, :, a]).reshape(-1), f"{name} agent {a}")


def _logger_statistics_match(stats, B, N, A, T, L):
    """As test_fused_collector_replays_through_oracle, per agent id: float32 running return per episode; an episode counts when it
    ended on a terminal or a timeout (an epoch cut alone does not; a terminal is the cut whose bootstrap value is exactly 0)."""
    rew, cut, lastv = B["rew"], B["cut"][:, :, 0], B["last_val"]
    lens = None
    for a in range(A):
        rets, ln = [], []
        for n in range(N):
            acc, run = np.float32(0.0), 0
            for t in range(T):
                acc = np.float32(acc + rew[t, n, a]); run += 1
                if cut[t, n]:
                    if t < T - 1 or run == L or lastv[t, n, a] == 0.0:
                        rets.append(float(acc)); ln.append(run)
                    acc, run = np.float32(0.0), 0
        rets = np.array(rets)
        assert lens is None or lens == ln                           # episodes are env-wide
        lens = ln
        assert abs(float(stats["EpRetSum"][a]) - rets.sum()) < 1e-3 and abs(float(stats["EpRetSqSum"][a]) - (rets ** 2).sum()) < 1e-2
        assert abs(float(stats["EpRetMax"][a]) - rets.max()) < 1e-6 and abs(float(stats["EpRetMin"][a]) - rets.min()) < 1e-6
    assert int(stats["EpCount"].item()) == len(lens) >= N * (T // L) - N and float(stats["EpLenSum"].item()) == float(sum(lens))
    assert stats["DoneCount"].shape == (A,) and stats["OutOfBound"].shape == (A,)


def _collect_and_replay(N, A, T, L, obst, seed, stride, team=False):
    env, agents, col = _team(N, A, T, L, obst, seed, team=team)
    stats = col.collect()
    e1 = _rows(col.buf)
    _logger_statistics_match(stats, e1, N, A, T, L)
    col.collect()                                                   # continues from the carried state
    B = _stack([e1, _rows(col.buf)])
    envs = list(range(0, N, stride))
    boot = _replay_team(B, envs, A, T, L, obst, 2, team=team)
    _outputs_match_float64(B, agents, boot, envs, f"N{N} A{A} obst{obst}", _uniforms(B, N, A))
    assert env.error_flags() == 0
    res = col.update()
    assert sorted(res) == list(range(A))
    for r in res.values():
        assert 1 <= r.stop_iteration <= 40
        assert all(np.isfinite(v) for v in (r.loss_policy, r.loss_critic, r.kl_divergence, r.Entropy, r.ClipFrac))
    return B


@pytest.mark.parametrize("N,A,obst,stride", [(24, 2, 2, 2), (80, 4, 0, 5)], ids=["N24-A2-obst2", "N80-A4-free"])
def test_team_collector_replays_through_oracle(N, A, obst, stride):
    _collect_and_replay(N, A, 48, 12, obst, seed=N + A, stride=stride)


def test_team_reward_fills_every_agent_column():
    B = _collect_and_replay(16, 2, 48, 12, 1, seed=5, stride=2, team=True)
    assert np.array_equal(B["rew"][:, :, 0], B["rew"][:, :, 1])
    assert bool((B["rew"] != 0).any())


def test_sharded_collectors_store_the_same_bits():
    """rs_mlp_forward's arithmetic per sample does not depend on the lane or the group the sample sits in; neither may the gather
    or the masking."""
    N, A, T, L = 96, 3, 24, 8
    _, agents, whole = _team(N, A, T, L, 1, seed=9)
    whole.collect()
    parts = []
    for base, n in ((0, 32), (32, 64)):
        _, _, col = _team(n, A, T, L, 1, seed=9, env_id_base=base, agents=copy.deepcopy(agents))
        col.collect()
        parts.append(col.buf)
    for k in FIELDS:
        cat = torch.cat([getattr(p, k) for p in parts], dim=1)
        got = getattr(whole.buf, k)
        assert got.shape == cat.shape and torch.equal(got.contiguous().view(torch.uint8), cat.contiguous().view(torch.uint8)), k


def _sim(env, A, epochs, T=24, L=8, **kw):
    from radiation_ppo_amd.train import train_PPO
    return train_PPO(env=env, logger_kwargs=kw.pop("logger_kwargs", {}),
                     ppo_kwargs=dict(observation_space=11, steps_per_epoch=T, steps_per_episode=L, number_of_agents=A, alpha=0.1, train_pi_iters=5),
                     seed=3, number_of_agents=A, actor_critic_architecture="ff", global_critic_flag=False, steps_per_epoch=T, steps_per_episode=L,
                     total_epochs=epochs, **kw)


def test_train_ppo_selects_the_team_collector():
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.ppo import Collector, FusedCollector, TeamCollector
    sim = _sim(RadSearchVec(32, number_agents=2, obstruction_count=1, enforce_grid_boundaries=True, seed=3), 2, 2)
    assert isinstance(sim.collector, TeamCollector)
    sim.train()
    for i in range(2):
        rows = sim.loggers[i].rows
        assert len(rows) == 2 and rows[1]["TotalEnvInteracts"] == 2 * 24 * 32
        assert all(np.isfinite(float(r[k])) for r in rows for k in ("loss_policy", "loss_critic", "kl_divergence", "Entropy"))
    # single-agent runs keep what they had
    one = _sim(RadSearchVec(20, number_agents=1, obstruction_count=1, enforce_grid_boundaries=True, seed=3), 1, 1)
    assert type(one.collector) is Collector
    one = _sim(RadSearchVec(32, number_agents=1, obstruction_count=1, enforce_grid_boundaries=True, seed=3), 1, 1)
    assert type(one.collector) is FusedCollector


def test_resumed_team_run_equals_the_uninterrupted_run(tmp_path):
    """One epoch, save_resume, a fresh train_PPO, load, one more epoch == two uninterrupted epochs: every parameter and buf.obs."""
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.ppo import TeamCollector

    def make(out, epochs):
        env = RadSearchVec(16, number_agents=2, obstruction_count=2, enforce_grid_boundaries=True, seed=11)
        return _sim(env, 2, epochs, T=20, L=8, logger_kwargs=dict(output_dir=str(out)), save_freq=1)

    def params(sim):
        return torch.cat([p.detach().reshape(-1) for ag in sim.agents.values() for p in ag.agent.parameters()])

    whole = make(tmp_path / "whole", 2)
    whole.train()
    first = make(tmp_path / "first", 1)
    first.train()
    second = make(tmp_path / "second", 2)
    assert isinstance(second.collector, TeamCollector)
    second.load(str(tmp_path / "first"))
    assert second.epochs_done == 1
    second.train()
    assert torch.equal(whole.collector.buf.obs.view(torch.int32), second.collector.buf.obs.view(torch.int32))
    assert torch.equal(params(whole).view(torch.int32), params(second).view(torch.int32))
