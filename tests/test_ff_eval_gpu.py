"""The HIP Monte-Carlo evaluation of feed-forward agents and teams (csrc/rs_eval.hip, evaluate.run_test_environments_team):
rs_ff_eval_step against rs_welford_standardize + rs_ff_team_step's step round and rs_eval_post_step against the torch composition,
both bit for bit; the fused run against the composed one; every lane of a team's run replayed through the oracle; the early stop on
the device-side finished-lane count; and the evaluate_PPO driver, which loads every agent of a feed-forward team."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _eval_runs as V  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _team(A, scale=4.0, seed=9):
    """A agents with their own (decisive: actor weights x scale, as tests/test_evaluate_gpu.py) networks"""
    from radiation_ppo_amd.ppo import VecAgentPPO
    torch.manual_seed(seed)
    agents = {i: VecAgentPPO(id=i, steps_per_epoch=480, steps_per_episode=40) for i in range(A)}
    with torch.no_grad():
        for ag in agents.values():
            for p in ag.agent.actor.parameters():
                p.mul_(scale)
    return agents


def _nets(agents):
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.ppo import mlp_params
    arr = _lib.RsMlpParams * len(agents)
    return (arr(*[mlp_params(agents[a].agent.actor) for a in range(len(agents))]),
            arr(*[mlp_params(agents[a].agent.critic) for a in range(len(agents))]))


# ------------------------------------------------------------------------------------------------------ the policy kernel
@pytest.mark.parametrize("standardise", [True, False], ids=["welford", "raw"])
@pytest.mark.parametrize("N,A", [(30, 1), (130, 3), (64, 8), (2048 * 64 + 70, 1)])
def test_eval_step_equals_standardize_plus_team_step_bit_for_bit(N, A, standardise):
    """(30, 1): one ragged group; (130, 3): a ragged last group and an odd row stride; (64, 8): the full team; (2048*64 + 70, 1): the
    grid-stride loop past the grid cap, in one launch"""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.ppo import DeviceWelford
    lib = _lib.load()
    agents = _team(A, scale=2.0)
    pa, pc = _nets(agents)
    g = torch.Generator(device=DEV).manual_seed(1000 * A + N % 997)
    obs = torch.rand(N, A, 11, device=DEV, generator=g)
    obs[..., 0] = obs[..., 0] * 800.0                               # the raw reading: counts, not a unit-scale number
    stat = DeviceWelford((N, A), DEV)
    stat.mean.copy_(torch.rand(N, A, device=DEV, generator=g, dtype=torch.float64) * 600.0)
    stat.std.copy_(1.0 + torch.rand(N, A, device=DEV, generator=g, dtype=torch.float64) * 80.0)
    u = torch.rand(N, A, device=DEV, generator=g)
    alive = torch.rand(N, device=DEV, generator=g) < 0.6
    alive[0], alive[N - 1] = True, False
    assert bool(alive.any()) and not bool(alive.all())
    # the reference: x from rs_welford_standardize, then rs_ff_team_step's step round on x and u
    x = obs.clone()
    if standardise:
        stat.standardize(obs[..., 0], out=x[..., 0])
    act = torch.full((A, N), -1, dtype=torch.int64, device=DEV)
    f = torch.zeros(A, 3, N, device=DEV)
    _lib.check(lib.rs_ff_team_step(pa, pc, A, x.data_ptr(), u.data_ptr(), act.data_ptr(), f.data_ptr(), None, None, N, _stream()), "team")
    want = torch.where(alive.view(N, 1), act.t(), torch.full_like(act.t(), 8)).to(torch.int8)
    got = torch.full((N, A), -7, dtype=torch.int8, device=DEV)
    m, s = (stat.mean.data_ptr(), stat.std.data_ptr()) if standardise else (None, None)
    _lib.check(lib.rs_ff_eval_step(pa, A, obs.data_ptr(), m, s, u.data_ptr(), alive.view(torch.uint8).data_ptr(), got.data_ptr(), N,
                                   _stream()), "eval")
    torch.cuda.synchronize()
    assert int(act.min()) >= 0 and int(act.max()) <= 7
    assert len(torch.unique(act)) >= 3                              # the draws are not all one action: the comparison means something
    assert torch.equal(got, want), (got != want).nonzero()[:8]


# ------------------------------------------------------------------------------------------------------ the post-step kernel
@pytest.mark.parametrize("use_team", [0, 1], ids=["individual", "team"])
@pytest.mark.parametrize("N,A", [(70, 1), (130, 3), (64, 8)])
def test_eval_post_step_equals_the_torch_composition_bit_for_bit(N, A, use_team):
    """6 lock-steps of hand-made env rows.  done is raised for a single agent only in some lanes (the any-agent rule), some lanes are
    finished on entry, some have Welford count 0 on entry (the first-sample branch)."""
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.ppo import DeviceWelford
    lib = _lib.load()
    T = 6
    g = torch.Generator(device=DEV).manual_seed(77 + N + A)
    env_obs = torch.rand(T, N, A, 11, device=DEV, generator=g)
    env_obs[..., 0] = torch.floor(env_obs[..., 0] * 900.0)
    env_rew = (torch.rand(T, N, A, device=DEV, generator=g) - 0.7) * 3.0
    env_team = (torch.rand(T, N, device=DEV, generator=g) - 0.7) * 3.0
    env_done = torch.zeros(T, N, A, dtype=torch.uint8, device=DEV)
    # one agent at a time: lane n's agent (n + t) % A raises its flag at step t where (n + 2 t) % 7 == 0 -- never two agents at once;
    # lanes with n % 7 == 2 are not reached within the 6 steps
    n_idx = torch.arange(N, device=DEV)
    for t in range(T):
        hit = (n_idx + 2 * t) % 7 == 0
        env_done[t, n_idx[hit], (n_idx[hit] + t) % A] = 1
    env_done[2, 1] = 1                                              # and one lane, alive until then, where every agent raises it
    assert int(env_done.sum(dim=2).max()) == A and (A == 1 or bool((env_done.sum(dim=2) == 1).any()))

    def fresh(impl):
        st = DeviceWelford((N, A), DEV, impl=impl)
        started = (n_idx % 3 != 1).view(N, 1).expand(N, A)         # lanes with n % 3 == 1 enter with count 0
        first = torch.floor(torch.rand(N, A, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) * 900.0).double()
        st.count.copy_(started.double()); st.mean.copy_(torch.where(started, first, torch.zeros_like(first)))
        alive = n_idx % 4 != 2                                      # lanes with n % 4 == 2 are finished on entry,
        success = (~alive) & (n_idx % 8 == 2)                       # half of them successfully
        ep_len = torch.where(alive, torch.zeros_like(n_idx), n_idx % 7 + 1).int()
        ep_ret = torch.where(alive, torch.zeros(N, device=DEV), -0.31 * (n_idx % 7 + 1).float())
        return st, alive.clone(), success.clone(), ep_len, ep_ret, torch.zeros(N, A, 11, device=DEV)

    st_t, alive_t, suc_t, len_t, ret_t, cur_t = fresh("torch")
    st_k, alive_k, suc_k, len_k, ret_k, cur_k = fresh("hip")
    assert bool((st_t.count == 0).any()) and bool((~alive_t).any()) and bool(alive_t.any())
    finished = torch.tensor([int((~alive_k).sum())], dtype=torch.int32, device=DEV)     # the caller's start value: monotonic from there
    o, r, tm, d = (torch.zeros_like(env_obs[0]), torch.zeros_like(env_rew[0]), torch.zeros_like(env_team[0]), torch.zeros_like(env_done[0]))
    p = lambda t: t.data_ptr()
    state = _lib.RsEvalState(N, A, use_team, p(o), p(r), p(tm), p(d), p(cur_k), p(st_k.count), p(st_k.mean), p(st_k.sq), p(st_k.std),
                             p(alive_k.view(torch.uint8)), p(suc_k.view(torch.uint8)), p(len_k), p(ret_k), p(finished))
    for t in range(T):
        o.copy_(env_obs[t]); r.copy_(env_rew[t]); tm.copy_(env_team[t]); d.copy_(env_done[t])
        _lib.check(lib.rs_eval_post_step(C.byref(state), _stream()), "rs_eval_post_step")
        # the torch composition (evaluate.py: the loop body of run_test_environments / run_test_environments_cnn)
        rr = env_team[t] if use_team else env_rew[t][:, 0]
        ret_t += torch.where(alive_t, rr, torch.zeros_like(rr))
        len_t += alive_t.int()
        found = env_done[t].bool().any(dim=1) & alive_t
        suc_t |= found
        alive_t &= ~found
        st_t.update(env_obs[t][..., 0], mask=alive_t)
        cur_t = env_obs[t].clone()
        torch.cuda.synchronize()
        for name, a, b in (("alive", alive_k, alive_t), ("success", suc_k, suc_t), ("ep_len", len_k, len_t), ("ep_ret", ret_k, ret_t),
                           ("count", st_k.count, st_t.count), ("mean", st_k.mean, st_t.mean), ("sq", st_k.sq, st_t.sq),
                           ("std", st_k.std, st_t.std), ("cur_obs", cur_k, cur_t)):
            assert a.dtype == b.dtype and torch.equal(a, b), (t, name)
        assert int(finished.item()) == int((~alive_t).sum()), t
    assert bool(suc_t.any()) and bool(alive_t.any()) and bool((st_t.std > 1.0).any())


# ------------------------------------------------------------------------------------------------------ whole runs
def _run(agents, sets, obst, seed, fused, R=5, L=40, **kw):
    from radiation_ppo_amd.evaluate import run_test_environments_team
    return run_test_environments_team(agents, sets, montecarlo_runs=R, steps_per_episode=L, obstruction_count=obst, seed=seed,
                                      return_actions=True, fused=fused, **kw)


@pytest.mark.parametrize("obst", [0, 3])
@pytest.mark.parametrize("A", [1, 2, 4])
def test_fused_run_equals_the_composed_run(A, obst):
    from radiation_ppo_amd.evaluate import sample_test_environments
    E, R = 6, 5
    sets = sample_test_environments(E, obstruction_count=obst, seed=77)
    agents = _team(A)
    res_f, sum_f, act_f = _run(agents, sets, obst, 123, True)
    res_c, sum_c, act_c = _run(agents, sets, obst, 123, False)
    assert act_f.dtype == np.int8 and act_f.shape[1:] == (E * R, A) and 1 <= act_f.shape[0] <= 40
    assert np.array_equal(act_f, act_c)
    assert len(res_f) == len(res_c) == E and sum_f["completed_runs"] == E * R
    V.same_records(res_f, res_c, R)
    assert sum_f["success_rate"] == sum_c["success_rate"]


# (A, seed of the saved set, seed of the run): chosen on the GPU so that both outcomes are present among the E * R lanes
REPLAY = [(2, 77, 7), (3, 11, 321)]


@pytest.mark.parametrize("A,set_seed,seed", REPLAY, ids=[f"A{c[0]}" for c in REPLAY])
def test_team_monte_carlo_evaluation_matches_oracle_replay(A, set_seed, seed):
    """Every (environment, run) lane replayed through the oracle -- refresh_environment, then the logged joint actions -- ends at the
    same step with the same success flag and agent 0's accumulated float32 return within 1e-4, in run order; a finished lane idles
    (tests/_eval_runs.py)."""
    from radiation_ppo_amd.evaluate import sample_test_environments
    E, R, L, obst = 6, 5, 40, 2
    sets = sample_test_environments(E, obstruction_count=obst, seed=set_seed)
    results, summary, actions = _run(_team(A), sets, obst, seed, True)
    assert len(results) == E and summary["completed_runs"] == E * R
    n_success = V.check_records(results, V.replay_lane_per_run(sets, actions, A, R, L, seed, obst), R)
    assert 0 < n_success < E * R, n_success


def test_the_run_stops_on_the_device_side_count_at_the_next_sixteenth_step():
    """The detector starts 5 cm from the source; a step moves at most 100 cm and the terminal radius is 110 cm, so every lane ends at
    lock-step 1 whatever is drawn.  (One agent: two agents that start on one spot and draw the same direction collide, neither moves,
    and a terminal flag is only raised by a move.)  The host reads the finished-lane count every 16 lock-steps: 16 rows, rows 1..15 idle."""
    E, R, A = 3, 4, 1
    V.check_stops_at_the_sixteenth(lambda sets, fused: _run(_team(A), sets, 0, 5, fused, R=R), E, R, A)


def test_the_runner_refuses_agent_ids_that_are_not_0_to_a_minus_1():
    from radiation_ppo_amd.evaluate import run_test_environments_team
    agents = _team(2)
    with pytest.raises(ValueError):
        run_test_environments_team({0: agents[0], 2: agents[1]}, {"env_0": (np.zeros(2), np.zeros(2), 1, 1)})


# ------------------------------------------------------------------------------------------------------ the driver
def test_evaluate_ppo_driver_loads_every_agent_of_a_feed_forward_team(tmp_path, monkeypatch):
    joblib = pytest.importorskip("joblib")
    from radiation_ppo_amd import evaluate as ev_mod
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.evaluate import evaluate_PPO, sample_test_environments
    from radiation_ppo_amd.train import train_PPO
    sets = sample_test_environments(5, obstruction_count=1, seed=3)
    os.makedirs(tmp_path / "sets")
    joblib.dump(sets, str(tmp_path / "sets" / "test_env_dict_obs1_low_v4"))
    env = RadSearchVec(8, number_agents=2, obstruction_count=1, enforce_grid_boundaries=True, seed=2)
    train_PPO(env=env, logger_kwargs=dict(output_dir=str(tmp_path / "models")), ppo_kwargs=dict(observation_space=11, steps_per_epoch=12, steps_per_episode=6, number_of_agents=2, alpha=0.1, train_pi_iters=1),
              seed=2, number_of_agents=2, actor_critic_architecture="ff", global_critic_flag=False, steps_per_epoch=12, steps_per_episode=6,
              total_epochs=1).train()
    saved = {}
    for i in range(2):
        d, = [x for x in sorted(os.listdir(tmp_path / "models")) if x.startswith(f"{i}_agent")]
        saved[i] = torch.load(str(tmp_path / "models" / d / "pyt_save" / "model.pt"), map_location=DEV, weights_only=True)
    assert not torch.equal(saved[0]["actor.0.weight"], saved[1]["actor.0.weight"])       # the two agents are told apart by their weights
    seen = []
    real_team, real_single = ev_mod.run_test_environments_team, ev_mod.run_test_environments
    monkeypatch.setattr(ev_mod, "run_test_environments_team", lambda agents, *a, **k: (seen.append(("team", agents, k)), real_team(agents, *a, **k))[1])
    monkeypatch.setattr(ev_mod, "run_test_environments", lambda agent, *a, **k: (seen.append(("single", agent, k)), real_single(agent, *a, **k))[1])
    kw = dict(test_env_path=str(tmp_path / "sets"), obstruction_count=1, snr="low", episodes=4, montecarlo_runs=3,
              model_path=str(tmp_path / "models"), actor_critic_architecture="ff", number_of_agents=2, steps_per_episode=10,
              enforce_boundaries=True, team_mode="individual", seed=1)
    results, summary = evaluate_PPO(dict(kw)).evaluate()
    assert len(results) == 4 and summary["completed_runs"] == 4 * 3 and 0.0 <= summary["success_rate"] <= 1.0
    (kind, agents, k), = seen
    assert kind == "team" and sorted(agents) == [0, 1] and k["team_mode"] == "individual"
    for i in range(2):
        got = agents[i].agent.state_dict()
        assert set(got) == set(saved[i]) and all(torch.equal(got[name], saved[i][name]) for name in got), i
    assert not torch.equal(agents[1].agent.actor[0].weight, saved[0]["actor.0.weight"])
    with pytest.raises(ValueError):
        evaluate_PPO(dict(kw, team_mode="team")).evaluate()
    del seen[:]
    results, summary = evaluate_PPO(dict(kw, number_of_agents=1)).evaluate()            # one agent: the path it always took
    assert [s[0] for s in seen] == ["single"] and summary["completed_runs"] == 12
