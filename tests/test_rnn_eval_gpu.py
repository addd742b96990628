"""The Monte-Carlo evaluation of the recurrent agent, RAD-A2C, as the one-agent case of the team's (csrc/rs_eval.hip,
evaluate.run_test_environments_rnn, a front to run_test_environments_rnn_team): rs_rnn_eval_post_step and rs_rnn_eval_post_refresh --
the entries that widen rs_rnn_eval_state to a team of one -- against the torch composition, bit for bit; the fused run against the
composed one with carried and with fresh hidden states, at the default and at sized widths; the fused sequential run replayed through
the oracle; the early stop on the device-side finished-lane count; the guard and the evaluate_PPO driver.  The shared pieces are in
tests/_rnn_eval.py and tests/_eval_runs.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _eval_runs as V  # noqa: E402
import _rnn_eval as H  # noqa: E402
from _rnn_eval import DEV, WIDTHS, _args  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ the two kernels
@pytest.mark.parametrize("optional", [True, False], ids=["counters", "no_counters"])
@pytest.mark.parametrize("Rl", [1, 3])
@pytest.mark.parametrize("N", [70, 300])
def test_rnn_eval_post_step_equals_the_torch_composition_bit_for_bit(N, Rl, optional):
    """14 lock-steps of hand-made env rows with integer-valued readings up to ~900, steps_per_episode 4.  N = 70: a ragged wave;
    N = 300: two 256-thread workgroups.  Lanes with n % 5 == 3 enter finished, lanes with n % 3 == 1 with Welford count 0; the terminal
    flag rises where (n + 3 t) % 11 == 0, every other run ends at the step limit.  A lane that runs from lock-step 0 has all of its at
    most 3 x 4 steps behind it after 12 lock-steps, so the lanes that must NOT finish are started late: the caller raises `active` of
    the lanes with n % 7 == 5 before lock-step 11 and their terminal flag stays down (3 steps: no run of 4 ends).  After every
    lock-step every array the struct names is compared, dtype and value; `no_counters` passes pf_calls = idle_act8 = NULL and those
    two arrays must then keep their start values."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    T, L = 14, 4
    g = torch.Generator(device=DEV).manual_seed(77 + N + Rl)
    env_obs = torch.rand(T, N, 1, 11, device=DEV, generator=g)
    env_obs[..., 0] = torch.floor(env_obs[..., 0] * 900.0)
    env_rew = (torch.rand(T, N, device=DEV, generator=g) - 0.7) * 3.0
    n = torch.arange(N, device=DEV)
    k, t = H.Lanes(N, 1, Rl, "hip"), H.Lanes(N, 1, Rl, "torch")
    env_done = torch.stack([((n + 3 * i) % 11 == 0) & ~k.late for i in range(T)]).to(torch.uint8)
    assert bool((k.active == 0).any()) and bool((k.active != 0).any()) and bool((k.stat.count[k.active != 0] == 0).any())
    o, r, d = torch.zeros_like(env_obs[0]), torch.zeros_like(env_rew[0]), torch.zeros_like(env_done[0])
    state = k.struct(L, o, r, d, optional, single=True)
    calls0, idle0 = t.calls.clone(), t.idle.clone()
    by_done = by_limit = next_runs = 0
    for i in range(T):
        if i == 11:
            for s in (k, t):
                s.active.masked_fill_(s.late, 1)
        o.copy_(env_obs[i]); r.copy_(env_rew[i]); d.copy_(env_done[i])
        _lib.check(lib.rs_rnn_eval_post_step(C.byref(state), H.stream()), "rs_rnn_eval_post_step")
        found, over, last = t.post_step(L, env_obs[i], env_rew[i], env_done[i])
        if not optional:
            t.calls.copy_(calls0); t.idle.copy_(idle0)
        torch.cuda.synchronize()
        H.same(k, t, i)
        by_done += int(found.sum())
        by_limit += int((over & ~found).sum())
        next_runs += int(t.again.sum())
    assert by_done > 0 and by_limit > 0 and (next_runs > 0) == (Rl > 1)
    started = ~t.done_before
    assert bool((started & (t.active == 0)).any()) and bool((t.active != 0).any())      # finished inside the 14 steps, and not
    assert int(t.finished.item()) == int((t.active == 0).sum()) and bool((t.stat.std > 1.0).any())


def test_rnn_eval_post_refresh_restarts_the_statistics_of_the_masked_lanes_only():
    """again set on the lanes with n % 3 == 0 -- set and clear lanes in every wave, 130 lanes: a ragged last wave.  The masked lanes
    equal DeviceWelford's reset + update + standardize on the refreshed rows bit for bit, every other lane and every other array
    keeps its sentinel."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    N, Rl = 130, 3
    g = torch.Generator(device=DEV).manual_seed(11)
    obs = torch.rand(N, 1, 11, device=DEV, generator=g)
    obs[..., 0] = torch.floor(obs[..., 0] * 900.0)
    n = torch.arange(N, device=DEV)
    k, t = H.Lanes(N, 1, Rl, "hip"), H.Lanes(N, 1, Rl, "torch")
    for s in (k, t):
        s.again.copy_((n % 3 == 0).to(torch.uint8))
        s.stat.count.fill_(7.0); s.stat.mean.fill_(123.5); s.stat.sq.fill_(9.25); s.stat.std.fill_(3.5)
    rew, done = torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rs_rnn_eval_post_refresh(C.byref(k.struct(4, obs, rew, done, single=True)), H.stream()), "rs_rnn_eval_post_refresh")
    t.post_refresh(obs)
    torch.cuda.synchronize()
    H.same(k, t)
    m = n % 3 == 0
    assert torch.equal(k.stat.count[m], torch.ones(int(m.sum()), 1, dtype=torch.float64, device=DEV))
    assert torch.equal(k.stat.mean[m][:, 0], obs[m][:, 0, 0].double()) and torch.equal(k.cur[m], obs[m])
    assert bool((k.stat.count[~m] == 7.0).all()) and bool((k.stat.mean[~m] == 123.5).all()) and bool((k.stat.sq[~m] == 9.25).all())
    assert bool((k.stat.std[~m] == 3.5).all()) and bool((k.cur[~m] == -1.0).all()) and bool((k.x[~m] == -2.0).all())
    assert bool((k.x[m][:, 0, 0] == 0.0).all()) and torch.equal(k.x[m][:, 0, 1:], obs[m][:, 0, 1:])


# ------------------------------------------------------------------------------------------------------ whole runs
E, R, L, SET_SEED = 6, 4, 30, 77
# seed of the run per (widths, carried hidden states, obstructions): chosen on the GPU so that among the E * R runs both a found
# source and a run that reaches the step limit occur (asserted below)
SEEDS = {("default", True, 0): 321, ("default", True, 2): 20, ("default", False, 0): 321, ("default", False, 2): 5,
         ("sized", True, 0): 123, ("sized", True, 2): 321, ("sized", False, 0): 123, ("sized", False, 2): 321}


def _run(agent, sets, obst, seed, fused, carry, runs=R, steps=L):
    from radiation_ppo_amd.evaluate import run_test_environments_rnn
    return run_test_environments_rnn(agent, sets, montecarlo_runs=runs, steps_per_episode=steps, obstruction_count=obst, seed=seed,
                                     return_actions=True, carry_hidden_across_runs=carry, fused=fused)


@pytest.mark.parametrize("obst", [0, 2])
@pytest.mark.parametrize("carry", [True, False], ids=["carried", "lane_per_run"])
@pytest.mark.parametrize("widths", list(WIDTHS))
def test_fused_run_equals_the_composed_run(widths, carry, obst):
    from radiation_ppo_amd.evaluate import sample_test_environments
    sets = sample_test_environments(E, obstruction_count=obst, seed=SET_SEED)
    agent = H.agent(widths)
    assert agent.agent.fused_policy == (widths == "default") and agent.agent.fused_pfgru == (widths == "default")
    seed = SEEDS[widths, carry, obst]
    res_f, sum_f, act_f = _run(agent, sets, obst, seed, True, carry)
    res_c, sum_c, act_c = _run(agent, sets, obst, seed, False, carry)
    lanes = E if carry else E * R
    assert act_f.dtype == act_c.dtype == np.int8 and act_f.shape[1] == act_c.shape[1] == lanes
    assert 1 <= act_f.shape[0] <= (L * R if carry else L)
    common = min(act_f.shape[0], act_c.shape[0])
    assert np.array_equal(act_f[:common], act_c[:common]), np.argwhere(act_f[:common] != act_c[:common])[:6]
    assert (act_f[common:] == 8).all() and (act_c[common:] == 8).all()
    assert int(act_f.min()) >= 0 and (act_f < 8).any()
    assert len(res_f) == len(res_c) == E and sum_f["completed_runs"] == sum_c["completed_runs"] == E * R
    V.same_records(res_f, res_c, R)
    assert sum_f["success_rate"] == sum_c["success_rate"]
    n_success = sum(r.success_counter for r in res_f)
    timed_out = sum(l == L for r in res_f for l in r.unsuccessful.episode_length)
    assert 0 < n_success < E * R and timed_out > 0, (n_success, timed_out)


def test_fused_sequential_run_replays_through_the_oracle(monkeypatch):
    """tests/test_evaluate_gpu.py: test_sequential_runs_carry_the_hidden_state_like_the_reference, part (ii), on the fused runner:
    every lane replays through the oracle -- refresh_environment, the logged actions, refresh again ... -- to the same lengths and
    success flags in run order and to returns within 1e-4 (that test's tolerance), while the GRU's h0 and the particle sets were drawn
    exactly once.  An idle row (8) ends a lane's replay: the policy draws 0..7."""
    from radiation_ppo_amd import evaluate as ev
    from radiation_ppo_amd.pfgru import PredictorBank
    seed, obst = SEEDS["default", True, 2], 2                    # a run with a found source among the 24
    sets = ev.sample_test_environments(E, obstruction_count=obst, seed=SET_SEED)
    agent = H.agent()
    calls = {"h0": 0, "bank_reset": 0}
    h0, br = agent.agent.gru_h0, PredictorBank.reset
    monkeypatch.setattr(agent.agent, "gru_h0", lambda u: (calls.__setitem__("h0", calls["h0"] + 1), h0(u))[1])
    monkeypatch.setattr(PredictorBank, "reset", lambda self, mask=None: (calls.__setitem__("bank_reset", calls["bank_reset"] + 1), br(self, mask))[1])
    results, summary, actions = _run(agent, sets, obst, seed, True, True)
    assert calls == {"h0": 1, "bank_reset": 1}
    assert summary["completed_runs"] == E * R and actions.shape[1] == E and 0 < sum(r.success_counter for r in results) < E * R
    V.check_records(results, V.replay_carried(sets, actions[:, :, None], seed, obst, R, L), R)


def test_the_run_stops_on_the_device_side_count_at_the_next_sixteenth_step():
    """The detector starts 5 cm from the source; a step moves at most 100 cm and the terminal radius is 110 cm, so every run ends at its
    first step whatever is drawn.  Carried hidden states: a lane's 4 runs take lock-steps 0..3; a lane per run: lock-step 0.  The host
    reads the finished-lane count every 16 lock-steps: 16 rows, idle (8) from there on.  (The fused form alone, carried runs, a
    [lock-steps, lanes] log: not the assertions of _eval_runs.check_stops_at_the_sixteenth.)"""
    Es, Rs = 3, 4
    sets = V.near_sets(Es)
    agent = H.agent()
    for carry, busy in ((True, Rs), (False, 1)):
        results, summary, actions = _run(agent, sets, 0, 5, True, carry, runs=Rs, steps=40)
        assert actions.shape == (16, Es if carry else Es * Rs), (carry, actions.shape)
        assert (actions[:busy] < 8).all() and (actions[busy:] == 8).all()
        assert summary["completed_runs"] == Es * Rs and summary["success_rate"] == 1.0
        for res in results:
            assert res.success_counter == Rs and res.total_episode_length == [1] * Rs and res.successful.episode_length == [1] * Rs
            assert res.unsuccessful.episode_length == []


# ------------------------------------------------------------------------------------------------------ guard and driver
def test_the_fused_form_refuses_a_width_no_kernel_serves():
    from radiation_ppo_amd.evaluate import run_test_environments_rnn
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    sets = {"env_0": (np.array([1350.0, 1350.0]), np.array([400.0, 400.0]), 2_000_000, 20)}
    wide = RNNAgentPPO(id=0, actor_critic_args=_args(80, 32, 32, 24))                    # rs_rnn_sized_step serves 1..64 GRU units
    assert not wide.agent.fused_policy and not wide.agent.sized_policy
    with pytest.raises(ValueError):
        run_test_environments_rnn(wide, sets, montecarlo_runs=2, steps_per_episode=5, fused=True)
    with pytest.raises(ValueError):
        run_test_environments_rnn(H.agent(), sets, montecarlo_runs=2, steps_per_episode=5, fused=True, device="cpu")


def test_evaluate_ppo_driver_reaches_the_rnn_runner(tmp_path, monkeypatch):
    joblib = pytest.importorskip("joblib")
    from radiation_ppo_amd import evaluate as ev_mod
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.train import train_PPO
    sets = ev_mod.sample_test_environments(4, obstruction_count=0, seed=3)
    os.makedirs(tmp_path / "sets")
    joblib.dump(sets, str(tmp_path / "sets" / "test_env_dict_obs0_high_v4"))
    env = RadSearchVec(16, number_agents=1, obstruction_count=0, enforce_grid_boundaries=True, seed=2)
    train_PPO(env=env, logger_kwargs=dict(output_dir=str(tmp_path / "models")), ppo_kwargs=dict(train_pi_iters=1, train_pfgru_iters=1),
              seed=2, number_of_agents=1, actor_critic_architecture="rnn", global_critic_flag=False, steps_per_epoch=12,
              steps_per_episode=6, total_epochs=1).train()
    seen = []
    real = ev_mod.run_test_environments_rnn
    monkeypatch.setattr(ev_mod, "run_test_environments_rnn", lambda agent, *a, **k: (seen.append((agent, k)), real(agent, *a, **k))[1])
    kw = dict(test_env_path=str(tmp_path / "sets"), obstruction_count=0, snr="high", episodes=3, montecarlo_runs=4,
              model_path=str(tmp_path / "models"), actor_critic_architecture="rnn", number_of_agents=1, steps_per_episode=10,
              enforce_boundaries=True, seed=1)
    results, summary = ev_mod.evaluate_PPO(dict(kw)).evaluate()
    assert len(results) == 3 and summary["completed_runs"] == 3 * 4 and 0.0 <= summary["success_rate"] <= 1.0
    (agent, k), = seen
    assert hasattr(agent.agent, "gru_cell") and k["fused"] is None and k["carry_hidden_across_runs"] is True
    assert k["montecarlo_runs"] == 4 and k["steps_per_episode"] == 10
    del seen[:]
    results, summary = ev_mod.evaluate_PPO(dict(kw, carry_hidden_across_runs=False)).evaluate()
    assert summary["completed_runs"] == 3 * 4 and seen[0][1]["carry_hidden_across_runs"] is False
