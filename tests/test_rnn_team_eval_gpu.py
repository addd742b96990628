"""The HIP Monte-Carlo evaluation of RAD-A2C teams of 1 to 8 recurrent agents (csrc/rs_rnn_policy.hip: rs_rnn_team_eval_step;
csrc/rs_eval.hip: rs_rnn_team_eval_post_step / _post_refresh; evaluate.run_test_environments_rnn_team): the team's policy round against
one K14 launch per agent, bit for bit; the two bookkeeping kernels against the torch composition, bit for bit; the fused run against
the composed one at the default and a sized width with both hidden-state lifetimes; one agent through the team runner against the
records of the commit that still had a one-agent lock-step (tests/golden/rnn_eval_parent.npz); a carried-hidden fused run of two
agents replayed through the oracle; the early stop on the device-side count; the refusals and the evaluate_PPO driver.  The shared
pieces are in tests/_rnn_eval.py and tests/_eval_runs.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _eval_runs as V  # noqa: E402
import _k7_bits as K  # noqa: E402
import _rnn_eval as H  # noqa: E402
from _rnn_eval import DEV, WIDTHS, _args  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ the policy round
MASKS = {"all": lambda n: torch.ones_like(n, dtype=torch.bool), "wave_off": lambda n: (n < 64) | (n >= 128), "thirds": lambda n: n % 3 != 1}


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("N,A", [(70, 2), (200, 3), (65, 8)])
def test_team_step_equals_one_k14_launch_per_agent_bit_for_bit(N, A, mask):
    """N = 70 and 65: a ragged last wave (with `wave_off` that whole wave is inactive and leaves); N = 200: four waves, 64..127 off.
    Every agent has its own random weights, so a wrong blockIdx.y -> agent mapping shows in h and in the draws.  act8 is pre-filled
    with -3: an inactive lane must keep it, and its h row."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(1000 + N + A)
    rnd = lambda *s: torch.rand(*s, device=DEV, generator=g)
    W = [(rnd(5296) - 0.5) * 0.8 for _ in range(A)]
    x, loc, u = rnd(N, A, 11) * 2.0 - 1.0, rnd(N, A, 2), rnd(N, A)
    h0 = rnd(A, N, 24) * 2.0 - 1.0
    active = MASKS[mask](torch.arange(N, device=DEV))
    a8m = active.to(torch.uint8)
    p = lambda t: t.data_ptr()
    h_k, act_k = h0.clone(), torch.full((N, A), -3, dtype=torch.int8, device=DEV)
    wp = (C.c_void_p * A)(*[p(w) for w in W])
    _lib.check(lib.rs_rnn_team_eval_step(wp, A, p(x), p(loc), p(h_k), p(u), p(a8m), p(act_k), N, H.stream()), "rs_rnn_team_eval_step")
    h_r, act_r = h0.clone(), torch.full((N, A), -3, dtype=torch.int8, device=DEV)
    scratch = torch.empty(N, dtype=torch.int64, device=DEV)
    for a in range(A):
        _lib.check(lib.rs_rnn_policy_step_rows(p(W[a]), p(x) + 44 * a, 11 * A, p(loc) + 8 * a, 2 * A, p(h_r[a]), p(u) + 4 * a, A, p(h_r[a]), None,
                                               p(scratch), None, p(act_r) + a, A, p(a8m), N, H.stream()), "rs_rnn_policy_step_rows")
    torch.cuda.synchronize()
    assert torch.equal(h_k, h_r), (h_k != h_r).nonzero()[:6].tolist()
    assert torch.equal(act_k, act_r), (act_k != act_r).nonzero()[:6].tolist()
    assert torch.equal(h_k[:, ~active], h0[:, ~active]) and bool((act_k[~active] == -3).all())
    assert bool((h_k[:, active] != h0[:, active]).any(dim=-1).all())                       # every active (agent, lane) row moved
    assert int(act_k[active].min()) >= 0 and int(act_k[active].max()) <= 7 and len(torch.unique(act_k[active])) > 2
    assert (mask == "all") == bool(active.all())


# ------------------------------------------------------------------------------------------------------ the two bookkeeping kernels
@pytest.mark.parametrize("optional", [True, False], ids=["counters", "no_counters"])
@pytest.mark.parametrize("Rl", [1, 3])
@pytest.mark.parametrize("A", [2, 3])
@pytest.mark.parametrize("N", [70, 300])
def test_team_post_step_equals_the_torch_composition_bit_for_bit(N, A, Rl, optional):
    """tests/test_rnn_eval_gpu.py's schedule with [N][A] rows: 14 lock-steps of hand-made env rows with integer-valued readings up to
    ~900, steps_per_episode 4; lanes with n % 5 == 3 enter finished, lanes with n % 3 == 1 with Welford count 0, lanes with n % 7 == 5
    are started late (before lock-step 11, terminal flag down) so that some lanes do not finish.  The terminal flag rises where
    (n + 3 t) % 11 == 0: on agent 1 ALONE for even n, on agent 0 alone for n % 4 == 1, on every agent for n % 4 == 3 -- a kernel that
    reads agent 0's flag only misses the even lanes.  Every agent has its own reward and its own reading, so a return or a statistic
    taken from the wrong column shows.  After every lock-step every array the struct names is compared, dtype and value;
    `no_counters` passes pf_calls = idle_act8 = NULL and those two arrays must then keep their start values."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    T, L = 14, 4
    g = torch.Generator(device=DEV).manual_seed(77 + N + Rl + 10 * A)
    env_obs = torch.rand(T, N, A, 11, device=DEV, generator=g)
    env_obs[..., 0] = torch.floor(env_obs[..., 0] * 900.0)
    env_rew = (torch.rand(T, N, A, device=DEV, generator=g) - 0.7) * 3.0
    assert bool((env_rew[..., 1] != env_rew[..., 0]).all())
    n = torch.arange(N, device=DEV)
    k, t = H.Lanes(N, A, Rl, "hip"), H.Lanes(N, A, Rl, "torch")
    ag = torch.arange(A, device=DEV).view(1, A)
    who = torch.where((n % 2 == 0).view(N, 1), ag == 1, torch.where((n % 4 == 1).view(N, 1), ag == 0, torch.ones_like(ag, dtype=torch.bool)))
    env_done = torch.stack([(((n + 3 * i) % 11 == 0) & ~k.late).view(N, 1) & who for i in range(T)]).to(torch.uint8)
    assert bool((env_done[:, :, 1] > env_done[:, :, 0]).any()) and bool((env_done[:, :, 0] > env_done[:, :, 1]).any())
    assert bool((k.active == 0).any()) and bool((k.active != 0).any()) and bool((k.stat.count[k.active != 0] == 0).any())
    o, r, d = torch.zeros_like(env_obs[0]), torch.zeros_like(env_rew[0]), torch.zeros_like(env_done[0])
    state = k.struct(L, o, r, d, optional)
    calls0, idle0 = t.calls.clone(), t.idle.clone()
    by_done = by_one = by_limit = next_runs = 0
    for i in range(T):
        if i == 11:
            for s in (k, t):
                s.active.masked_fill_(s.late, 1)
        o.copy_(env_obs[i]); r.copy_(env_rew[i]); d.copy_(env_done[i])
        _lib.check(lib.rs_rnn_team_eval_post_step(C.byref(state), H.stream()), "rs_rnn_team_eval_post_step")
        found, over, last = t.post_step(L, env_obs[i], env_rew[i], env_done[i])
        if not optional:
            t.calls.copy_(calls0); t.idle.copy_(idle0)
        torch.cuda.synchronize()
        H.same(k, t, i)
        by_done += int(found.sum())
        by_one += int((found & (env_done[i, :, 0] == 0)).sum())
        by_limit += int((over & ~found).sum())
        next_runs += int(t.again.sum())
    assert by_done > by_one > 0 and by_limit > 0 and (next_runs > 0) == (Rl > 1)
    started = ~t.done_before
    assert bool((started & (t.active == 0)).any()) and bool((t.active != 0).any())      # finished inside the 14 steps, and not
    assert int(t.finished.item()) == int((t.active == 0).sum()) and bool((t.stat.std > 1.0).any())
    if optional:
        assert bool((t.idle[started & (t.active == 0)] == 8).all())


def test_team_post_refresh_restarts_the_statistics_of_the_masked_lanes_only():
    """again set on the lanes with n % 3 == 0 -- set and clear lanes in every wave, 130 lanes of 3 agents: a ragged last wave.  The
    masked lanes equal DeviceWelford's reset + update + standardize on the refreshed rows bit for bit, for every agent; every other
    lane and every other array keeps its sentinel."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    N, A, Rl = 130, 3, 3
    g = torch.Generator(device=DEV).manual_seed(11)
    obs = torch.rand(N, A, 11, device=DEV, generator=g)
    obs[..., 0] = torch.floor(obs[..., 0] * 900.0)
    n = torch.arange(N, device=DEV)
    k, t = H.Lanes(N, A, Rl, "hip"), H.Lanes(N, A, Rl, "torch")
    for s in (k, t):
        s.again.copy_((n % 3 == 0).to(torch.uint8))
        s.stat.count.fill_(7.0); s.stat.mean.fill_(123.5); s.stat.sq.fill_(9.25); s.stat.std.fill_(3.5)
    rew, done = torch.zeros(N, A, device=DEV), torch.zeros(N, A, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rs_rnn_team_eval_post_refresh(C.byref(k.struct(4, obs, rew, done)), H.stream()), "rs_rnn_team_eval_post_refresh")
    t.post_refresh(obs)
    torch.cuda.synchronize()
    H.same(k, t)
    m = n % 3 == 0
    assert torch.equal(k.stat.count[m], torch.ones(int(m.sum()), A, dtype=torch.float64, device=DEV))
    assert torch.equal(k.stat.mean[m], obs[m][..., 0].double()) and torch.equal(k.cur[m], obs[m])
    assert bool((k.stat.count[~m] == 7.0).all()) and bool((k.stat.mean[~m] == 123.5).all()) and bool((k.stat.sq[~m] == 9.25).all())
    assert bool((k.stat.std[~m] == 3.5).all()) and bool((k.cur[~m] == -1.0).all()) and bool((k.x[~m] == -2.0).all())
    assert bool((k.x[m][..., 0] == 0.0).all()) and torch.equal(k.x[m][..., 1:], obs[m][..., 1:])


# ------------------------------------------------------------------------------------------------------ whole runs
E, R, L, SET_SEED = 6, 4, 30, 77
# seed of the run per (agents, widths, carried hidden states, obstructions): chosen on the GPU so that among the E * R runs both a
# found source and a run that reaches the step limit occur (asserted below)
SEEDS = {(2, "default", True, 0): 321, (2, "default", True, 2): 99, (2, "default", False, 0): 321, (2, "default", False, 2): 5,
         (2, "sized", True, 0): 321, (2, "sized", True, 2): 2, (2, "sized", False, 0): 20, (2, "sized", False, 2): 42,
         (3, "default", True, 2): 5}


def _run(team, sets, obst, seed, fused, carry, runs=R, steps=L):
    from radiation_ppo_amd.evaluate import run_test_environments_rnn_team
    return run_test_environments_rnn_team(team, sets, montecarlo_runs=runs, steps_per_episode=steps, obstruction_count=obst, seed=seed,
                                          return_actions=True, carry_hidden_across_runs=carry, fused=fused)


@pytest.mark.parametrize("A,widths,carry,obst", list(SEEDS), ids=[f"A{a}-{w}-{'carried' if c else 'lane_per_run'}-obst{o}" for a, w, c, o in SEEDS])
def test_fused_run_equals_the_composed_run(A, widths, carry, obst):
    from radiation_ppo_amd.evaluate import sample_test_environments
    sets = sample_test_environments(E, obstruction_count=obst, seed=SET_SEED)
    team = H.team(A, widths)
    assert all(ag.agent.fused_policy == (widths == "default") and ag.agent.fused_pfgru == (widths == "default") for ag in team.values())
    seed = SEEDS[A, widths, carry, obst]
    res_f, sum_f, act_f = _run(team, sets, obst, seed, True, carry)
    res_c, sum_c, act_c = _run(team, sets, obst, seed, False, carry)
    lanes = E if carry else E * R
    assert act_f.dtype == act_c.dtype == np.int8 and act_f.shape[1:] == act_c.shape[1:] == (lanes, A)
    assert 1 <= act_f.shape[0] <= (L * R if carry else L)
    common = min(act_f.shape[0], act_c.shape[0])
    assert np.array_equal(act_f[:common], act_c[:common]), np.argwhere(act_f[:common] != act_c[:common])[:6]
    assert (act_f[common:] == 8).all() and (act_c[common:] == 8).all()
    assert int(act_f.min()) >= 0 and (act_f < 8).any()
    assert ((act_f == 8).all(axis=2) | (act_f < 8).all(axis=2)).all()                     # a lane's agents idle together
    assert sum_f["completed_runs"] == sum_c["completed_runs"] == E * R and len(res_f) == E
    V.same_records(res_f, res_c, R)
    assert sum_f["success_rate"] == sum_c["success_rate"]
    n_success = sum(r.success_counter for r in res_f)
    timed_out = sum(l == L for r in res_f for l in r.unsuccessful.episode_length)
    assert 0 < n_success < E * R and timed_out > 0, (n_success, timed_out)


def test_recurrent_team_start_with_one_agent_is_recurrent_start():
    """A = 1: recurrent_team_start is recurrent_start -- same bank, same h0, bit for bit"""
    from radiation_ppo_amd import evaluate as ev
    team = H.team(1)
    dev = torch.device(DEV)
    bank1, hid1 = ev.recurrent_start(team[0].agent, 50, 3, dev, "hip")
    bankt, hidt = ev.recurrent_team_start(team, 50, 3, dev, "hip")
    assert hidt.shape == (1, 50, 24) and torch.equal(hidt[0], hid1) and torch.equal(bankt.h, bank1.h) and torch.equal(bankt.p, bank1.p)
    assert torch.equal(bankt._base, bank1._base) and torch.equal(bankt.episode, bank1.episode) and bankt.cells[0] is team[0].agent.model


PARENT = K.maker("make_rnn_eval_parent")         # the recorder: its cases, its run() and its encoding


@pytest.mark.parametrize("case", list(PARENT.CASES), ids=[PARENT.name(*c) for c in PARENT.CASES])
def test_one_agent_runs_equal_the_parent_commits(case):
    """tests/golden/rnn_eval_parent.npz holds what run_test_environments_rnn (fused and composed) and run_test_environments computed
    for one recurrent agent before they became fronts to the team runner: today's results equal it member by member -- keys, dtype,
    shape, bytes: every field of the records, the returns as float32 bits, the fused run's action log."""
    want = np.load(PARENT.OUT)
    tag = "." + PARENT.name(*case) + "."
    keys = sorted(k for k in want.files if tag in k)
    got = PARENT.run(case)
    assert sorted(got) == keys and "rnn_fused" + tag + "log" in keys and "rnn_composed" + tag + "id" in keys
    assert ("plain" + tag + "id" in keys) == (case in PARENT.PLAIN)
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert (got["rnn_fused" + tag + "log"] < 8).any()


def test_fused_sequential_team_run_replays_through_the_oracle(monkeypatch):
    """tests/test_rnn_eval_gpu.py: test_fused_sequential_run_replays_through_the_oracle with two agents: every lane replays through the
    oracle -- refresh_environment, both agents' logged actions, refresh again ... -- a run ending when any agent's flag rises or at L,
    returns from individual_reward[0], to the same lengths and success flags in run order and to returns within 1e-4 (that test's
    tolerance); gru_h0 was called once per agent and the bank's particle sets were drawn once.  An idle row (8) ends a lane's replay."""
    from radiation_ppo_amd import evaluate as ev
    from radiation_ppo_amd.pfgru import PredictorBank
    A, obst = 2, 2
    seed = SEEDS[A, "default", True, obst]
    sets = ev.sample_test_environments(E, obstruction_count=obst, seed=SET_SEED)
    team = H.team(A)
    calls = {"h0": 0, "bank_reset": 0}
    br = PredictorBank.reset
    for ag in team.values():
        h0 = ag.agent.gru_h0
        monkeypatch.setattr(ag.agent, "gru_h0", lambda u, h0=h0: (calls.__setitem__("h0", calls["h0"] + 1), h0(u))[1])
    monkeypatch.setattr(PredictorBank, "reset", lambda self, mask=None: (calls.__setitem__("bank_reset", calls["bank_reset"] + 1), br(self, mask))[1])
    results, summary, actions = _run(team, sets, obst, seed, True, True)
    assert calls == {"h0": A, "bank_reset": 1}
    assert summary["completed_runs"] == E * R and actions.shape[1:] == (E, A) and 0 < sum(r.success_counter for r in results) < E * R
    V.check_records(results, V.replay_carried(sets, actions, seed, obst, R, L), R)


def test_the_team_run_stops_on_the_device_side_count_at_the_next_sixteenth_step():
    """The detectors start 5 cm from the source; a step moves at most 100 cm and the terminal radius is 110 cm, so a run ends with the
    first step in which an agent moves or idles unhindered -- its first step, unless the two stacked agents draw the same move: then
    both are refused and the env makes no terminal test (a second step is needed).  Every run is therefore a success after a step or
    two and a lane's at most 4 runs are over well inside 16 lock-steps.  A lane's rows hold actions for exactly as many lock-steps as
    its runs took, then 8; the host reads the finished-lane count every 16 lock-steps: 16 rows.  (The fused form alone, two agents,
    carried runs: not the assertions of _eval_runs.check_stops_at_the_sixteenth.)"""
    Es, Rs, A = 3, 4, 2
    sets = V.near_sets(Es)
    team = H.team(A)
    for carry in (True, False):
        results, summary, actions = _run(team, sets, 0, 5, True, carry, runs=Rs, steps=40)
        assert actions.shape == (16, Es if carry else Es * Rs, A), (carry, actions.shape)
        assert summary["completed_runs"] == Es * Rs and summary["success_rate"] == 1.0
        lens = np.array([res.total_episode_length for res in results])                  # [Es, Rs]
        assert lens.min() == 1 and lens.max() <= 3 and all(res.unsuccessful.episode_length == [] for res in results)
        busy = lens.sum(axis=1) if carry else lens.reshape(-1)                          # lock-steps a lane had a run going
        assert busy.max() < 16
        running = np.arange(16).reshape(16, 1) < busy.reshape(1, -1)
        assert ((actions < 8) == running[:, :, None]).all() and (actions[~running] == 8).all()


# ------------------------------------------------------------------------------------------------------ refusals and driver
def test_the_team_runner_refuses_what_it_cannot_serve():
    from radiation_ppo_amd.evaluate import run_test_environments_rnn_team
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    sets = {"env_0": (np.array([1350.0, 1350.0]), np.array([400.0, 400.0]), 2_000_000, 20)}
    kw = dict(montecarlo_runs=2, steps_per_episode=5)
    team = H.team(2)
    with pytest.raises(ValueError):
        run_test_environments_rnn_team({1: team[0], 2: team[1]}, sets, **kw)                                  # ids must be 0..A-1
    with pytest.raises(ValueError):
        run_test_environments_rnn_team({}, sets, **kw)
    with pytest.raises(ValueError):
        run_test_environments_rnn_team({i: team[0] for i in range(9)}, sets, **kw)                            # more than RS_MAX_AGENTS
    with pytest.raises(ValueError):
        run_test_environments_rnn_team({0: team[0], 1: H.team(1, "sized")[0]}, sets, **kw)                     # mixed widths
    wide = {i: RNNAgentPPO(id=i, actor_critic_args=_args(80, 32, 32, 24)) for i in range(2)}                  # the sized step serves 1..64 units
    assert not wide[0].agent.fused_policy and not wide[0].agent.sized_policy
    with pytest.raises(ValueError):
        run_test_environments_rnn_team(wide, sets, fused=True, **kw)
    with pytest.raises(ValueError):
        run_test_environments_rnn_team(team, sets, fused=True, device="cpu", **kw)
    results, summary = run_test_environments_rnn_team(wide, sets, fused=None, **kw)                           # the composed form serves it
    assert summary["completed_runs"] == 2


def test_evaluate_ppo_driver_reaches_the_team_runner(tmp_path, monkeypatch):
    joblib = pytest.importorskip("joblib")
    from radiation_ppo_amd import evaluate as ev_mod
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.train import train_PPO
    sets = ev_mod.sample_test_environments(4, obstruction_count=0, seed=3)
    os.makedirs(tmp_path / "sets")
    joblib.dump(sets, str(tmp_path / "sets" / "test_env_dict_obs0_high_v4"))
    env = RadSearchVec(16, number_agents=2, obstruction_count=0, enforce_grid_boundaries=True, seed=2)
    train_PPO(env=env, logger_kwargs=dict(output_dir=str(tmp_path / "models")), ppo_kwargs=dict(train_pi_iters=1, train_pfgru_iters=1),
              seed=2, number_of_agents=2, actor_critic_architecture="rnn", global_critic_flag=False, steps_per_epoch=12,
              steps_per_episode=6, total_epochs=1).train()
    seen, seen_one = [], []
    real, real_one = ev_mod.run_test_environments_rnn_team, ev_mod.run_test_environments_rnn
    monkeypatch.setattr(ev_mod, "run_test_environments_rnn_team", lambda agents, *a, **k: (seen.append((agents, k)), real(agents, *a, **k))[1])
    monkeypatch.setattr(ev_mod, "run_test_environments_rnn", lambda agent, *a, **k: (seen_one.append((agent, k)), real_one(agent, *a, **k))[1])
    kw = dict(test_env_path=str(tmp_path / "sets"), obstruction_count=0, snr="high", episodes=3, montecarlo_runs=4,
              model_path=str(tmp_path / "models"), actor_critic_architecture="rnn", number_of_agents=2, steps_per_episode=10,
              enforce_boundaries=True, seed=1)
    results, summary = ev_mod.evaluate_PPO(dict(kw)).evaluate()
    assert len(results) == 3 and summary["completed_runs"] == 3 * 4 and 0.0 <= summary["success_rate"] <= 1.0
    (agents, k), = seen
    assert not seen_one and sorted(agents) == [0, 1] and k["fused"] is None and k["carry_hidden_across_runs"] is True
    assert k["montecarlo_runs"] == 4 and k["steps_per_episode"] == 10
    saved = [torch.load(str(tmp_path / "models" / f"{i}_agent" / "pyt_save" / "model.pt"), map_location=DEV, weights_only=True) for i in range(2)]
    for i in range(2):
        sd = agents[i].agent.state_dict()
        assert agents[i].id == i and sd.keys() == saved[i].keys() and all(torch.equal(sd[n], saved[i][n]) for n in sd)
    assert any(not torch.equal(saved[0][n], saved[1][n]) for n in saved[0] if n.startswith("pi."))
    assert any(not torch.equal(saved[0][n], saved[1][n]) for n in saved[0] if n.startswith("model."))
    del seen[:]
    results, summary = ev_mod.evaluate_PPO(dict(kw, carry_hidden_across_runs=False)).evaluate()
    assert summary["completed_runs"] == 3 * 4 and seen[0][1]["carry_hidden_across_runs"] is False
    with pytest.raises(ValueError):
        ev_mod.evaluate_PPO(dict(kw, team_mode="team")).evaluate()
    del seen[:]
    results, summary = ev_mod.evaluate_PPO(dict(kw, number_of_agents=1)).evaluate()                           # one agent: through the front
    assert len(seen_one) == 1 and hasattr(seen_one[0][0].agent, "gru_cell") and summary["completed_runs"] == 3 * 4
    (agents, k), = seen                                         # the front's own call of the team runner, and no other
    assert list(agents) == [0] and agents[0] is seen_one[0][0] and k["fused"] is True and k["carry_hidden_across_runs"] is True
