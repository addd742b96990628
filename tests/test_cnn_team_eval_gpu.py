"""The HIP lock-step of the RAD-TEAM (CNN) Monte-Carlo evaluation, run_test_environments_cnn_team, and its two kernels.

rs_cnn_team_trunk_infer against one rs_cnn_trunk_infer per agent, bit for bit: a round is three images, so N = 1, 2, 3, 4 and 64, 65 sit at
its edges, 193 spans several workgroups, and (4099, 3) has more rounds (1367) than the resident grid, which is then no divisor of them:
the stride loop runs with a ragged last trip.  Fresh maps (both cells -1) and agents sharing a cell are among the lanes
(_cnn_team_ref.random_maps); a2 lies between sentinel guard rows.

rs_cnn_team_eval_head against float64 under the rule of tests/_cnn_team_ref.py (its CPU self-check: test_cnn_team_eval_cpu.py) on a2 from
the trunk kernel, at N = 1, 31, 32, 33, 63, 64, 65, 130 (the 32-image MFMA tile, the 64-image workgroup, ragged tiles) with 3 agents and
(64, 8) for the full team; the existing path (rs_cnn_trunk_infer + BLAS linear + rs_cnn_head) goes through the same rule in the same
test.  Every worst ratio is printed; profiles/cnn_team_head_float64_ratios.txt keeps a copy.

Both bodies are tests/_cnn_team_drive.py's (check_team_trunk, head_matches_float64_and_so_does_the_existing_path), run here with
FAMILY27; the any-side twin is tests/test_cnn_sized_team_eval_gpu.py.

Whole runs: every lane of a fused run replayed through the oracle, fused against composed, the early stop, the arguments, the driver."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_team_drive as D  # noqa: E402
import _cnn_team_ref as T  # noqa: E402
import _eval_runs as V  # noqa: E402

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the team trunk
TRUNK_CASES = [(N, A) for N in (1, 2, 3, 4, 64, 65, 193) for A in (1, 3, 8)] + [(4099, 3)]


@pytest.mark.parametrize("N,A", TRUNK_CASES, ids=[f"N{n}-A{a}" for n, a in TRUNK_CASES])
def test_team_trunk_equals_one_trunk_launch_per_agent_bit_for_bit(N, A):
    seqs = D.actors(A, 27, 100 * N + A)
    maps, cells, pcells = T.random_maps(N, A, seed=31 * N + A)
    if N > 3:
        assert bool(((cells < 0) & (pcells < 0)).all(dim=1).any())                  # a fresh map is among the lanes
    if N > 5 and A > 1:
        assert bool(((cells[:, 0] == cells[:, A - 1]) & (cells[:, 0] >= 0)).any())  # and two agents on one cell
    D.check_team_trunk(D.FAMILY27, "actor", seqs, maps, cells, pcells)


# ------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("N,A", T.CASES, ids=[f"N{n}-A{a}" for n, a in T.CASES])
def test_team_head_matches_float64_and_so_does_the_existing_path(N, A):
    D.head_matches_float64_and_so_does_the_existing_path(D.FAMILY27, A, N)


# ------------------------------------------------------------------------------------------------ whole runs
# chosen on the GPU: with the three Linear layers x 20 (decisive policies) 3 of the 12 lanes find the source within 30 steps, for 2
# agents and for 4; untrained policies at scale 1 found none in 30 steps under any of 24 seed sets
RUN_SEEDS = dict(torch=32, sets=72, run=332)
RUN_SCALE = 20.0


def _agents(A, seed, scale=1.0):
    """A CNN agents with their own predictor cells (the runner loads them into its bank: without them every run would draw a fresh
    random predictor) and, with scale, more decisive policies."""
    from radiation_ppo_amd.pfgru import PFGRUCell
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO
    torch.manual_seed(seed)
    agents = {i: CNNAgentPPO(id=i) for i in range(A)}
    for ag in agents.values():
        ag.model = PFGRUCell().to(ag.device)
    if scale != 1.0:
        with torch.no_grad():
            for ag in agents.values():
                for i in (6, 8, 10):
                    for p in ag.pi.actor[i].parameters():
                        p.mul_(scale)
    return agents


@pytest.mark.parametrize("team_mode", ["individual", "team"])
def test_fused_run_replays_through_the_oracle_and_equals_the_composed_run(team_mode):
    """2 agents, E = 4, R = 3, L = 30, 2 obstructions.  (a) every lane of the fused run replays through the oracle (the same last step,
    success flag and return in run order, finished lanes log 8: tests/_eval_runs.py), both outcomes are among the lanes; (b) the
    composed form gives the same action log and the same records.  The BLAS first layer rounds differently from the MFMA one, so a
    seed could in principle put a uniform between the two paths' CDF steps; these seeds do not."""
    from radiation_ppo_amd.evaluate import run_test_environments_cnn_team, sample_test_environments
    E, R, L, A, obst = 4, 3, 30, 2, 2
    sets = sample_test_environments(E, obstruction_count=obst, seed=RUN_SEEDS["sets"])
    agents = _agents(A, RUN_SEEDS["torch"], RUN_SCALE)
    kw = dict(montecarlo_runs=R, steps_per_episode=L, team_mode=team_mode, obstruction_count=obst, seed=RUN_SEEDS["run"], return_actions=True)
    results, summary, actions = run_test_environments_cnn_team(agents, sets, fused=True, **kw)
    assert len(results) == E and summary["completed_runs"] == E * R and actions.shape[1:] == (E * R, A) and actions.dtype == np.int8
    n_success = V.check_records(results, V.replay_lane_per_run(sets, actions, A, R, L, RUN_SEEDS["run"], obst, team_mode=team_mode), R)
    assert 0 < n_success < E * R, n_success
    res_c, sum_c, act_c = run_test_environments_cnn_team(agents, sets, fused=False, **kw)
    assert act_c.shape == actions.shape and np.array_equal(act_c, actions)
    V.same_records(res_c, results, R)
    assert sum_c["success_rate"] == summary["success_rate"]


def test_fused_run_of_four_agents_replays_and_equals_the_composed_run():
    from radiation_ppo_amd.evaluate import run_test_environments_cnn_team, sample_test_environments
    E, R, L, A, obst = 4, 3, 30, 4, 2
    sets = sample_test_environments(E, obstruction_count=obst, seed=RUN_SEEDS["sets"])
    agents = _agents(A, RUN_SEEDS["torch"], RUN_SCALE)
    kw = dict(montecarlo_runs=R, steps_per_episode=L, obstruction_count=obst, seed=RUN_SEEDS["run"], return_actions=True)
    results, summary, actions = run_test_environments_cnn_team(agents, sets, fused=True, **kw)
    n_success = V.check_records(results, V.replay_lane_per_run(sets, actions, A, R, L, RUN_SEEDS["run"], obst), R)
    assert 0 < n_success < E * R, n_success
    res_c, _, act_c = run_test_environments_cnn_team(agents, sets, fused=False, **kw)
    assert np.array_equal(act_c, actions)
    V.same_records(res_c, results, R)


def test_the_run_stops_on_the_device_side_count_at_the_next_sixteenth_step():
    """The detector starts 5 cm from the source; a step moves at most 100 cm and the terminal radius is 110 cm, so every lane ends at
    lock-step 1 whatever is drawn (one agent: two agents on one spot that draw the same direction collide and neither moves).  The host
    reads the finished-lane count every 16 lock-steps: 16 rows, rows 1..15 idle, in both forms."""
    from radiation_ppo_amd.evaluate import run_test_environments_cnn_team
    E, R = 3, 4
    agents = _agents(1, 11)
    V.check_stops_at_the_sixteenth(lambda sets, fused: run_test_environments_cnn_team(
        agents, sets, montecarlo_runs=R, steps_per_episode=40, seed=5, return_actions=True, fused=fused), E, R, 1)


def test_the_runner_without_predictor_and_its_refusals():
    from radiation_ppo_amd.evaluate import run_test_environments_cnn_team, sample_test_environments
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO
    sets = sample_test_environments(2, obstruction_count=0, seed=8)
    agents = _agents(2, 12)
    kw = dict(montecarlo_runs=2, steps_per_episode=6, seed=3)
    out = {}
    for fused in (True, False):
        results, summary, actions = run_test_environments_cnn_team(agents, sets, use_predictor=False, return_actions=True, fused=fused, **kw)
        assert summary["completed_runs"] == 4 and actions.shape == (6, 4, 2)
        out[fused] = (actions, results)
    assert np.array_equal(out[True][0], out[False][0])
    V.same_records(out[True][1], out[False][1], 2)
    results, summary = run_test_environments_cnn_team(agents, sets, **kw)                       # no log: one fixed action buffer
    assert summary["completed_runs"] == 4
    with pytest.raises(ValueError, match="run_test_environments_cnn"):
        run_test_environments_cnn_team({0: agents[0], 2: agents[1]}, sets, **kw)
    with pytest.raises(ValueError, match="run_test_environments_cnn"):
        run_test_environments_cnn_team(agents, sets, device="cpu", **kw)
    big = {i: CNNAgentPPO(id=i, map_dim=(147, 147)) for i in range(2)}
    with pytest.raises(ValueError, match="run_test_environments_cnn"):                          # walls off: 147 x 147 maps
        run_test_environments_cnn_team(big, sets, enforce_grid_boundaries=False, **kw)
    with pytest.raises(ValueError, match="run_test_environments_cnn"):
        run_test_environments_cnn_team(agents, sets, enforce_grid_boundaries=False, **kw)


def test_evaluate_ppo_driver_reaches_the_team_runner_with_every_agents_own_weights(tmp_path, monkeypatch):
    joblib = pytest.importorskip("joblib")
    from radiation_ppo_amd import evaluate as ev_mod
    from radiation_ppo_amd.evaluate import evaluate_PPO, sample_test_environments
    sets = sample_test_environments(4, obstruction_count=1, seed=3)
    os.makedirs(tmp_path / "sets")
    joblib.dump(sets, str(tmp_path / "sets" / "test_env_dict_obs1_low_v4"))
    saved = {}
    for i, ag in _agents(2, 21).items():
        ag.save(str(tmp_path / "models" / f"{i}_agent"))
        saved[i] = {k: v.clone() for k, v in ag.pi.state_dict().items()}
    assert not torch.equal(saved[0]["actor.6.weight"], saved[1]["actor.6.weight"])       # the two agents are told apart by their weights
    seen = []
    real_team, real_old = ev_mod.run_test_environments_cnn_team, ev_mod.run_test_environments_cnn
    monkeypatch.setattr(ev_mod, "run_test_environments_cnn_team", lambda agents, *a, **k: (seen.append(("team", agents, k)), real_team(agents, *a, **k))[1])
    monkeypatch.setattr(ev_mod, "run_test_environments_cnn", lambda agents, *a, **k: (seen.append(("composed", agents, k)), real_old(agents, *a, **k))[1])
    kw = dict(test_env_path=str(tmp_path / "sets"), obstruction_count=1, snr="low", episodes=3, montecarlo_runs=2,
              model_path=str(tmp_path / "models"), actor_critic_architecture="cnn", number_of_agents=2, steps_per_episode=8,
              enforce_boundaries=True, team_mode="team", seed=1)
    results, summary = evaluate_PPO(dict(kw)).evaluate()
    assert len(results) == 3 and summary["completed_runs"] == 6 and 0.0 <= summary["success_rate"] <= 1.0
    (kind, agents, k), = seen
    assert kind == "team" and sorted(agents) == [0, 1] and k["team_mode"] == "team"
    for i in range(2):
        got = agents[i].pi.state_dict()
        assert set(got) == set(saved[i]) and all(torch.equal(got[name].cpu(), saved[i][name].cpu()) for name in got), i
    assert not torch.equal(agents[1].pi.actor[6].weight.cpu(), saved[0]["actor.6.weight"].cpu())
