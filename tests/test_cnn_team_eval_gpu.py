"""The HIP lock-step of the RAD-TEAM (CNN) Monte-Carlo evaluation, run_test_environments_cnn_team, and its two kernels.

rs_cnn_team_trunk_infer against one rs_cnn_trunk_infer per agent, bit for bit: a round is three images, so N = 1, 2, 3, 4 and 64, 65 sit at
its edges, 193 spans several workgroups, and (4099, 3) has more rounds (1367) than the resident grid, which is then no divisor of them:
the stride loop runs with a ragged last trip.  Fresh maps (both cells -1) and agents sharing a cell are among the lanes
(_cnn_team_ref.random_maps); a2 lies between sentinel guard rows.

rs_cnn_team_eval_head against float64 under the rule of tests/_cnn_team_ref.py (its CPU self-check: test_cnn_team_eval_cpu.py) on a2 from
the trunk kernel, at N = 1, 31, 32, 33, 63, 64, 65, 130 (the 32-image MFMA tile, the 64-image workgroup, ragged tiles) with 3 agents and
(64, 8) for the full team; the existing path (rs_cnn_trunk_infer + BLAS linear + rs_cnn_head) goes through the same rule in the same
test.  Every worst ratio is printed; profiles/cnn_team_head_float64_ratios.txt keeps a copy.

Whole runs: every lane of a fused run replayed through the oracle, fused against composed, the early stop, the arguments, the driver."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_team_ref as T  # noqa: E402
import _eval_runs as V  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678
FLAT = 2704


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _prepare(lib, seqs):
    """every actor's convolution weights in K9's layout: wt [A, scratch]"""
    from radiation_ppo_amd import _lib
    wt = torch.empty(len(seqs), lib.rs_cnn_trunk_scratch_floats(6), dtype=torch.float32, device="cuda")
    for a, s in enumerate(seqs):
        _lib.check(lib.rs_cnn_trunk_prepare(6, s[0].weight.data_ptr(), s[0].bias.data_ptr(), s[3].weight.data_ptr(), s[3].bias.data_ptr(),
                                            wt[a].data_ptr(), _stream()), "rs_cnn_trunk_prepare")
    return wt


def _team_trunk(lib, maps, cells32, pcells32, wt, A, N, out):
    from radiation_ppo_amd import _lib
    _lib.check(lib.rs_cnn_team_trunk_infer(maps.data_ptr(), cells32.data_ptr(), pcells32.data_ptr(), A, N, wt.data_ptr(), out.data_ptr(),
                                           _stream()), "rs_cnn_team_trunk_infer")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the team trunk
TRUNK_CASES = [(N, A) for N in (1, 2, 3, 4, 64, 65, 193) for A in (1, 3, 8)] + [(4099, 3)]


@pytest.mark.parametrize("N,A", TRUNK_CASES, ids=[f"N{n}-A{a}" for n, a in TRUNK_CASES])
def test_team_trunk_equals_one_trunk_launch_per_agent_bit_for_bit(N, A):
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import CNNActor
    lib = _lib.load()
    torch.manual_seed(100 * N + A)
    seqs = [CNNActor().cuda().actor for _ in range(A)]
    with torch.no_grad():                                  # make biases matter (pool ties on empty regions, ReLU gates)
        for s in seqs:
            s[0].bias.uniform_(-0.05, 0.15)
            s[3].bias.uniform_(-0.1, 0.1)
    maps, cells, pcells = (t.cuda() for t in T.random_maps(N, A, seed=31 * N + A))
    if N > 3:
        assert bool(((cells < 0) & (pcells < 0)).all(dim=1).any())                  # a fresh map is among the lanes
    if N > 5 and A > 1:
        assert bool(((cells[:, 0] == cells[:, A - 1]) & (cells[:, 0] >= 0)).any())  # and two agents on one cell
    wt = _prepare(lib, seqs)
    G = 2 * FLAT                                           # guard rows on both sides of [A][N][2704]
    buf = torch.full((G + A * N * FLAT + G,), SENTINEL, device="cuda")
    _team_trunk(lib, maps, cells.int().contiguous(), pcells.int().contiguous(), wt, A, N, buf[G:])
    got = buf[G:G + A * N * FLAT].view(A, N, FLAT)
    sent = _bits(torch.full((G,), SENTINEL, device="cuda"))
    assert torch.equal(_bits(buf[:G]), sent) and torch.equal(_bits(buf[G + A * N * FLAT:]), sent), (N, A)
    assert not bool((got == SENTINEL).any()), (N, A)       # every element written
    for a in range(A):
        want = torch.full((N, FLAT), SENTINEL, device="cuda")
        _lib.check(lib.rs_cnn_trunk_infer(maps.data_ptr(), cells.data_ptr(), pcells.data_ptr(), A, a, N, wt[a].data_ptr(), want.data_ptr(),
                                          _stream()), "rs_cnn_trunk_infer")
        torch.cuda.synchronize()
        assert float(want.abs().max()) > 0 and bool(torch.isfinite(want).all())
        assert torch.equal(_bits(got[a]), _bits(want)), (N, A, a)
    if A > 1:
        assert not torch.equal(got[0], got[A - 1])         # the agents are told apart: their own weights and cell columns


# ------------------------------------------------------------------------------------------------ the head
_MASTER = {}


def _master(A):
    """Once per team size: the actors on the GPU, a2 [A, MASTER, 2704] from the team trunk on the master maps, and the head's
    outputs on all MASTER lanes (what a case's lanes must equal bit for bit: grid independence)."""
    if A in _MASTER:
        return _MASTER[A]
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    t = T.team(A)
    seqs = [T.clone_seq(ac.actor, "cuda") for ac in t.actors]
    wt = _prepare(lib, seqs)
    a2 = torch.empty(A, T.MASTER, FLAT, device="cuda")
    _team_trunk(lib, t.maps.cuda(), t.cells.int().cuda(), t.pcells.int().cuda(), wt, A, T.MASTER, a2)
    assert float(a2.min()) >= 0.0 and float((a2 == 0).float().mean()) > 0.2        # non-negative and sparse, as in a run
    m = dict(t=t, seqs=seqs, wt=wt, a2=a2)
    m["out"] = _head(lib, seqs, a2, t.u.cuda(), T.alive_for(t, T.MASTER).cuda(), A, T.MASTER)
    _MASTER[A] = m
    return m


def _head_params(seqs):
    from radiation_ppo_amd import _lib
    p = lambda t: t.data_ptr()
    return (_lib.RsCnnHeadParams * len(seqs))(*[_lib.RsCnnHeadParams(p(s[6].weight), p(s[6].bias), p(s[8].weight), p(s[8].bias), p(s[10].weight),
                                                                      p(s[10].bias)) for s in seqs])


def _head(lib, seqs, a2, u, alive, A, N, outputs=True):
    """rs_cnn_team_eval_head into sentinel-guarded buffers: dict(act8 [N, A], act [A, N], logp [A, N], y1 [A, N, 32]); outputs=False:
    the three optional outputs NULL."""
    from radiation_ppo_amd import _lib
    act8 = torch.full((N + 2, A), -1, dtype=torch.int8, device="cuda")
    act = torch.full((A * N + 2,), -1, dtype=torch.int64, device="cuda")
    logp = torch.full((A * N + 2,), SENTINEL, device="cuda")
    y1 = torch.full((A * N + 2, 32), SENTINEL, device="cuda")
    o = (act[1:].data_ptr(), logp[1:].data_ptr(), y1[1:].data_ptr()) if outputs else (None, None, None)
    _lib.check(lib.rs_cnn_team_eval_head(_head_params(seqs), A, a2.data_ptr(), u.data_ptr(), alive.data_ptr(), act8[1:].data_ptr(), *o, N,
                                         _stream()), "rs_cnn_team_eval_head")
    torch.cuda.synchronize()
    assert bool((act8[0] == -1).all()) and bool((act8[N + 1] == -1).all())          # the guards on both sides
    assert int(act[0]) == -1 and int(act[-1]) == -1
    for t in (logp[0], logp[-1], y1[0], y1[-1]):
        assert torch.equal(_bits(t), _bits(torch.full_like(t, SENTINEL)))
    if not outputs:
        assert bool((act == -1).all()) and torch.equal(_bits(logp), _bits(torch.full_like(logp, SENTINEL)))
    return dict(act8=act8[1:N + 1], act=act[1:A * N + 1].view(A, N), logp=logp[1:A * N + 1].view(A, N), y1=y1[1:A * N + 1].view(A, N, 32))


def _existing_path(lib, m, a, N, u, alive):
    """The collector's composition for agent a on the case's lanes: rs_cnn_trunk_infer + BLAS linear + rs_cnn_head + the idle rule."""
    from radiation_ppo_amd import _lib
    t, s = m["t"], m["seqs"][a]
    A = t.A
    a2 = torch.empty(N, FLAT, device="cuda")
    maps, cells, pcells = t.maps[:N].cuda().contiguous(), t.cells[:N].cuda().contiguous(), t.pcells[:N].cuda().contiguous()
    _lib.check(lib.rs_cnn_trunk_infer(maps.data_ptr(), cells.data_ptr(), pcells.data_ptr(), A, a, N, m["wt"][a].data_ptr(), a2.data_ptr(),
                                      _stream()), "rs_cnn_trunk_infer")
    with torch.no_grad():
        y1 = torch.nn.functional.linear(a2, s[6].weight, s[6].bias)
    act = torch.empty(N, dtype=torch.int64, device="cuda")
    logp = torch.empty(N, device="cuda")
    _lib.check(lib.rs_cnn_head(y1.data_ptr(), s[8].weight.data_ptr(), s[8].bias.data_ptr(), s[10].weight.data_ptr(), s[10].bias.data_ptr(), 8,
                               u.data_ptr() + 4 * a, A, act.data_ptr(), logp.data_ptr(), None, 1, None, 1, 0, None, N, _stream()), "rs_cnn_head")
    torch.cuda.synchronize()
    return a2, y1, act, logp, torch.where(alive != 0, act, torch.full_like(act, 8)).to(torch.int8)


@pytest.mark.parametrize("N,A", T.CASES, ids=[f"N{n}-A{a}" for n, a in T.CASES])
def test_team_head_matches_float64_and_so_does_the_existing_path(N, A):
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    m = _master(A)
    t, seqs = m["t"], m["seqs"]
    a2 = m["a2"][:, :N].contiguous()
    u, alive = t.u[:N].cuda().contiguous(), T.alive_for(t, N).cuda()
    assert int(alive[N - 1]) == 0 and (N == 1 or (int(alive[0]) == 1 and 0 < int(alive.sum()) < N))
    got = _head(lib, seqs, a2, u, alive, A, N)
    refs = [T.reference(t.actors[a].actor, a2[a], u[:, a]) for a in range(A)]
    master_refs = [T.reference(t.actors[a].actor, m["a2"][a], t.u[:, a]) for a in range(A)]
    worst = {k: dict(y1=0.0, logp=0.0, differing=0, unexcused=0, act8=0) for k in ("kernel", "existing")}
    fails = []
    for a in range(A):
        assert T.distinct_actions(master_refs[a]) >= 3, a           # a visibly non-uniform policy that still draws several actions
        if N >= 31:
            assert T.distinct_actions(refs[a]) >= 3, (N, a)
        q = T.ratios(refs[a], u[:, a], alive, got["act"][a], got["logp"][a], got["act8"][:, a], y1=got["y1"][a])
        xa2, y1, act, logp, a8 = _existing_path(lib, m, a, N, u, alive)
        assert torch.equal(_bits(xa2), _bits(a2[a])), a              # both paths start from the same trunk bits
        qe = T.ratios(refs[a], u[:, a], alive, act, logp, a8, y1=y1)
        for name, r in (("kernel", q), ("existing", qe)):
            for k in r:
                worst[name][k] = max(worst[name][k], r[k])
            if not T.passes(r):
                fails.append((name, a, r))
    for name in worst:
        print(f"cnn team head N{N} A{A} {name:8s} | " + " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in worst[name].items()))
    assert not [f for f in fails if f[0] == "existing"], fails       # the existing path past 1.0 would mean the MODEL is wrong
    assert not fails, fails
    assert bool((got["act"] >= 0).all()) and bool((got["act"] <= 7).all())
    want8 = torch.where(alive.view(N, 1) != 0, got["act"].t(), torch.full_like(got["act"].t(), 8)).to(torch.int8)
    assert torch.equal(got["act8"], want8)                           # act8[n][a] = alive[n] ? act[a][n] : 8, exactly
    # the optional outputs NULL: act8 alone, the same rows; a second call: the same bits
    only8 = _head(lib, seqs, a2, u, alive, A, N, outputs=False)
    assert torch.equal(only8["act8"], got["act8"])
    again = _head(lib, seqs, a2, u, alive, A, N)
    for k in got:
        assert torch.equal(_bits(again[k]), _bits(got[k])) if got[k].dtype == torch.float32 else torch.equal(again[k], got[k]), k
    # the same lanes inside a larger N: equal bits (no dependence on N or the grid)
    big = m["out"]
    assert torch.equal(_bits(big["y1"][:, :N]), _bits(got["y1"])) and torch.equal(_bits(big["logp"][:, :N]), _bits(got["logp"]))
    assert torch.equal(big["act"][:, :N], got["act"])


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
