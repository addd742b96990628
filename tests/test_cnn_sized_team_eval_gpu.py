"""The HIP lock-step of the walls-off RAD-TEAM (CNN) Monte-Carlo evaluation, run_test_environments_cnn_team_sized, and its two kernels.

rs_cnn_sized_team_infer against one rs_cnn_sized_infer per agent, bit for bit, a2 between sentinel guard rows and every element written:
sides 8 (P = 4), 31 (P = 15, one ragged tile), 33 (P = 16, exactly one tile), 35 (P = 17, 2 x 2 tiles, the last one cell wide) with N in
(1, 2, 5) and A in (1, 3, 8), 147 with N = 2, and (side 35, N = 130, A = 3): 1560 (agent, image, tile) units on a persistent grid of
three workgroups per CU, 768 on 256 CUs, which the units exceed without being a multiple of it (asserted for any grid under 1500).  The
lanes (_lanes) are the cases of the empty-window shortcut: nothing anywhere, nothing but the owner's stamp, stamps on and one pixel
outside a window's edge rows and columns, a single nonzero / a single -0.0f in a window's corner pixel, a dense map, two agents on one
cell; the host-side model (_cnn_sized_team_ref.shortcut_units) says which units skip conv1, and the test asserts that both kinds occur.

rs_cnn_sized_team_eval_head at P = 4, 5, 14, 15, 16, 73 (wave quarters of 2 and 3 pieces, tails of 0, 16 and 4 floats, the walls-off
depth 85 264): (1) one-hot rows of a2 must give y1 == float32(W1[j][k] + b1[j]) bit for bit at every edge k of the quarters, pieces,
lane halves and tails; (2) the float64 rule of tests/_cnn_team_ref.py with K1 at the case's depth on a2 from the trunk kernel, for the
kernel and for the existing path (rs_cnn_sized_infer + BLAS linear + rs_cnn_head) on the same a2 bits.  Every worst ratio is printed;
profiles/cnn_sized_team_head_float64_ratios.txt keeps a copy.

The trunk check, the guarded head call and the body of (2) are tests/_cnn_team_drive.py's, run here with SIZED; the 27 x 27 twin is
tests/test_cnn_team_eval_gpu.py.  The lanes of the shortcut, the 147-side and resident-grid cases and (1) are this family's own.

Whole runs, walls off, steps_per_episode = 8 (35 x 35 maps): every lane of a fused run replayed through the oracle, fused against
composed, the scratch bound, the early stop, the arguments, the driver."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_sized_team_ref as S  # noqa: E402
import _cnn_team_drive as D  # noqa: E402
import _eval_runs as V  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the team trunk
def _lanes(M, A, N, seed):
    """(maps [N, 4, M, M], cells [N, A], pcells [N, A], tags): the shortcut's cases first, in the order of `tags`, then sparse random
    lanes; a case of N lanes takes the first N.  E = the first pixel of the second tile's window (29) where the map has one."""
    g = torch.Generator().manual_seed(seed)
    maps, cells, pcells = S.random_maps(max(N, 20), A, M, seed)
    E = 29 if M > 29 else M - 1
    cell = lambda r, c: r * M + c
    tags = []

    def lane(tag, planes=None, loc=None, pc=None):
        i = len(tags)
        tags.append(tag)
        maps[i] = 0.0 if planes is None else planes
        cells[i], pcells[i] = -1, -1
        for a, at in (loc or {}).items():
            cells[i, a] = at
        for a, at in (pc or {}).items():
            pcells[i, a] = at

    lane("nothing")                                                                  # every unit takes the shortcut
    lane("stamp only", loc={a: cell((5 + 3 * a) % M, (2 + 5 * a) % M) for a in range(A)})
    lane("dense", planes=torch.rand(4, M, M, generator=g) - 0.3, loc={a: cell(a % M, (M - 1 - a) % M) for a in range(A)},
         pc={a: cell((M - 1 - a) % M, a % M) for a in range(A)})
    sparse = (torch.rand(4, M, M, generator=g) - 0.3) * (torch.rand(4, M, M, generator=g) < 0.02)
    lane("shared cell", planes=sparse, loc={0: cell(M // 2, M // 3), A - 1: cell(M // 2, M // 3)}, pc={0: cell(1, 1)})
    one = torch.zeros(4, M, M)
    one[2, E, E] = 0.37
    lane("corner nonzero", planes=one)
    one = torch.zeros(4, M, M)
    one[3, E, E] = -0.0
    lane("corner -0.0", planes=one)
    if M > 29:
        # on the first row / column of the second tile's window, and one pixel outside it
        lane("first row", loc={0: cell(29, 31)}); lane("above first row", loc={0: cell(28, 31)})
        lane("first column", pc={A - 1: cell(31, 29)}); lane("left of first column", pc={A - 1: cell(31, 28)})
        lane("corner stamp", loc={0: cell(29, 29)}, pc={0: cell(28, 28)})
    if M > 35:
        # on the last row / column of the first tile's window (pixel 34), and one pixel outside it
        lane("last row", loc={0: cell(34, 10)}); lane("below last row", loc={0: cell(35, 10)})
        lane("last column", pc={A - 1: cell(10, 34)}); lane("right of last column", pc={A - 1: cell(10, 35)})
    return maps[:N].contiguous(), cells[:N].contiguous(), pcells[:N].contiguous(), tags[:N]


def _check_team_trunk(M, N, A, maps, cells, pcells):
    D.check_team_trunk(D.SIZED, "actor", D.actors(A, M, 100 * N + A + M), maps, cells, pcells)


TRUNK_CASES = [(M, N, A) for M in (8, 31, 33, 35) for N in (1, 2, 5) for A in (1, 3, 8)]


@pytest.mark.parametrize("M,N,A", TRUNK_CASES, ids=[f"M{m}-N{n}-A{a}" for m, n, a in TRUNK_CASES])
def test_sized_team_trunk_equals_one_trunk_launch_per_agent_bit_for_bit(M, N, A):
    maps, cells, pcells, tags = _lanes(M, A, N, seed=31 * N + A + M)
    sc = S.shortcut_units(maps, cells, pcells)
    assert tags[0] == "nothing" and bool(sc[0].all())
    if N >= 2:
        assert tags[1] == "stamp only" and float(maps[1].abs().max()) == 0.0 and bool((cells[1] >= 0).all()) and not bool(sc[1, :, 0, 0].any())
    if N >= 5:
        assert tags[2] == "dense" and not bool(sc[2].any()) and tags[4] == "corner nonzero"
        assert bool((cells[3, 0] == cells[3, A - 1]) & (cells[3, 0] >= 0))
    _check_team_trunk(M, N, A, maps, cells, pcells)


def test_sized_team_trunk_at_147_with_stamps_on_and_beside_the_window_edges():
    """N = 2, A = 3 at the walls-off size (5 x 5 tiles): lane 0 holds nothing but the agents' stamps, on the last row / column of tile
    (0, 0)'s window (pixel 34) and one past it, and on the first row of tile (1, .)'s (29) and one before it; lane 1 is dense."""
    M, A = 147, 3
    cell = lambda r, c: r * M + c
    g = torch.Generator().manual_seed(147)
    maps = torch.zeros(2, 4, M, M)
    maps[1] = torch.rand(4, M, M, generator=g) - 0.3
    cells = torch.tensor([[cell(34, 10), cell(10, 34), cell(29, 100)], [cell(3, 3), cell(146, 146), cell(3, 3)]])
    pcells = torch.tensor([[cell(35, 10), cell(10, 35), cell(28, 100)], [cell(70, 70), -1, cell(0, 146)]])
    sc = S.shortcut_units(maps, cells, pcells)
    assert sc.shape == (2, 3, 5, 5) and not bool(sc[1].any())
    assert not sc[0, 0, 0, 0] and not sc[0, 0, 1, 0] and sc[0, 0, 0, 1]                # (34, 10) in tile (0, 0)'s window, (35, 10) in (1, 0)'s only
    assert not sc[0, 1, 0, 0] and not sc[0, 1, 0, 1] and sc[0, 1, 1, 0]
    assert not sc[0, 2, 0, 3] and not sc[0, 2, 1, 3] and sc[0, 2, 0, 2] and sc[0, 2, 2, 3]       # column 100: tile column 3 (93..130) alone
    assert 0 < int(sc[0].sum()) < sc[0].numel()
    _check_team_trunk(M, 2, A, maps, cells, pcells)


def test_sized_team_trunk_with_more_units_than_the_resident_grid():
    """side 35, N = 130, A = 3: 130 x 4 x 3 = 1560 units.  The grid is the resident workgroups, 3 per CU (168 VGPRs; 34 KB of LDS would
    allow 4) = 768 on 256 CUs: the stride loop runs two full trips and a ragged third.  Every shortcut case of _lanes is among the
    lanes."""
    M, N, A = 35, 130, 3
    units = N * 4 * A
    assert all(units % grid for grid in (256, 512, 768, 1024, 1280)) and units > 1500
    maps, cells, pcells, tags = _lanes(M, A, N, seed=9)
    sc = S.shortcut_units(maps, cells, pcells)
    i = {t: k for k, t in enumerate(tags)}
    assert bool(sc[i["nothing"]].all()) and bool(sc[i["corner -0.0"]].all()) and not bool(sc[i["corner nonzero"]].any())
    assert not bool(sc[i["dense"]].any())
    assert float(maps[i["stamp only"]].abs().max()) == 0.0 and 0 < int(sc[i["stamp only"]].sum()) < sc[0].numel()
    assert not bool(sc[i["first row"], 0].any()) and sc[i["above first row"], 0].tolist() == [[False, False], [True, True]]
    assert not bool(sc[i["first column"], A - 1].any()) and sc[i["left of first column"], A - 1].tolist() == [[False, True], [False, True]]
    assert not bool(sc[i["corner stamp"], 0].any()) and bool(sc[i["corner stamp"], 1].all())
    assert bool((cells[i["shared cell"], 0] == cells[i["shared cell"], A - 1]) & (cells[i["shared cell"], 0] >= 0))
    # both paths are taken (tile (0, 0)'s window is the whole map at this side: the random lanes are dense in every unit)
    assert int(sc.sum()) >= 40 and int((~sc).sum()) >= 1000
    _check_team_trunk(M, N, A, maps, cells, pcells)


# ------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("P", sorted(S.SIDE))
def test_sized_team_head_first_layer_is_exact_on_one_hot_rows(P):
    """a2 rows that are 1.0 at one k and 0 elsewhere: y1[j] = a single term plus exact zeros, then the bias = float32(W1[j][k] + b1[j]),
    bit for bit, at the first and last float of every wave's quarter and of its tail, at the piece boundaries 31 / 32 and the lane
    halves' 15 / 16.  A dropped or doubled float at any of these edges fails here; the float64 rule below would let it pass."""
    A, flat = 2, S.flat_of(P)
    seqs = D.actors(A, S.SIDE[P], 40 + P)
    ks = S.onehot_ks(P)
    a2, u = D.onehot_rows(A, flat, ks)
    got = D.eval_head(D.SIZED, seqs, flat, a2, u, torch.ones(len(ks), dtype=torch.uint8, device="cuda"), len(ks))
    D.check_onehot_y1(got["y1"], seqs, ks, P)


@pytest.mark.parametrize("P,N,A", S.HEAD_CASES, ids=[f"P{p}-N{n}-A{a}" for p, n, a in S.HEAD_CASES])
def test_sized_team_head_matches_float64_and_so_does_the_existing_path(P, N, A):
    """the master call has 130 lanes at P = 15 and at P = 73 with 2 agents"""
    D.head_matches_float64_and_so_does_the_existing_path(D.SIZED, (P, A), N)


# ------------------------------------------------------------------------------------------------ whole runs
L_RUN = 8                                                  # walls off: 27 + 8 = 35 cells a side
RUN_SEEDS = dict(torch=41, sets=17, run=205)


def _agents(A, seed, side=35):
    """A CNN agents for side x side maps with their own predictor cells (the runner loads them into its bank)."""
    from radiation_ppo_amd.pfgru import PFGRUCell
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO
    torch.manual_seed(seed)
    agents = {i: CNNAgentPPO(id=i, map_dim=(side, side)) for i in range(A)}
    for ag in agents.values():
        ag.model = PFGRUCell().to(ag.device)
    return agents


def _sets(E, obst, seed, near=(0,)):
    """E saved environments from the environment's own spawn rules, walls off; the detectors of those in `near` are moved to 5 cm from
    the source: a step moves at most 100 cm and the terminal radius is 110 cm, so a run of them ends at the first lock-step in which an
    agent moves, whatever is drawn -- lock-step 1 for one agent; agents on one spot that propose the same cell block each other and the
    environment raises the terminal flag only for an agent that moved, so a team may need another lock-step.  The others start more
    than 8 * 100 + 110 cm away (asserted): no run of them can end within 8 steps."""
    from radiation_ppo_amd.evaluate import sample_test_environments
    sets = sample_test_environments(E, obstruction_count=obst, enforce_grid_boundaries=False, seed=seed)
    for i in range(E):
        e = list(sets[f"env_{i}"])
        if i in near:
            e[1] = e[0] + np.array([3.0, 4.0])
        else:
            assert float(np.linalg.norm(e[1] - e[0])) > L_RUN * 100 + 110, i
        sets[f"env_{i}"] = tuple(e)
    return sets


def _replay(sets, results, actions, A, R, seed, obst, team_mode, near=(0,)):
    """every lane through the oracle, walls off, with the logged joint actions: the same last step, success flag and return in run
    order; finished lanes log 8 (tests/_eval_runs.py).  The runs of the `near` environments end (at the first lock-step in which an
    agent moves), no other run ends."""
    runs = V.replay_lane_per_run(sets, actions, A, R, L_RUN, seed, obst, team_mode=team_mode, enforce_grid_boundaries=False)
    for n, (steps, found, _) in enumerate(runs):
        assert found == (n // R in near) and (found or steps == L_RUN), (n, steps, found)
    assert V.check_records(results, runs, R) == len(near) * R


@pytest.mark.parametrize("A,team_mode", [(2, "individual"), (2, "team"), (4, "individual"), (4, "team")])
def test_fused_run_replays_through_the_oracle_and_equals_the_composed_run(A, team_mode):
    """E = 4, R = 3, L = 8 (35 x 35 maps), 2 obstructions.  (a) every lane of the fused run replays through the oracle with walls off;
    the runs of environment 0 end, the others run all 8; (b) the composed form gives the same action log and the same records.  The
    BLAS first layer rounds differently from the MFMA one, so a seed could in principle put a uniform between the two paths' CDF steps;
    these seeds do not."""
    from radiation_ppo_amd.evaluate import run_test_environments_cnn_team_sized
    E, R, obst = 4, 3, 2
    sets = _sets(E, obst, RUN_SEEDS["sets"])
    agents = _agents(A, RUN_SEEDS["torch"])
    kw = dict(montecarlo_runs=R, steps_per_episode=L_RUN, team_mode=team_mode, obstruction_count=obst, enforce_grid_boundaries=False,
              seed=RUN_SEEDS["run"], return_actions=True)
    results, summary, actions = run_test_environments_cnn_team_sized(agents, sets, fused=True, **kw)
    assert len(results) == E and summary["completed_runs"] == E * R and actions.shape == (L_RUN, E * R, A) and actions.dtype == np.int8
    _replay(sets, results, actions, A, R, RUN_SEEDS["run"], obst, team_mode)
    res_c, sum_c, act_c = run_test_environments_cnn_team_sized(agents, sets, fused=False, **kw)
    assert act_c.shape == actions.shape and np.array_equal(act_c, actions)
    V.same_records(res_c, results, R)
    assert sum_c["success_rate"] == summary["success_rate"]


def test_the_scratch_bound_does_not_change_the_records():
    """132 lanes: a2_bytes = 1 gives the smallest chunk, 64 lanes, so three chunks (64, 64, 4) per lock-step; the log and the records
    equal those of the default (one chunk), in both forms."""
    from radiation_ppo_amd.evaluate import run_test_environments_cnn_team_sized
    E, R, A = 4, 33, 2
    sets = _sets(E, 2, RUN_SEEDS["sets"])
    agents = _agents(A, RUN_SEEDS["torch"])
    kw = dict(montecarlo_runs=R, steps_per_episode=L_RUN, obstruction_count=2, enforce_grid_boundaries=False, seed=RUN_SEEDS["run"],
              return_actions=True)
    results, _, actions = run_test_environments_cnn_team_sized(agents, sets, **kw)
    assert actions.shape == (L_RUN, 132, A) and (actions[0] < 8).all() and (actions[-1, :R] == 8).all() and (actions[:, R:] < 8).all()
    for fused in (True, False):
        res_s, _, act_s = run_test_environments_cnn_team_sized(agents, sets, a2_bytes=1, fused=fused, **kw)
        assert np.array_equal(act_s, actions), fused
        V.same_records(res_s, results, R)


def test_the_run_stops_on_the_device_side_count_at_the_next_sixteenth_step():
    """Every environment starts 5 cm from its source, so every lane ends at lock-step 1.  The host reads the finished-lane count every
    16 lock-steps: 16 rows, rows 1..15 idle, in both forms (steps_per_episode = 20: 47 x 47 maps)."""
    from radiation_ppo_amd.evaluate import run_test_environments_cnn_team_sized
    E, R = 3, 4
    agents = _agents(1, 11, side=47)
    V.check_stops_at_the_sixteenth(lambda sets, fused: run_test_environments_cnn_team_sized(
        agents, sets, montecarlo_runs=R, steps_per_episode=20, seed=5, enforce_grid_boundaries=False, return_actions=True, fused=fused), E, R, 1)


def test_the_runner_without_predictor_and_its_refusals():
    from radiation_ppo_amd.evaluate import run_test_environments_cnn_team_sized
    sets = _sets(2, 0, 8, near=())
    agents = _agents(2, 12)
    kw = dict(montecarlo_runs=2, steps_per_episode=L_RUN, seed=3, enforce_grid_boundaries=False)
    out = {}
    for fused in (True, False):
        results, summary, actions = run_test_environments_cnn_team_sized(agents, sets, use_predictor=False, return_actions=True, fused=fused,
                                                                         **kw)
        assert summary["completed_runs"] == 4 and actions.shape == (L_RUN, 4, 2)
        out[fused] = (actions, results)
    assert np.array_equal(out[True][0], out[False][0])
    V.same_records(out[True][1], out[False][1], 2)
    results, summary = run_test_environments_cnn_team_sized(agents, sets, **kw)                  # no log: one fixed action buffer
    assert summary["completed_runs"] == 4
    with pytest.raises(ValueError, match="run_test_environments_cnn"):
        run_test_environments_cnn_team_sized({0: agents[0], 2: agents[1]}, sets, **kw)
    with pytest.raises(ValueError, match="run_test_environments_cnn"):
        run_test_environments_cnn_team_sized(agents, sets, device="cpu", **kw)
    with pytest.raises(ValueError, match="run_test_environments_cnn"):                           # agents for 27 x 27 maps, 35 x 35 maps
        run_test_environments_cnn_team_sized(_agents(2, 12, side=27), sets, **kw)
    with pytest.raises(ValueError, match="run_test_environments_cnn"):                           # agents for 35 x 35 maps, 27 x 27 maps
        run_test_environments_cnn_team_sized(agents, sets, **dict(kw, enforce_grid_boundaries=True))


def test_evaluate_ppo_driver_loads_walls_off_agents_and_reaches_the_sized_runner(tmp_path, monkeypatch):
    """Two agents built for 35 x 35 maps are saved; evaluate_PPO with enforce_boundaries=False, steps_per_episode=8 loads each agent's
    own weights (the driver used to build every CNN agent for 27 x 27 maps: Linear(16 * 17 * 17, 32) could not be loaded) and reaches
    run_test_environments_cnn_team_sized.  With enforce_boundaries=True (and 27 x 27 agents) it still reaches
    run_test_environments_cnn_team."""
    joblib = pytest.importorskip("joblib")
    from radiation_ppo_amd import evaluate as ev_mod
    from radiation_ppo_amd.evaluate import evaluate_PPO, sample_test_environments
    os.makedirs(tmp_path / "sets")
    for walls in (False, True):
        sets = sample_test_environments(4, obstruction_count=1, enforce_grid_boundaries=walls, seed=3)
        joblib.dump(sets, str(tmp_path / "sets" / f"test_env_dict_obs1_{'low' if walls else 'med'}_v4"))
    seen = []
    for name in ("run_test_environments_cnn_team_sized", "run_test_environments_cnn_team", "run_test_environments_cnn"):
        real = getattr(ev_mod, name)
        monkeypatch.setattr(ev_mod, name, lambda agents, *a, _n=name, _r=real, **k: (seen.append((_n, agents, k)), _r(agents, *a, **k))[1])
    for walls, side, runner in ((False, 35, "run_test_environments_cnn_team_sized"), (True, 27, "run_test_environments_cnn_team")):
        saved = {}
        for i, ag in _agents(2, 21 + side, side=side).items():
            ag.save(str(tmp_path / f"models{side}" / f"{i}_agent"))
            saved[i] = {k: v.clone() for k, v in ag.pi.state_dict().items()}
        assert saved[0]["actor.6.weight"].shape == (32, 16 * (side // 2) ** 2)
        assert not torch.equal(saved[0]["actor.6.weight"], saved[1]["actor.6.weight"])   # the two agents are told apart by their weights
        kw = dict(test_env_path=str(tmp_path / "sets"), obstruction_count=1, snr="low" if walls else "med", episodes=3, montecarlo_runs=2,
                  model_path=str(tmp_path / f"models{side}"), actor_critic_architecture="cnn", number_of_agents=2, steps_per_episode=L_RUN,
                  enforce_boundaries=walls, team_mode="team", seed=1)
        del seen[:]
        results, summary = evaluate_PPO(dict(kw)).evaluate()
        assert len(results) == 3 and summary["completed_runs"] == 6 and 0.0 <= summary["success_rate"] <= 1.0
        (kind, agents, k), = seen
        assert kind == runner and sorted(agents) == [0, 1] and k["team_mode"] == "team" and k["enforce_grid_boundaries"] == walls
        for i in range(2):
            assert tuple(agents[i].map_dim) == (side, side)
            got = agents[i].pi.state_dict()
            assert set(got) == set(saved[i]) and all(torch.equal(got[name].cpu(), saved[i][name].cpu()) for name in got), i
        assert not torch.equal(agents[1].pi.actor[6].weight.cpu(), saved[0]["actor.6.weight"].cpu())
