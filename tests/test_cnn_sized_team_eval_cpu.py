"""rs_cnn_sized_team_infer and rs_cnn_sized_team_eval_head without a GPU (their signatures, rs_cnn_conv_params' layout and their
export: tests/test_abi_cpu.py): every argument check returns before any HIP call (this machine has no device: a launch would have come back as
RS_ERR_HIP), and the self-check of the float64 rule of tests/_cnn_sized_team_ref.py at every depth the GPU test uses: the float32 torch
composition passes it, a y1 moved by twice its allowance fails it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_sized_team_ref as S  # noqa: E402

from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG, RS_ERR_UNSUPPORTED, RS_OK  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


def _convs(n=None, spoil=None):
    from radiation_ppo_amd import _lib
    n = n or _lib.RS_MAX_AGENTS
    rows = [[0x10000 * (i + 1) + 0x100 * k for k in range(4)] for i in range(n)]
    if spoil is not None:
        rows[spoil[0]][spoil[1]] = None
    return (_lib.RsCnnConvParams * n)(*[_lib.RsCnnConvParams(*r) for r in rows])


# a valid call over fake (never dereferenced) addresses, then one argument spoilt per case
TRUNK_GOOD = dict(maps=0x1000, cells=0x2000, pcells=0x3000, num_agents=2, num_samples=64, map_side=147, convs=True, a2=0x5000)
TRUNK_CASES = ([(f"{k} NULL", {k: None}, RS_ERR_INVALID_ARG) for k in ("maps", "cells", "pcells", "a2")]
               + [("convs NULL", dict(convs=False), RS_ERR_INVALID_ARG), ("no agent", dict(num_agents=0), RS_ERR_INVALID_ARG),
                  ("negative agents", dict(num_agents=-1), RS_ERR_INVALID_ARG), ("nine agents", dict(num_agents=9), RS_ERR_INVALID_ARG),
                  ("negative samples", dict(num_samples=-1), RS_ERR_INVALID_ARG),
                  ("no sample, a2 NULL", dict(num_samples=0, a2=None), RS_ERR_INVALID_ARG),
                  ("side 7", dict(map_side=7), RS_ERR_UNSUPPORTED), ("side 257", dict(map_side=257), RS_ERR_UNSUPPORTED),
                  ("side 7, no sample", dict(map_side=7, num_samples=0), RS_ERR_UNSUPPORTED),
                  ("side 257, negative samples", dict(map_side=257, num_samples=-1), RS_ERR_INVALID_ARG)])


@pytest.mark.parametrize("name,spoil,want", TRUNK_CASES, ids=[c[0] for c in TRUNK_CASES])
def test_sized_team_trunk_checks_its_arguments_before_any_hip_call(lib, name, spoil, want):
    a = dict(TRUNK_GOOD, **spoil)
    rc = lib.rs_cnn_sized_team_infer(a["maps"], a["cells"], a["pcells"], a["num_agents"], a["num_samples"], a["map_side"],
                                     _convs() if a["convs"] else None, a["a2"], None)
    assert rc == want, (name, rc)


@pytest.mark.parametrize("agent,field", [(0, 0), (1, 3), (1, 1)])
def test_sized_team_trunk_refuses_a_null_pointer_inside_a_conv(lib, agent, field):
    a = TRUNK_GOOD
    call = lambda convs: lib.rs_cnn_sized_team_infer(a["maps"], a["cells"], a["pcells"], 2, 64, 147, convs, a["a2"], None)
    assert call(_convs(2, spoil=(agent, field))) == RS_ERR_INVALID_ARG
    # behind the team's agents nothing is looked at (no sample: the call returns RS_OK before a launch)
    assert lib.rs_cnn_sized_team_infer(a["maps"], a["cells"], a["pcells"], 2, 0, 147, _convs(3, spoil=(2, field)), a["a2"], None) == RS_OK


@pytest.mark.parametrize("side", [8, 35, 147, 256])
def test_sized_team_trunk_with_no_sample_is_ok_and_launches_nothing(lib, side):
    a = TRUNK_GOOD
    assert lib.rs_cnn_sized_team_infer(a["maps"], a["cells"], a["pcells"], a["num_agents"], 0, side, _convs(), a["a2"], None) == RS_OK


HEAD_GOOD = dict(heads=True, num_agents=2, flat=85264, a2=0x1000, u=0x2000, alive=0x3000, act8=0x4000, act=0x5000, logp=0x6000, y1_out=0x7000,
                 num_envs=64)
HEAD_CASES = ([("heads NULL", dict(heads=False))] + [(f"{k} NULL", {k: None}) for k in ("a2", "u", "alive", "act8")]
              + [("no agent", dict(num_agents=0)), ("negative agents", dict(num_agents=-1)), ("nine agents", dict(num_agents=9)),
                 ("no env", dict(num_envs=0)), ("negative envs", dict(num_envs=-5)),
                 ("optional outputs NULL, a2 NULL", dict(act=None, logp=None, y1_out=None, a2=None))]
              # flat must be 16 p p, p = 4..128: 2704 + 16 lies between p = 13 and 14, 144 is p = 3, 16 * 129^2 is past the range
              + [(f"flat {f}", dict(flat=f)) for f in (2704 + 16, 2704 + 4, 2705, 0, -2704, 16, 144, 255, 16 * 129 * 129, 85264 + 16)])


def _heads(n=None, spoil=None):
    from radiation_ppo_amd import _lib
    n = n or _lib.RS_MAX_AGENTS
    rows = [[0x10000 * (i + 1) + 0x100 * k for k in range(6)] for i in range(n)]
    if spoil is not None:
        rows[spoil[0]][spoil[1]] = None
    return (_lib.RsCnnHeadParams * n)(*[_lib.RsCnnHeadParams(*r) for r in rows])


@pytest.mark.parametrize("name,spoil", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_sized_team_head_refuses_invalid_arguments_before_any_hip_call(lib, name, spoil):
    a = dict(HEAD_GOOD, **spoil)
    rc = lib.rs_cnn_sized_team_eval_head(_heads() if a["heads"] else None, a["num_agents"], a["flat"], a["a2"], a["u"], a["alive"], a["act8"],
                                         a["act"], a["logp"], a["y1_out"], a["num_envs"], None)
    assert rc == RS_ERR_INVALID_ARG, (name, rc)


def test_sized_team_head_refuses_a_null_pointer_inside_a_head(lib):
    a = HEAD_GOOD
    for field in range(6):
        rc = lib.rs_cnn_sized_team_eval_head(_heads(2, spoil=(1, field)), 2, 2704, a["a2"], a["u"], a["alive"], a["act8"], None, None, None, 64,
                                             None)
        assert rc == RS_ERR_INVALID_ARG, field


# ------------------------------------------------------------------------------------------------ the rule's self-check
CPU_LANES = 66


@pytest.mark.parametrize("P", sorted(S.SIDE))
def test_float32_torch_composition_passes_the_rule_and_a_moved_y1_fails_it(P):
    """66 lanes of 2 % dense maps per depth, 3 agents: the float32 composition passes (its worst ratios are printed), every agent draws
    at least 3 distinct actions, and y1 moved by twice its allowance on one element fails."""
    A = 3
    from radiation_ppo_amd.maps import CNNActor
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(900 + P)
        actors = [CNNActor(map_dim=(S.SIDE[P], S.SIDE[P])) for _ in range(A)]
    with torch.no_grad():
        for ac in actors:
            ac.actor[0].bias.uniform_(-0.05, 0.15)
            ac.actor[3].bias.uniform_(-0.1, 0.1)
            for i in (6, 8, 10):
                for p in ac.actor[i].parameters():
                    p.mul_(S.SCALE)
    t = S.Team()
    t.A, t.actors = A, actors
    t.maps, t.cells, t.pcells = S.random_maps(CPU_LANES, A, S.SIDE[P], seed=77 + P)
    g = torch.Generator().manual_seed(5 + P)
    t.u = torch.rand(CPU_LANES, A, generator=g)
    t.alive = (torch.rand(CPU_LANES, generator=g) < 0.6).to(torch.uint8)
    a2 = S.trunk_cpu(t)
    assert a2.shape == (A, CPU_LANES, S.flat_of(P)) and float(a2.min()) >= 0.0
    alive = S.alive_for(t, CPU_LANES)
    for a in range(A):
        ref = S.reference(actors[a].actor, a2[a], t.u[:, a])
        assert S.distinct_actions(ref) >= 3, (P, a)
        y1, act, logp, act8 = S.torch32(actors[a].actor, a2[a], t.u[:, a], alive)
        q = S.ratios(ref, t.u[:, a], alive, act, logp, act8, y1=y1)
        print(f"float32 torch P{P} flat {S.flat_of(P)} agent {a} | " + " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in q.items()))
        assert S.passes(q), (P, a, q)
        moved = y1.double().clone()
        moved[CPU_LANES // 2, 7] += 2.0 * ref.y1_allow[CPU_LANES // 2, 7]
        qm = S.ratios(ref, t.u[:, a], alive, act, logp, act8, y1=moved)
        assert 1.0 < qm["y1"] < 3.1 and not S.passes(qm), (P, a, qm)


def test_onehot_positions_cover_quarters_tails_and_piece_boundaries():
    for P in S.SIDE:
        kw, flat = 4 * P * P, S.flat_of(P)
        ks = S.onehot_ks(P)
        assert ks[0] == 0 and ks[-1] == flat - 1 and all(0 <= k < flat for k in ks)
        for w in range(4):
            assert {w * kw, w * kw + kw - 1, w * kw + 31, w * kw + 32} <= set(ks)
            if kw % 32:
                assert w * kw + kw // 32 * 32 in ks
    assert [4 * P * P % 32 for P in sorted(S.SIDE)] == [0, 4, 16, 4, 0, 4] and 4 * 4 * 4 // 32 == 2 and 4 * 5 * 5 // 32 == 3


def test_shortcut_model_on_hand_made_maps():
    """side 35: tile (0, 0)'s window is the whole map, the others' windows start at pixel 29"""
    M = 35
    maps = torch.zeros(5, 4, M, M)
    cells = torch.full((5, 1), -1)
    pcells = torch.full((5, 1), -1)
    cells[1, 0] = 28 * M + 31                        # one pixel above tile row 1's windows
    cells[2, 0] = 29 * M + 31                        # on their first row
    maps[3, 2, 29, 29] = -0.0
    maps[4, 2, 29, 29] = float("nan")
    sc = S.shortcut_units(maps, cells, pcells)[:, 0]
    assert sc[0].all() and sc[3].all() and not sc[4].any()
    assert sc[1].tolist() == [[False, False], [True, True]] and sc[2].tolist() == [[False, False], [False, False]]
