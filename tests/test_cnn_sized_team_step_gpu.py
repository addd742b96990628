"""The walls-off RAD-TEAM (CNN) training round: rs_cnn_sized_team_step_head (Linear(flat, 32) split over k across workgroups, a
fixed-order second stage), rs_cnn_sized_team_critic_infer and the collector that issues them (CNNCollector.use_sized_team_round).

First layer, exact: a2 rows that are one-hot at k must give y1 == float32(W1[:, k] + b1) bit for bit on actor and critic rows, at the k
computed from rs_cnn_sized_team_head_slice_floats() (_cnn_sized_team_ref.onehot_ks_sliced) -- in the first, a middle and the last slice
the first and last float of every wave quarter, the piece boundary 31 / 32, the lane halves' 15 / 16 (7 / 8 of a 16-float tail), the
first and last float of a tail, and the floats on either side of every slice boundary -- at p = 4 (less than one slice), 5, 15, the
first p whose depth is a whole number of slices, and 73 (85 264).

Float64: tests/_cnn_team_ref.reference with K1 at the case's depth on the actor rows (y1, log-probability, the draws equal except
within DRAW_CAP), the same allowance for the one output on the critic rows (_cnn_team_ref.value_ratios at that K1); p = 15
with A = 3, C in {1, 3}, N in {1, 63, 64, 65, 130} and p = 73 with (N, A) in {(64, 8), (33, 2), (130, 2)}, both critic modes.  The float32
torch composition on the same inputs is held to the same rule by tests/test_cnn_sized_team_eval_cpu.py.  Every worst ratio is printed;
profiles/cnn_sized_team_step_float64_ratios.txt keeps a copy.

Scratch discipline (the scratch is NaN before every call of this file and guarded on both sides: every output finite), the bootstrap
round, sharding (N = 130 against 65 twice), the critic team trunk against rs_cnn_sized_infer(agent = -1) per critic, and the collector on
31 x 31 maps: team round on against off, every stored row against the modules, graph against eager, two half collectors against one,
the fall-back conditions, and one walls-off train_PPO('cnn') epoch.

The guarded calls (the scratch among them), the master and the bodies this file has in common with tests/test_cnn_team_step_gpu.py are
tests/_cnn_team_drive.py's, run here with SIZED; what is written out below is this family's own."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_sized_team_ref as S  # noqa: E402
import _cnn_team_drive as D  # noqa: E402
import _cnn_team_ref as T  # noqa: E402
from _cnn_team_drive import SIZED as F, bits as _bits, is_sentinel as _is_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib_():
    from radiation_ppo_amd import _lib
    return _lib, _lib.load()


def _side(P):
    return S.SIDE.get(P, 2 * P + 1)


def _call(actors, critics, flat, a2a, a2c, u, N, A, **kw):
    return D.step_head(F, actors, critics, flat, a2a, a2c, u, N, A, **kw)


# ------------------------------------------------------------------------------------------------ the first layer, exact
def _whole_p(sl):
    """the first p in 4..128 whose depth 16 p p is a whole number of slices, or None"""
    return next((p for p in range(4, 129) if (16 * p * p) % sl == 0), None)


def _onehot_depths():
    return [4, 5, 15, "whole", 73]


@pytest.mark.parametrize("P", _onehot_depths())
def test_first_layer_is_exact_on_one_hot_rows(P):
    _lib, lib = _lib_()
    sl = lib.rs_cnn_sized_team_head_slice_floats()
    if P == "whole":
        P = _whole_p(sl)
        if P is None:
            return                                          # no depth is a whole number of slices at this slice length
        assert (16 * P * P) % sl == 0
    A, flat, M = 2, S.flat_of(P), _side(P)
    from radiation_ppo_amd.maps import CNNActor
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(50 + P)
        seqs = [CNNActor(map_dim=(M, M)).actor.cuda() for _ in range(A)]
    crit = [c.critic.cuda() for c in D.critics(A, 60 + P, M)]
    assert seqs[0][6].weight.shape == (32, flat) and crit[0][6].weight.shape == (32, flat)
    ks = S.onehot_ks_sliced(flat, sl)
    if flat > sl:
        assert {sl - 1, sl, sl // 4 - 1, sl // 4, 15, 16, 31, 32} <= set(ks)
    a2, u = D.onehot_rows(A, flat, ks)
    got = _call(seqs, crit, flat, a2, a2, u, len(ks), A)
    assert got["rc"] == 0
    D.check_onehot_y1(got["y1"], seqs + crit, ks, P)


# ------------------------------------------------------------------------------------------------ float64
F64_CASES = [(15, N, 3) for N in (1, 63, 64, 65, 130)] + [(73, 64, 8), (73, 33, 2), (73, 130, 2)]


@pytest.mark.parametrize("P,N,A", F64_CASES, ids=[f"P{p}-N{n}-A{a}" for p, n, a in F64_CASES])
def test_step_round_holds_to_float64_in_both_critic_modes(P, N, A):
    m = D.master(F, (P, A), critics_too=True)
    t = m["t"]
    a2a, a2c, u = m["a2a"][:, :N].contiguous(), m["a2c"][:, :N].contiguous(), m["u"][:N].contiguous()
    alive = torch.ones(N, dtype=torch.uint8)
    refs = [S.reference(t.actors[a].actor, a2a[a], u[:, a]) for a in range(A)]
    crit_ref = {}
    worst = dict(y1=0.0, logp=0.0, differing=0, unexcused=0, act8=0, critic_y1=0.0, value=0.0)
    fails, first = [], None
    for nc in (1, A):
        got = _call(m["seqs"], m["crit"][:nc], t.flat, a2a, a2c[:nc].contiguous(), u, N, A)
        assert got["rc"] == 0
        assert bool((got["act"] >= 0).all()) and bool((got["act"] <= 7).all()) and torch.equal(got["act8"].long(), got["act"].t())
        assert _is_sentinel(got["f"][:, 2])                                  # the step round leaves the bootstrap slot alone
        for a in range(A):
            q = S.ratios(refs[a], u[:, a], alive, got["act"][a], got["f"][a, 0], got["act8"][:, a], y1=got["y1"][a])
            for k in q:
                worst[k] = max(worst[k], q[k])
            if not S.passes(q):
                fails.append((nc, a, q))
        if first is None:
            first = got
        else:                                                                # the actor rows do not depend on the critic mode
            assert torch.equal(got["act"], first["act"]) and torch.equal(_bits(got["f"][:, 0]), _bits(first["f"][:, 0]))
            assert torch.equal(_bits(got["y1"][:A]), _bits(first["y1"][:A]))
        for c in range(nc):
            rows = range(A) if nc == 1 else (c,)
            for a in rows:                                                   # a global critic's value in every agent's row
                assert torch.equal(_bits(got["f"][a, 1]), _bits(got["f"][rows[0], 1])), (nc, c, a)
            if c in crit_ref:                                                # critic 0 in the second mode: the same bits as in the first
                assert torch.equal(_bits(got["f"][c, 1]), _bits(crit_ref[c][0])) and torch.equal(_bits(got["y1"][A + c]), _bits(crit_ref[c][1]))
                continue
            crit_ref[c] = (got["f"][rows[0], 1].clone(), got["y1"][A + c].clone())
            qy, qv = T.value_ratios(m["cpu_critics"][c].critic, a2c[c], got["f"][rows[0], 1], got["y1"][A + c], S.k1(t.flat))
            worst["critic_y1"], worst["value"] = max(worst["critic_y1"], qy), max(worst["value"], qv)
        if nc == A and A > 1:
            assert not torch.equal(got["f"][0, 1], got["f"][A - 1, 1])       # every critic its own value
    line = f"cnn sized team step {F.case(t, N)} | " + D.fmt(worst)
    print(line)
    assert not fails, (line, fails)
    assert T.value_passes(worst["critic_y1"], worst["value"]), line
    if N >= 63:
        assert all(S.distinct_actions(r) >= 3 for r in refs)                 # visibly non-uniform policies that still draw several actions


# ------------------------------------------------------------------------------------------------ scratch discipline, sharding
def test_bootstrap_round_writes_slot_two_under_the_mask_and_nothing_else():
    def boot_y1(got, step, on, A):                          # the k-split kernel masks per lane
        assert _is_sentinel(got["y1"][A:][:, ~on]) and torch.equal(_bits(got["y1"][A:][:, on]), _bits(step["y1"][A:][:, on]))

    def masked_y1(got, on):
        assert _is_sentinel(got["y1"][:, ~on])

    P, A, N = 15, 3, 130
    m, step = D.bootstrap_round(F, (P, A), boot_y1, masked_y1)
    flat, a2a, a2c, u = m["t"].flat, m["a2a"], m["a2c"], m["u"]
    # refusals that need no launch: a bootstrap round without a mask, a scratch one float short, a depth that is no 16 p p
    _lib, lib = _lib_()
    scr = torch.empty(lib.rs_cnn_sized_team_head_scratch_floats(flat, 2 * A, N), device="cuda")
    f = step[A]["f"].clone()
    ap, cp = D.head_params(m["seqs"]), D.head_params(m["crit"])
    assert D.call("rs_cnn_sized_team_step_head", None, A, cp, A, flat, None, a2c, None, None, f, None, None, None, scr, scr.numel(), N) == 1
    for bad_flat, floats in ((flat, scr.numel() - 1), (flat + 16, scr.numel())):
        assert D.call("rs_cnn_sized_team_step_head", ap, A, cp, A, bad_flat, a2a, a2c, u, step[A]["act"], f, step[A]["act8"], None, None, scr,
                      floats, N) == 1
    assert torch.equal(_bits(f), _bits(step[A]["f"]))


def test_results_do_not_depend_on_how_the_envs_are_sharded():
    """N = 130 in one call against the same lanes as two calls of 65, each through a scratch of its own size: equal bits in every output;
    and a scratch larger than needed changes nothing."""
    m, whole = D.sharding(F, (15, 3))
    big = _call(m["seqs"], m["crit"], m["t"].flat, m["a2a"], m["a2c"], m["u"], 130, 3, rows_of_scratch=16)
    assert torch.equal(big["act"], whole["act"]) and torch.equal(_bits(big["f"][:, :2]), _bits(whole["f"][:, :2]))


# ------------------------------------------------------------------------------------------------ the critic team trunk
CRITIC_TRUNK_CASES = [(M, N, nc) for M in (8, 31, 33, 35) for N in (1, 3) for nc in (1, 3, 8)] + [(147, 1, nc) for nc in (1, 3, 8)]


def _trunk_maps(M, N):
    """random_maps' planes, sparse enough at 147 that some tiles' windows are empty; lane 1 of three holds nothing at all"""
    maps = S.random_maps(N, 2, M, seed=17 * N + M, density=0.0003 if M == 147 else 0.02)[0]
    if N > 1:
        maps[1] = 0.0
    return maps


def test_critic_team_trunk_cases_take_the_shortcut_and_the_full_path():
    none = lambda n: torch.full((n, 1), -1)
    for M, N in ((147, 1), (35, 3), (8, 3)):
        sc = S.shortcut_units(_trunk_maps(M, N), none(N), none(N))
        assert bool(sc.any()) and not bool(sc.all()), (M, N)


@pytest.mark.parametrize("M,N,nc", CRITIC_TRUNK_CASES, ids=[f"M{m}-N{n}-C{c}" for m, n, c in CRITIC_TRUNK_CASES])
def test_critic_team_trunk_equals_one_trunk_launch_per_critic_bit_for_bit(M, N, nc):
    crit = [c.critic.cuda() for c in D.critics(nc, 100 * N + nc + M, M)]
    D.check_team_trunk(F, "critic", crit, _trunk_maps(M, N))


# ------------------------------------------------------------------------------------------------ the collector, walls off
CN, CA, CT, CL = 64, 3, 8, 4                                # 4-step episodes: 31 x 31 maps
FLAG = "sized_team_round"


def _collector(team, **kw):
    col, agents = D.collector(team, FLAG, False, CT, CL, **kw)
    assert tuple(col.maps.map_dimensions) == (31, 31)
    return col, agents


@pytest.mark.parametrize("team", [True, False], ids=["global-critic", "own-critics"])
def test_collector_sized_team_round_against_the_per_agent_round_and_the_modules(team):
    cf, cm = D.collector_round_against_the_per_agent_round_and_the_modules(_collector, FLAG, team, CT, CA)
    assert not cf.use_team_round and not cm.use_team_round
    assert getattr(cf, "_sz_scratch", None) is not None and cf._sz_a2_cri.shape[0] == (1 if team else CA)
    assert getattr(cm, "_sz_scratch", None) is None


@pytest.mark.parametrize("team", [True, False], ids=["global-critic", "own-critics"])
def test_collector_sized_team_round_graph_equals_eager_and_two_halves_equal_the_whole(team):
    D.collector_graph_equals_eager_and_two_halves_equal_the_whole(_collector, FLAG, team, CN)


def test_collector_falls_back_to_the_per_agent_round():
    def finite(col, cols):
        col.collect()
        assert col.env.error_flags() == 0 and getattr(col, "_sz_scratch", None) is None      # the sized team round never ran
        b = col.buf
        assert int(b.act.min()) >= 0 and int(b.act.max()) <= 7
        for k in ("logp", "val", "last_val", "rew"):
            assert bool(torch.isfinite(getattr(b, k)[:, :, cols]).all()), k
    col, _ = _collector(True, N=8, on=False)
    assert col.use_heads and not col.use_sized_team_round and not col.use_team_round
    finite(col, [0, 1, 2])
    col, _ = _collector(True, N=8)
    assert col.use_sized_team_round
    col.heads = False
    assert not col.use_heads and not col.use_sized_team_round
    finite(col, [0, 1, 2])
    col, _ = _collector(True, N=8, mixed=True)                          # agents 0 and 1 share a critic, agent 2 has its own
    assert col.use_heads and not col.use_sized_team_round
    finite(col, [0, 1, 2])
    col, _ = _collector(False, N=8, ids=(0, 2))                         # the ids are not 0..A-1 (agent 1 has no policy: it stays put)
    assert col.use_heads and not col.use_sized_team_round
    col._act8.zero_()
    finite(col, [0, 2])


def test_train_ppo_cnn_runs_a_walls_off_epoch_with_the_sized_team_round_on():
    col = D.train_ppo_cnn_one_epoch(walls=False).collector
    assert tuple(col.maps.map_dimensions) == (35, 35) and col.use_sized_team_round and not col.use_team_round
    A, flat = 2, 16 * 17 * 17
    assert col._sz_a2_act.shape == (A, 16, flat) and col._sz_a2_cri.shape == (1, 16, flat)                # the sized team round ran
    _lib, lib = _lib_()
    assert col._sz_scratch.numel() == lib.rs_cnn_sized_team_head_scratch_floats(flat, A + 1, 16) > 0 and getattr(col, "_cv_act", None) is not None
