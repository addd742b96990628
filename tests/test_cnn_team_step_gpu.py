"""The RAD-TEAM (CNN) training round in three launches: rs_cnn_team_step_head, rs_cnn_team_critic_trunk_infer and the collector that
issues them (CNNCollector.use_team_round).

Actor rows: act, slot 0 (logp) and y1 equal rs_cnn_team_eval_head's (alive all 1) bit for bit and act8 is the drawn action, at the cases
of tests/_cnn_team_ref.py -- N = 1, 31, 32, 33, 63, 64, 65, 130 with 3 agents and (64, 8): the 32-image MFMA tile, the 64-image workgroup,
ragged tiles -- on its maps and teams.  So no draw can differ from the float64 draw that did not differ for the evaluation head, whose
own test holds it to DRAW_CAP.

Critic rows: the first layer exact on one-hot a2 rows at the edges of the k-quarters, pieces, lane halves and the 4-float tail; the value
(slot 1) equal to rs_cnn_head(out_dim = 1) on the kernel's own y1 bit for bit, and within the float64 rule of tests/_f64_ref.py's heads
(HEAD_K2, HEAD_K3) with the first layer's K1 term of tests/_cnn_team_ref.py -- the allowance _cnn_team_ref.reference gives a logit, here
for the one output (_cnn_team_ref.value_ratios).  The worst ratios are printed; profiles/cnn_team_step_float64_ratios.txt keeps a copy.

Both critic modes, the bootstrap round (slot 2 under a mask, nothing else touched, an all-masked tile and an all-zero mask), sharding
(N = 130 against 65 twice), the critic team trunk against rs_cnn_trunk_infer(agent = -1) per critic, and the collector: team round on
against off, every stored row against the modules, graph against eager, two half collectors against one, the fall-back conditions, and
one train_PPO('cnn') epoch.

The guarded calls, the master and the bodies this file has in common with tests/test_cnn_sized_team_step_gpu.py are
tests/_cnn_team_drive.py's, run here with FAMILY27; what is written out below is this family's own."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_sized_team_ref as S  # noqa: E402
import _cnn_team_drive as D  # noqa: E402
import _cnn_team_ref as T  # noqa: E402
from _cnn_team_drive import FAMILY27 as F, bits as _bits, is_sentinel as _is_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu
FLAT = T.FLAT


def _call(actors, critics, a2a, a2c, u, N, A, **kw):
    return D.step_head(F, actors, critics, FLAT, a2a, a2c, u, N, A, **kw)


def _value_by_rs_cnn_head(s, y1, N):
    v = torch.full((N,), D.SENTINEL, device="cuda")
    D.run("rs_cnn_head", y1.contiguous(), s[8].weight, s[8].bias, s[10].weight, s[10].bias, 1, None, 1, None, None, None, 1, v, 1, 0, None, N)
    return v


@pytest.mark.parametrize("N,A", T.CASES, ids=[f"N{n}-A{a}" for n, a in T.CASES])
def test_step_round_actor_rows_are_the_evaluation_heads_bits_and_critic_rows_hold_to_float64(N, A):
    m = D.master(F, A, critics_too=True)
    a2a, a2c, u = m["a2a"][:, :N].contiguous(), m["a2c"][:, :N].contiguous(), m["u"][:N].contiguous()
    ev = D.eval_head(F, m["seqs"], FLAT, a2a, u, torch.ones(N, dtype=torch.uint8, device="cuda"), N)
    assert int(torch.unique(ev["act"]).numel()) >= (3 if N >= 31 else 1)
    worst_y1 = worst_v = 0.0
    for nc in (1, A):
        got = _call(m["seqs"], m["crit"][:nc], a2a, a2c[:nc].contiguous(), u, N, A)
        assert got["rc"] == 0
        # ---- actor rows
        assert torch.equal(got["act"], ev["act"]) and torch.equal(_bits(got["f"][:, 0]), _bits(ev["logp"])), (N, A, nc)
        assert torch.equal(_bits(got["y1"][:A]), _bits(ev["y1"]))
        assert torch.equal(got["act8"].long(), got["act"].t()) and torch.equal(got["act8"], ev["act8"])
        assert _is_sentinel(got["f"][:, 2])                                  # the step round leaves the bootstrap slot alone
        # ---- critic rows
        for c in range(nc):
            y1 = got["y1"][A + c]
            want = _value_by_rs_cnn_head(m["crit"][c], y1, N)
            rows = range(A) if nc == 1 else (c,)
            for a in rows:                                                   # a global critic's value in every agent's row
                assert torch.equal(_bits(got["f"][a, 1]), _bits(want)), (N, A, nc, c, a)
            qy, qv = T.value_ratios(m["cpu_critics"][c].critic, a2c[c], got["f"][rows[0], 1], y1, T.K1)
            worst_y1, worst_v = max(worst_y1, qy), max(worst_v, qv)
        if nc == A and A > 1:
            assert not torch.equal(got["f"][0, 1], got["f"][A - 1, 1])       # every critic its own value
    line = f"cnn team step N{N} A{A} critic rows | y1 {worst_y1:.4f} value {worst_v:.4f}"
    print(line)
    assert T.value_passes(worst_y1, worst_v), line


def test_critic_first_layer_is_exact_on_one_hot_rows():
    """a2 rows that are 1.0 at one k and 0 elsewhere: y1[j] = float32(W1[j][k] + b1[j]) bit for bit at the first and last float of
    every wave's quarter and of its 4-float tail, the piece boundaries 31 / 32 and the lane halves' 15 / 16 -- on the critic rows and,
    through the same loop, the actor rows."""
    A = 2
    m = D.master(F, 3, critics_too=True)
    ks = S.onehot_ks(13)
    assert {0, 675, 676, 2703, 672, 671, 15, 16, 31, 32} <= set(ks)
    a2, u = D.onehot_rows(A, FLAT, ks)
    got = _call(m["seqs"][:A], m["crit"][:A], a2, a2, u, len(ks), A)
    D.check_onehot_y1(got["y1"], m["seqs"][:A] + m["crit"][:A], ks, 13)


def test_bootstrap_round_writes_slot_two_under_the_mask_and_nothing_else():
    def boot_y1(got, step, on, A):                          # the kernel skips whole tiles: lanes 0..63 are all masked out
        assert _is_sentinel(got["y1"][A:, :64]) and not _is_sentinel(got["y1"][A:, 64:][:, on[64:]])

    A, N = 3, 130
    m, step = D.bootstrap_round(F, A, boot_y1, None)
    a2a, a2c, u = m["a2a"], m["a2c"], m["u"]
    # refusals that need no launch: a bootstrap round without a mask, a step round without act8, two critics for three agents
    ap, cp = D.head_params(m["seqs"]), D.head_params(m["crit"])
    assert D.call("rs_cnn_team_step_head", None, A, cp, A, None, a2c, None, None, step[A]["f"], None, None, None, N) == 1
    assert D.call("rs_cnn_team_step_head", ap, A, cp, A, a2a, a2c, u, step[A]["act"], step[A]["f"], None, None, None, N) == 1
    assert D.call("rs_cnn_team_step_head", ap, A, D.head_params(m["crit"][:2]), 2, a2a, a2c, u, step[A]["act"], step[A]["f"], step[A]["act8"],
                  None, None, N) == 1


def test_results_do_not_depend_on_how_the_envs_are_sharded():
    """N = 130 in one call against the same lanes as two calls of 65: equal bits in every output."""
    D.sharding(F, 3)


CRITIC_TRUNK_CASES = [(N, nc) for N in (1, 2, 3, 4, 193) for nc in (1, 3, 8)]


@pytest.mark.parametrize("N,nc", CRITIC_TRUNK_CASES, ids=[f"N{n}-C{c}" for n, c in CRITIC_TRUNK_CASES])
def test_critic_team_trunk_equals_one_trunk_launch_per_critic_bit_for_bit(N, nc):
    crit = [c.critic.cuda() for c in D.critics(nc, 100 * N + nc)]
    D.check_team_trunk(F, "critic", crit, T.random_maps(N, 2, seed=17 * N + nc)[0])


# ------------------------------------------------------------------------------------------------ the collector
CN, CA, CT, CL = 64, 3, 12, 7
FLAG = "team_round"


def _collector(team, walls=True, T_=CT, L=CL, **kw):
    return D.collector(team, FLAG, walls, T_, L, **kw)


@pytest.mark.parametrize("team", [True, False], ids=["global-critic", "own-critics"])
def test_collector_team_round_against_the_per_agent_round_and_the_modules(team):
    D.collector_round_against_the_per_agent_round_and_the_modules(_collector, FLAG, team, CT, CA)


@pytest.mark.parametrize("team", [True, False], ids=["global-critic", "own-critics"])
def test_collector_team_round_graph_equals_eager_and_two_halves_equal_the_whole(team):
    D.collector_graph_equals_eager_and_two_halves_equal_the_whole(_collector, FLAG, team, CN)


def test_collector_falls_back_to_the_per_agent_round():
    col, _ = _collector(True, N=8, walls=False, T_=8, L=4)              # walls off, 4-step episodes: 31 x 31 maps, today's round
    assert tuple(col.maps.map_dimensions) == (31, 31) and col.use_heads and not col.use_team_round
    col.collect()
    assert int(col.buf.act.max()) <= 7 and bool(torch.isfinite(col.buf.val).all())
    col, _ = _collector(True, N=8, on=False)
    assert not col.use_team_round
    col.collect()
    assert bool(torch.isfinite(col.buf.logp).all())
    col, _ = _collector(True, N=8)
    assert col.use_team_round
    col.heads = False
    assert not col.use_team_round


def test_train_ppo_cnn_runs_an_epoch_with_the_team_round_on():
    sim = D.train_ppo_cnn_one_epoch(walls=True)
    assert sim.collector.use_team_round and getattr(sim.collector, "_hp_act", None) is not None          # the team round ran
