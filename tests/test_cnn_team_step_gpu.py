"""The RAD-TEAM (CNN) training round in three launches: rs_cnn_team_step_head, rs_cnn_team_critic_trunk_infer and the collector that
issues them (CNNCollector.use_team_round).

Actor rows: act, slot 0 (logp) and y1 equal rs_cnn_team_eval_head's (alive all 1) bit for bit and act8 is the drawn action, at the cases
of tests/_cnn_team_ref.py -- N = 1, 31, 32, 33, 63, 64, 65, 130 with 3 agents and (64, 8): the 32-image MFMA tile, the 64-image workgroup,
ragged tiles -- on its maps and teams.  So no draw can differ from the float64 draw that did not differ for the evaluation head, whose
own test holds it to DRAW_CAP.

Critic rows: the first layer exact on one-hot a2 rows at the edges of the k-quarters, pieces, lane halves and the 4-float tail; the value
(slot 1) equal to rs_cnn_head(out_dim = 1) on the kernel's own y1 bit for bit, and within the float64 rule of tests/_f64_ref.py's heads
(HEAD_K2, HEAD_K3) with the first layer's K1 term of tests/_cnn_team_ref.py -- the allowance _cnn_team_ref.reference gives a logit, here
for the one output.  The worst ratios are printed; profiles/cnn_team_step_float64_ratios.txt keeps a copy.

Both critic modes, the bootstrap round (slot 2 under a mask, nothing else touched, an all-masked tile and an all-zero mask), sharding
(N = 130 against 65 twice), the critic team trunk against rs_cnn_trunk_infer(agent = -1) per critic, and the collector: team round on
against off, every stored row against the modules, graph against eager, two half collectors against one, the fall-back conditions, and
one train_PPO('cnn') epoch."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_sized_team_ref as S  # noqa: E402
import _cnn_team_ref as T  # noqa: E402
import _f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678
FLAT = 2704
SEED = 1234


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _params(seqs):
    from radiation_ppo_amd import _lib
    return (_lib.RsCnnHeadParams * len(seqs))(*[_lib.RsCnnHeadParams(_p(s[6].weight), _p(s[6].bias), _p(s[8].weight), _p(s[8].bias),
                                                                      _p(s[10].weight), _p(s[10].bias)) for s in seqs])


def _prepare(lib, seqs, cin):
    from radiation_ppo_amd import _lib
    wt = torch.empty(len(seqs), lib.rs_cnn_trunk_scratch_floats(cin), dtype=torch.float32, device="cuda")
    for i, s in enumerate(seqs):
        _lib.check(lib.rs_cnn_trunk_prepare(cin, _p(s[0].weight), _p(s[0].bias), _p(s[3].weight), _p(s[3].bias), _p(wt[i]), _stream()),
                   "rs_cnn_trunk_prepare")
    return wt


def _critics(n, seed):
    """n critic networks with biases that matter and visibly different values"""
    from radiation_ppo_amd.maps import CNNCritic
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        mods = [CNNCritic() for _ in range(n)]
    with torch.no_grad():
        for m in mods:
            m.critic[0].bias.uniform_(-0.05, 0.15)
            m.critic[3].bias.uniform_(-0.1, 0.1)
            for i in (6, 8, 10):
                for p in m.critic[i].parameters():
                    p.mul_(T.SCALE)
    return mods


_MASTER = {}


def _master(A):
    """Once per team size: _cnn_team_ref's actors and maps, A critics, both roles' trunk outputs on the MASTER lanes."""
    if A in _MASTER:
        return _MASTER[A]
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    t = T.team(A)
    seqs = [T.clone_seq(ac.actor, "cuda") for ac in t.actors]
    cpu_critics = _critics(A, 7300 + A)
    crit = [T.clone_seq(c.critic, "cuda") for c in cpu_critics]
    wt, wt_c = _prepare(lib, seqs, 6), _prepare(lib, crit, 4)
    N = T.MASTER
    maps = t.maps.cuda()
    a2a = torch.empty(A, N, FLAT, device="cuda")
    a2c = torch.empty(A, N, FLAT, device="cuda")
    _lib.check(lib.rs_cnn_team_trunk_infer(_p(maps), _p(t.cells.int().cuda()), _p(t.pcells.int().cuda()), A, N, _p(wt), _p(a2a), _stream()),
               "rs_cnn_team_trunk_infer")
    _lib.check(lib.rs_cnn_team_critic_trunk_infer(_p(maps), A, N, _p(wt_c), _p(a2c), _stream()), "rs_cnn_team_critic_trunk_infer")
    torch.cuda.synchronize()
    assert float(a2c.min()) >= 0.0 and float(a2c.max()) > 0.0
    m = dict(t=t, seqs=seqs, crit=crit, cpu_critics=cpu_critics, a2a=a2a, a2c=a2c, u=t.u.cuda())
    _MASTER[A] = m
    return m


def _call(lib, actors, critics, a2a, a2c, u, N, A, mask=None, boot=False):
    """rs_cnn_team_step_head into sentinel-filled, guarded buffers: dict(rc, act [A, N], f [A, 3, N], act8 [N, A], y1 [A + C, N, 32])"""
    nc = len(critics)
    act = torch.full((A * N + 2,), -1, dtype=torch.int64, device="cuda")
    f = torch.full((A * 3 * N + 2,), SENTINEL, device="cuda")
    act8 = torch.full((N + 2, A), -1, dtype=torch.int8, device="cuda")
    y1 = torch.full(((A + nc) * N + 2, 32), SENTINEL, device="cuda")
    if boot:
        rc = lib.rs_cnn_team_step_head(None, A, _params(critics), nc, None, _p(a2c), None, None, _p(f[1:]), None, _p(mask), _p(y1[1:]), N, _stream())
    else:
        rc = lib.rs_cnn_team_step_head(_params(actors), A, _params(critics), nc, _p(a2a), _p(a2c), _p(u), _p(act[1:]), _p(f[1:]), _p(act8[1:]),
                                       _p(mask), _p(y1[1:]), N, _stream())
    torch.cuda.synchronize()
    assert int(act[0]) == -1 and int(act[-1]) == -1 and bool((act8[0] == -1).all()) and bool((act8[N + 1] == -1).all())
    for g in (f[0], f[-1], y1[0], y1[-1]):
        assert torch.equal(_bits(g), _bits(torch.full_like(g, SENTINEL)))
    return dict(rc=rc, act=act[1:A * N + 1].view(A, N), f=f[1:A * 3 * N + 1].view(A, 3, N), act8=act8[1:N + 1],
                y1=y1[1:(A + nc) * N + 1].view(A + nc, N, 32))


def _is_sentinel(t):
    return torch.equal(_bits(t), _bits(torch.full_like(t, SENTINEL)))


def _eval_head(lib, seqs, a2, u, A, N):
    from radiation_ppo_amd import _lib
    act8 = torch.empty(N, A, dtype=torch.int8, device="cuda")
    act = torch.empty(A, N, dtype=torch.int64, device="cuda")
    logp, y1 = torch.empty(A, N, device="cuda"), torch.empty(A, N, 32, device="cuda")
    alive = torch.ones(N, dtype=torch.uint8, device="cuda")
    _lib.check(lib.rs_cnn_team_eval_head(_params(seqs), A, _p(a2), _p(u), _p(alive), _p(act8), _p(act), _p(logp), _p(y1), N, _stream()),
               "rs_cnn_team_eval_head")
    torch.cuda.synchronize()
    return act8, act, logp, y1


def _value_by_rs_cnn_head(lib, s, y1, N):
    from radiation_ppo_amd import _lib
    v = torch.full((N,), SENTINEL, device="cuda")
    y1 = y1.contiguous()
    _lib.check(lib.rs_cnn_head(_p(y1), _p(s[8].weight), _p(s[8].bias), _p(s[10].weight), _p(s[10].bias), 1, None, 1, None, None, None, 1,
                               _p(v), 1, 0, None, N, _stream()), "rs_cnn_head")
    torch.cuda.synchronize()
    return v


def _value_ratio(seq_cpu, a2, got_v, got_y1):
    """(worst |y1 - ref| / allowance, worst |value - ref| / allowance) under _cnn_team_ref.reference's lines for y1 and for a logit"""
    s64 = R.f64(seq_cpu)
    with torch.no_grad():
        x = a2.detach().double().cpu()
        W1, b1, W2, W3 = s64[6].weight, s64[6].bias, s64[8].weight, s64[10].weight
        y1 = x @ W1.t() + b1
        mag1 = x.abs() @ W1.abs().t() + b1.abs()
        y1_allow = R.FF_RTOL * y1.abs() + T.K1 * R.U * mag1 + R.FF_TINY
        val, mag3, carried = R.cnn_head_f64(s64, y1)
        through = (mag1 @ W2.abs().t()) @ W3.abs().t()
        allow = R.FF_RTOL * val.abs() + R.U * (T.K1 * through + R.HEAD_K2 * carried + R.HEAD_K3 * mag3) + R.FF_TINY
        gv, gy = got_v.detach().double().cpu().reshape(val.shape), got_y1.detach().double().cpu()
        assert bool(torch.isfinite(gv).all()) and bool(torch.isfinite(gy).all())
        return float(((gy - y1).abs() / y1_allow).max()), float(((gv - val).abs() / allow).max())


@pytest.mark.parametrize("N,A", T.CASES, ids=[f"N{n}-A{a}" for n, a in T.CASES])
def test_step_round_actor_rows_are_the_evaluation_heads_bits_and_critic_rows_hold_to_float64(N, A):
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    m = _master(A)
    a2a, a2c, u = m["a2a"][:, :N].contiguous(), m["a2c"][:, :N].contiguous(), m["u"][:N].contiguous()
    e8, eact, elogp, ey1 = _eval_head(lib, m["seqs"], a2a, u, A, N)
    assert int(torch.unique(eact).numel()) >= (3 if N >= 31 else 1)
    worst_y1 = worst_v = 0.0
    for nc in (1, A):
        got = _call(lib, m["seqs"], m["crit"][:nc], a2a, a2c[:nc].contiguous(), u, N, A)
        assert got["rc"] == 0
        # ---- actor rows
        assert torch.equal(got["act"], eact) and torch.equal(_bits(got["f"][:, 0]), _bits(elogp)), (N, A, nc)
        assert torch.equal(_bits(got["y1"][:A]), _bits(ey1))
        assert torch.equal(got["act8"].long(), got["act"].t()) and torch.equal(got["act8"], e8)
        assert _is_sentinel(got["f"][:, 2])                                  # the step round leaves the bootstrap slot alone
        # ---- critic rows
        for c in range(nc):
            y1 = got["y1"][A + c]
            want = _value_by_rs_cnn_head(lib, m["crit"][c], y1, N)
            rows = range(A) if nc == 1 else (c,)
            for a in rows:                                                   # a global critic's value in every agent's row
                assert torch.equal(_bits(got["f"][a, 1]), _bits(want)), (N, A, nc, c, a)
            qy, qv = _value_ratio(m["cpu_critics"][c].critic, a2c[c], got["f"][rows[0], 1], y1)
            worst_y1, worst_v = max(worst_y1, qy), max(worst_v, qv)
        if nc == A and A > 1:
            assert not torch.equal(got["f"][0, 1], got["f"][A - 1, 1])       # every critic its own value
    line = f"cnn team step N{N} A{A} critic rows | y1 {worst_y1:.4f} value {worst_v:.4f}"
    print(line)
    assert worst_y1 <= 1.0 and worst_v <= 1.0, line


def test_critic_first_layer_is_exact_on_one_hot_rows():
    """a2 rows that are 1.0 at one k and 0 elsewhere: y1[j] = float32(W1[j][k] + b1[j]) bit for bit at the first and last float of
    every wave's quarter and of its 4-float tail, the piece boundaries 31 / 32 and the lane halves' 15 / 16 -- on the critic rows and,
    through the same loop, the actor rows."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    A = 2
    m = _master(3)
    ks = S.onehot_ks(13)
    assert {0, 675, 676, 2703, 672, 671, 15, 16, 31, 32} <= set(ks)
    N = len(ks)
    a2 = torch.zeros(A, N, FLAT, device="cuda")
    a2[:, torch.arange(N), torch.tensor(ks)] = 1.0
    u = torch.rand(N, A, device="cuda")
    got = _call(lib, m["seqs"][:A], m["crit"][:A], a2, a2, u, N, A)
    for row, s in enumerate(m["seqs"][:A] + m["crit"][:A]):
        with torch.no_grad():
            want = s[6].weight[:, ks].t().contiguous() + s[6].bias
        bad = (_bits(got["y1"][row]) != _bits(want)).nonzero()
        assert bad.numel() == 0, (row, [(ks[n], j) for n, j in bad[:6].tolist()])
        assert float(want.abs().min()) > 0


def test_bootstrap_round_writes_slot_two_under_the_mask_and_nothing_else():
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    A, N = 3, 130
    m = _master(A)
    a2a, a2c, u = m["a2a"], m["a2c"], m["u"]
    step = {nc: _call(lib, m["seqs"], m["crit"][:nc], a2a, a2c[:nc].contiguous(), u, N, A) for nc in (1, A)}
    mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
    mask[[64, 70, 127, 128, 129]] = 1                                       # lanes 0..63 all zero: the first tile returns early
    mask[100] = 7                                                           # any non-zero byte counts
    on = mask != 0
    for nc in (1, A):
        got = _call(lib, None, m["crit"][:nc], None, a2c[:nc].contiguous(), None, N, A, mask=mask, boot=True)
        assert got["rc"] == 0
        assert bool((got["act"] == -1).all()) and bool((got["act8"] == -1).all())
        assert _is_sentinel(got["f"][:, 0]) and _is_sentinel(got["f"][:, 1]) and _is_sentinel(got["y1"][:A])
        assert _is_sentinel(got["f"][:, 2][:, ~on]) and _is_sentinel(got["y1"][A:, :64])
        # the masked envs: the step round's value bits (the same critic on the same a2), in slot 2
        assert torch.equal(_bits(got["f"][:, 2][:, on]), _bits(step[nc]["f"][:, 1][:, on])), nc
        assert not _is_sentinel(got["y1"][A:, 64:][:, on[64:]])
    # a step round under a mask: the masked-out envs write nothing, the others what the unmasked round wrote
    got = _call(lib, m["seqs"], m["crit"], a2a, a2c, u, N, A, mask=mask)
    assert got["rc"] == 0
    assert bool((got["act"][:, ~on] == -1).all()) and bool((got["act8"][~on] == -1).all()) and _is_sentinel(got["f"][:, :, ~on])
    assert torch.equal(got["act"][:, on], step[A]["act"][:, on]) and torch.equal(_bits(got["f"][:, :2][:, :, on]), _bits(step[A]["f"][:, :2][:, :, on]))
    # an empty mask: nothing written, RS_OK
    got = _call(lib, None, m["crit"], None, a2c, None, N, A, mask=torch.zeros(N, dtype=torch.uint8, device="cuda"), boot=True)
    assert got["rc"] == 0 and _is_sentinel(got["f"]) and _is_sentinel(got["y1"])
    # refusals that need no launch: a bootstrap round without a mask, a step round without act8, two critics for three agents
    H = _lib.RsCnnHeadParams
    assert lib.rs_cnn_team_step_head(None, A, _params(m["crit"]), A, None, _p(a2c), None, None, _p(step[A]["f"]), None, None, None, N, _stream()) == 1
    assert lib.rs_cnn_team_step_head(_params(m["seqs"]), A, _params(m["crit"]), A, _p(a2a), _p(a2c), _p(u), _p(step[A]["act"]), _p(step[A]["f"]),
                                     None, None, None, N, _stream()) == 1
    assert lib.rs_cnn_team_step_head(_params(m["seqs"]), A, (H * 2)(*_params(m["crit"])[:2]), 2, _p(a2a), _p(a2c), _p(u), _p(step[A]["act"]),
                                     _p(step[A]["f"]), _p(step[A]["act8"]), None, None, N, _stream()) == 1


def test_results_do_not_depend_on_how_the_envs_are_sharded():
    """N = 130 in one call against the same lanes as two calls of 65: equal bits in every output."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    A, N = 3, 130
    m = _master(A)
    whole = _call(lib, m["seqs"], m["crit"], m["a2a"], m["a2c"], m["u"], N, A)
    for lo in (0, 65):
        sl = slice(lo, lo + 65)
        part = _call(lib, m["seqs"], m["crit"], m["a2a"][:, sl].contiguous(), m["a2c"][:, sl].contiguous(), m["u"][sl].contiguous(), 65, A)
        assert torch.equal(part["act"], whole["act"][:, sl]) and torch.equal(part["act8"], whole["act8"][sl])
        assert torch.equal(_bits(part["f"][:, :2]), _bits(whole["f"][:, :2, sl])) and torch.equal(_bits(part["y1"]), _bits(whole["y1"][:, sl]))


CRITIC_TRUNK_CASES = [(N, nc) for N in (1, 2, 3, 4, 193) for nc in (1, 3, 8)]


@pytest.mark.parametrize("N,nc", CRITIC_TRUNK_CASES, ids=[f"N{n}-C{c}" for n, c in CRITIC_TRUNK_CASES])
def test_critic_team_trunk_equals_one_trunk_launch_per_critic_bit_for_bit(N, nc):
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    crit = [c.critic.cuda() for c in _critics(nc, 100 * N + nc)]
    maps = T.random_maps(N, 2, seed=17 * N + nc)[0].cuda()
    wt = _prepare(lib, crit, 4)
    G = 2 * FLAT
    buf = torch.full((G + nc * N * FLAT + G,), SENTINEL, device="cuda")
    _lib.check(lib.rs_cnn_team_critic_trunk_infer(_p(maps), nc, N, _p(wt), _p(buf[G:]), _stream()), "rs_cnn_team_critic_trunk_infer")
    torch.cuda.synchronize()
    assert _is_sentinel(buf[:G]) and _is_sentinel(buf[G + nc * N * FLAT:])
    got = buf[G:G + nc * N * FLAT].view(nc, N, FLAT)
    assert not bool((got == SENTINEL).any())
    for c in range(nc):
        want = torch.full((N, FLAT), SENTINEL, device="cuda")
        _lib.check(lib.rs_cnn_trunk_infer(_p(maps), None, None, 0, -1, N, _p(wt[c]), _p(want), _stream()), "rs_cnn_trunk_infer")
        torch.cuda.synchronize()
        assert float(want.abs().max()) > 0 and torch.equal(_bits(got[c]), _bits(want)), (N, nc, c)
    if nc > 1:
        assert not torch.equal(got[0], got[nc - 1])


# ------------------------------------------------------------------------------------------------ the collector
CN, CA, CT, CL = 64, 3, 12, 7
KEYS = ("obs", "act", "rew", "val", "logp", "last_val", "cut", "adv", "ret")


def _collector(team, N=CN, base=32, use_graph=False, team_round=None, record=None, walls=True, T_=CT, L=CL):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.maps import CNNCritic, heat_map_geometry
    from radiation_ppo_amd.ppo_cnn import CNNAgentPPO, CNNCollector
    torch.manual_seed(8)
    env = RadSearchVec(N, number_agents=CA, obstruction_count=2, enforce_grid_boundaries=walls, seed=SEED, env_id_base=base)
    kw = {} if walls else dict(map_dim=tuple(heat_map_geometry(env, L, False)[2]))
    gc = CNNCritic(**kw).cuda() if team else None
    agents = {i: CNNAgentPPO(id=i, GlobalCritic=gc, GlobalCriticOptimizer=torch.optim.Adam(gc.parameters(), lr=1e-3) if team else None, **kw)
              for i in range(CA)}
    with torch.no_grad():
        for ag in agents.values():
            for p in list(ag.pi.actor[6:].parameters()):
                p.mul_(3.0)                                   # visibly non-uniform policies
    col = CNNCollector(env, agents, T_, L, global_critic_flag=team, use_graph=use_graph)
    if team_round is not None:
        col.team_round = team_round
    if record is not None:                                    # the bootstrap rounds' maps and masks, as the team round receives them
        inner = col._team_round

        def spy(maps, mask8=None):
            if mask8 is not None:
                record.append((int(col._t), maps.clone(), mask8.clone()))
            return inner(maps, mask8=mask8)
        col._team_round = spy
    return col, agents


def _stored(col):
    return {**{k: getattr(col.buf, k).clone() for k in KEYS}, "shared": col.shared.clone(), "cells": col.cells.clone(),
            "pcells": col.pcells.clone(), "complete_len": col.complete_len.clone()}


@pytest.mark.parametrize("team", [True, False], ids=["global-critic", "own-critics"])
def test_collector_team_round_against_the_per_agent_round_and_the_modules(team):
    boots = []
    cf, af = _collector(team, record=boots)
    assert cf.use_team_round
    cf.collect()
    cm, _ = _collector(team, team_round=False)
    assert not cm.use_team_round and cm.use_heads
    cm.collect()
    # ---- the first lock-step, where both collectors see the same state
    same = cf.buf.act[0] == cm.buf.act[0]
    assert float(same.float().mean()) > 0.99
    assert torch.allclose(cf.buf.logp[0][same], cm.buf.logp[0][same], rtol=1e-4, atol=2e-5)
    assert torch.allclose(cf.buf.val[0], cm.buf.val[0], rtol=1e-4, atol=2e-5)
    assert torch.equal(cf.buf.obs[0], cm.buf.obs[0]) and torch.equal(cf.shared[0], cm.shared[0])
    assert torch.equal(cf.cells[0], cm.cells[0]) and torch.equal(cf.pcells[0], cm.pcells[0])
    # ---- the whole epoch: every stored row against the modules on the stored maps
    assert int(cf.buf.act.min()) >= 0 and int(cf.buf.act.max()) <= 7 and int(torch.unique(cf.buf.act).numel()) >= 3
    for t in range(CT):
        for a, ag in af.items():
            logits = ag.pi.logits_from_maps(cf.shared[t], cf.cells[t], cf.pcells[t], a)
            lp = torch.log_softmax(logits, dim=-1).gather(-1, cf.buf.act[t, :, a].unsqueeze(-1)).squeeze(-1)
            assert torch.allclose(cf.buf.logp[t, :, a], lp, rtol=1e-4, atol=2e-5), (t, a)
            assert torch.allclose(cf.buf.val[t, :, a], ag.critic.value_from_maps(cf.shared[t]), rtol=1e-4, atol=2e-5), (t, a)
    if not team:
        assert not torch.equal(cf.buf.val[:, :, 0], cf.buf.val[:, :, CA - 1])
    # ---- last_val: non-zero on cut rows only, and there the critic on the bootstrap round's maps
    nz = cf.buf.last_val != 0
    assert int(nz.sum()) > 0 and bool((cf.buf.cut[nz.any(dim=2)] == 1).all())
    assert len(boots) == CT
    timeouts = 0
    for t, maps, mask in boots:
        on = mask != 0
        assert not bool(nz[t][~on].any()), t
        if t < CT - 1:
            timeouts += int(on.sum())                                   # before the epoch's end only time-outs are bootstrapped
        for a, ag in af.items():
            v = ag.critic.value_from_maps(maps)
            assert torch.allclose(cf.buf.last_val[t, :, a][on], v[on], rtol=1e-4, atol=2e-5), (t, a)
    assert timeouts > 0 and bool((boots[-1][2] != 0).all())


@pytest.mark.parametrize("team", [True, False], ids=["global-critic", "own-critics"])
def test_collector_team_round_graph_equals_eager_and_two_halves_equal_the_whole(team):
    runs = {}
    for name, kw in (("eager", dict()), ("graph", dict(use_graph=True)), ("lo", dict(N=CN // 2, base=32)), ("hi", dict(N=CN // 2, base=32 + CN // 2))):
        col, _ = _collector(team, **kw)
        assert col.use_team_round
        col.collect()
        assert (col._graph is not None) == (name == "graph") and col.env.error_flags() == 0
        runs[name] = _stored(col)
    for k in runs["eager"]:
        assert torch.equal(runs["graph"][k], runs["eager"][k]), k
        if k in ("complete_len",):
            halves = torch.cat([runs["lo"][k], runs["hi"][k]], dim=0)
        else:
            halves = torch.cat([runs["lo"][k], runs["hi"][k]], dim=1)
        if k in ("adv", "ret"):
            continue                                                    # (GAE over the rows checked here)
        assert torch.equal(halves, runs["eager"][k]), k


def test_collector_falls_back_to_the_per_agent_round():
    col, _ = _collector(True, N=8, walls=False, T_=8, L=4)              # walls off, 4-step episodes: 31 x 31 maps, today's round
    assert tuple(col.maps.map_dimensions) == (31, 31) and col.use_heads and not col.use_team_round
    col.collect()
    assert int(col.buf.act.max()) <= 7 and bool(torch.isfinite(col.buf.val).all())
    col, _ = _collector(True, N=8, team_round=False)
    assert not col.use_team_round
    col.collect()
    assert bool(torch.isfinite(col.buf.logp).all())
    col, _ = _collector(True, N=8)
    assert col.use_team_round
    col.heads = False
    assert not col.use_team_round


def test_train_ppo_cnn_runs_an_epoch_with_the_team_round_on():
    import numpy as np
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.train import train_PPO
    A = 2
    env = RadSearchVec(16, number_agents=A, obstruction_count=1, enforce_grid_boundaries=True, seed=6)
    sim = train_PPO(env=env, logger_kwargs={}, ppo_kwargs=dict(steps_per_epoch=16, steps_per_episode=8, number_of_agents=A, train_pi_iters=2,
                                                               train_v_iters=2),
                    seed=6, number_of_agents=A, actor_critic_architecture="cnn", global_critic_flag=True, steps_per_epoch=16,
                    steps_per_episode=8, total_epochs=1)
    sim.train()
    assert sim.collector.use_team_round and getattr(sim.collector, "_hp_act", None) is not None          # the team round ran
    for i in range(A):
        rows = sim.loggers[i].rows
        assert len(rows) == 1 and np.isfinite(rows[0]["loss_policy"]), i
    assert np.isfinite(sim.loggers[0].rows[0]["loss_critic"])         # only agent 0 updates the global critic (ppo.py:858)
    buf = sim.collector.buf
    assert bool(torch.isfinite(buf.logp).all()) and bool(torch.isfinite(buf.val).all()) and int(buf.act.max()) <= 7
