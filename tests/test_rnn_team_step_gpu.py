"""A recurrent team's policy round as one launch (csrc/rs_rnn_policy.hip: rs_rnn_team_step; csrc/rs_rnn_sized.hip:
rs_rnn_sized_team_step): the kernels against one K14 / sized-step launch per agent, bit for bit, in the three uses they have (the
collector's step round, its bootstrap round, the evaluation's round without value and log-probability); RNNCollector with
use_team_step against the per-agent form, bit for bit over two epochs, eagerly and through the captured graph, also across a change of
the policy between the epochs; run_test_environments_rnn_team at a sized width of another tier than 32, fused against composed; and
train_PPO with two recurrent agents end to end."""
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
from test_ppo_gpu import SEED  # noqa: E402

pytestmark = pytest.mark.gpu

MASKS = {"all": lambda n: torch.ones_like(n, dtype=torch.bool), "wave_off": lambda n: (n < 64) | (n >= 128), "thirds": lambda n: n % 3 != 1}
SHAPES = [(70, 2), (200, 3), (65, 8)]
# None: rs_rnn_team_step (GRU 24, heads 32 / 32); (hid, pol, val): rs_rnn_sized_team_step, one case per GRU tier (16, 32, 48, 64) -- a hid
# that is no multiple of 4 takes the float-by-float row loads and stores, a head width that is no multiple of 8 the padded head blocks
KERNEL_WIDTHS = [None, (13, 2, 37), (32, 64, 64), (40, 9, 8), (64, 33, 2)]
F_MARK, ACT_MARK, ACT8_MARK = 12345.0, -7, -3


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def packed():
    """{widths: eight agents' packed weights}: every agent its own seeded network, policy scaled to be decisive; packed once, read only"""
    from radiation_ppo_amd.rada2c import RNNModelActorCritic, pack_policy_weights, pack_sized_policy_weights
    out = {}
    for w in KERNEL_WIDTHS:
        out[w] = []
        for a in range(8):
            torch.manual_seed(50 + 7 * a)
            ac = RNNModelActorCritic(**(_args(*w, 16) if w else {})).to(DEV)
            assert ac.fused_policy == (w is None) and ac.sized_policy == (w is not None)
            with torch.no_grad():
                for q in ac.pi.parameters():
                    q.mul_(3.0)
                out[w].append((pack_policy_weights(ac) if w is None else pack_sized_policy_weights(ac)).contiguous())
    return out


def _team(lib, widths, wp, A, x, loc, h, u, act, f, act8, mask, N):
    from radiation_ppo_amd import _lib
    tail = (_p(x), _p(loc), _p(h), _p(u), _p(act), _p(f), _p(act8), _p(mask), N, H.stream())
    if widths is None:
        _lib.check(lib.rs_rnn_team_step(wp, A, *tail), "rs_rnn_team_step")
    else:
        _lib.check(lib.rs_rnn_sized_team_step(wp, A, *widths, *tail), "rs_rnn_sized_team_step")


def _per_agent(lib, widths, w, a, A, x, loc, h, u, h_out, value, act, logp, act8, mask, N):
    """one K14 / sized-step launch on agent a's rows of the [N][A][.] tensors: the reference"""
    from radiation_ppo_amd import _lib
    xa, la = _p(x) + 44 * a, _p(loc) + 8 * a
    ua = None if u is None else _p(u) + 4 * a
    a8 = None if act8 is None else _p(act8) + a
    if widths is None:
        _lib.check(lib.rs_rnn_policy_step_rows(_p(w), xa, 11 * A, la, 2 * A, _p(h), ua, A, _p(h_out), _p(value), _p(act), _p(logp), a8, A,
                                               _p(mask), N, H.stream()), "rs_rnn_policy_step_rows")
    else:
        _lib.check(lib.rs_rnn_sized_step(_p(w), *widths, xa, 11 * A, la, 2 * A, _p(h), ua, A, _p(h_out), None, _p(value), _p(act), _p(logp),
                                         a8, A, _p(mask), N, H.stream()), "rs_rnn_sized_step")


def _same(got, want, name):
    assert got.dtype == want.dtype and torch.equal(got, want), (name, (got != want).nonzero()[:6].tolist())


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("N,A", SHAPES)
@pytest.mark.parametrize("widths", KERNEL_WIDTHS, ids=lambda w: "default" if w is None else "x".join(map(str, w)))
def test_team_step_equals_one_launch_per_agent_bit_for_bit(packed, widths, N, A, mask):
    """N = 70 and 65: a ragged last wave (with `wave_off` that whole wave is masked out and leaves); N = 200: four waves, 64..127 off.
    Every agent has its own weights, so a wrong blockIdx.y -> agent mapping shows.  Every output starts from a sentinel.  With `all`
    the collector's two rounds get mask = NULL and the evaluation's round a mask of ones."""
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    hid = 24 if widths is None else widths[0]
    g = torch.Generator(device=DEV).manual_seed(1000 + N + A)
    rnd = lambda *s: torch.rand(*s, device=DEV, generator=g)
    W = packed[widths][:A]
    wp = (C.c_void_p * A)(*[_p(w) for w in W])
    x, loc, u = rnd(N, A, 11) * 2.0 - 1.0, rnd(N, A, 2), rnd(N, A)
    h0 = (rnd(A, N, hid) * 2.0 - 1.0) / hid ** 0.5
    on = MASKS[mask](torch.arange(N, device=DEV))
    m8 = on.to(torch.uint8)
    m_null = None if mask == "all" else m8

    def fresh():
        return (h0.clone(), torch.full((A, N), ACT_MARK, dtype=torch.int64, device=DEV), torch.full((A, 3, N), F_MARK, device=DEV),
                torch.full((N, A), ACT8_MARK, dtype=torch.int8, device=DEV))

    # ---- 1. the collector's step round
    h_k, act_k, f_k, a8_k = fresh()
    _team(lib, widths, wp, A, x, loc, h_k, u, act_k, f_k, a8_k, m_null, N)
    h_r, act_r, f_r, a8_r = fresh()
    for a in range(A):
        _per_agent(lib, widths, W[a], a, A, x, loc, h_r[a], u, h_r[a], f_r[a, 1], act_r[a], f_r[a, 0], a8_r, m_null, N)
    torch.cuda.synchronize()
    for name, got, want in (("h", h_k, h_r), ("act", act_k, act_r), ("logp_val_boot", f_k, f_r), ("act8", a8_k, a8_r)):
        _same(got, want, "step round: " + name)
    assert bool((f_k[:, 2] == F_MARK).all())                                               # the bootstrap slot is not the step round's
    assert torch.equal(h_k[:, ~on], h0[:, ~on]) and bool((a8_k[~on] == ACT8_MARK).all()) and bool((act_k[:, ~on] == ACT_MARK).all())
    assert bool((f_k[:, :, ~on] == F_MARK).all())
    assert bool((h_k[:, on] != h0[:, on]).any(dim=-1).all())                               # every live (agent, env) row moved
    assert bool((f_k[:, :2, on] != F_MARK).all()) and bool((f_k[:, 0, on] <= 0).all())
    assert torch.equal(act_k.t().to(torch.int8)[on], a8_k[on])
    assert int(a8_k[on].min()) >= 0 and int(a8_k[on].max()) <= 7 and len(torch.unique(a8_k[on])) > 2

    # ---- 2. the collector's bootstrap round, on the states the step round left
    h1 = h_k.clone()
    f_b, f_br = f_k.clone(), f_k.clone()
    _team(lib, widths, wp, A, x, loc, h_k, None, None, f_b, None, m_null, N)
    for a in range(A):
        _per_agent(lib, widths, W[a], a, A, x, loc, h1[a], None, None, f_br[a, 2], None, None, None, m_null, N)
    torch.cuda.synchronize()
    _same(f_b, f_br, "bootstrap round: logp_val_boot")
    _same(h_k, h1, "bootstrap round: h")                                                   # not written
    assert torch.equal(f_b[:, :2], f_k[:, :2]) and bool((f_b[:, 2, ~on] == F_MARK).all()) and bool((f_b[:, 2, on] != F_MARK).all())
    assert not torch.equal(f_b[:, 2, on], f_k[:, 1, on])                                   # the value of the NEXT state

    # ---- 3. the evaluation's round: no value, no log-probability, no int64 action
    h_e, _, _, a8_e = fresh()
    _team(lib, widths, wp, A, x, loc, h_e, u, None, None, a8_e, m8, N)
    torch.cuda.synchronize()
    _same(h_e, h_r, "evaluation round: h")
    _same(a8_e, a8_r, "evaluation round: act8")
    assert (mask == "all") == bool(on.all())


# ------------------------------------------------------------------------------------------------------ the collector
FIELDS = ("obs", "act", "rew", "val", "logp", "last_val", "cut", "adv", "ret", "source_tar")


def _collect(A, obst, widths, team_step, use_graph=False, change_policy=False):
    """two epochs of an 80-env collector; everything it wrote and everything it carries after each.  change_policy: every policy
    parameter is changed in place between the epochs (what an update does: the packed buffers are re-packed in place)"""
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector
    N, T, L = 80, 26, 8
    torch.manual_seed(4)
    env = RadSearchVec(N, number_agents=A, obstruction_count=obst, enforce_grid_boundaries=True, seed=SEED, env_id_base=32)
    agents = {a: RNNAgentPPO(id=a, steps_per_epoch=T, steps_per_episode=L, seed=3 + a, train_pi_iters=1, train_pfgru_iters=1,
                             actor_critic_args=WIDTHS[widths]) for a in range(A)}
    with torch.no_grad():
        for ag in agents.values():
            for p in ag.agent.pi.parameters():
                p.mul_(2.0)
    col = RNNCollector(env, agents, T, L, use_graph=use_graph)
    assert col.use_glue and col.use_team_step is True and col.use_k14 == (widths == "default")
    col.use_team_step = team_step
    out = []
    for ep in range(2):
        st = col.collect()
        out.append({**{k: getattr(col.buf, k).clone() for k in FIELDS}, **{"stat_" + k: v.clone() for k, v in st.items()},
                    "c_obs": col.obs.clone(), "c_ret": col.ep_ret.clone(), "c_steps": col.steps_in_ep.clone(), "c_h": col.h.clone(),
                    "w_count": col.stat.count.clone(), "w_mean": col.stat.mean.clone(), "w_sq": col.stat.sq.clone(), "w_std": col.stat.std.clone(),
                    "pf_h": col.bank.h.clone(), "pf_p": col.bank.p.clone(), "pf_episode": col.bank.episode.clone(), "pf_calls": col.bank.calls.clone(),
                    "begun": col.episodes_begun.clone(), "t": col._t.clone()})
        if change_policy and ep == 0:
            with torch.no_grad():
                for a, ag in agents.items():
                    for p in ag.agent.pi.parameters():
                        p.mul_(0.5 + 0.125 * a)
    assert (col._graph is not None) == use_graph
    assert env.error_flags() == 0
    return out


def _same_epochs(got, want):
    assert int(want[0]["cut"].sum()) > 80 * 2 * 2 and float(want[0]["last_val"].abs().sum()) > 0
    for ep in range(2):
        assert got[ep].keys() == want[ep].keys()
        for k in want[ep]:
            assert torch.equal(got[ep][k], want[ep][k]), (ep, k)


@pytest.mark.parametrize("widths", ["default", "sized"])
@pytest.mark.parametrize("A,obst", [(2, 0), (2, 2), (3, 0), (3, 2)])
def test_collector_with_the_team_step_equals_the_per_agent_form(A, obst, widths):
    """rs_rnn_team_step / rs_rnn_sized_team_step in the glued lock-step's two policy rounds against one launch per agent and round:
    after each of two epochs every buffer, the epoch statistics and everything the collector carries are identical, bit for bit"""
    _same_epochs(_collect(A, obst, widths, True), _collect(A, obst, widths, False))


def test_collector_defaults_to_the_team_step_for_teams_only():
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.rada2c import RNNAgentPPO, RNNCollector
    for A, want in ((1, False), (2, True)):
        env = RadSearchVec(16, number_agents=A, obstruction_count=0, enforce_grid_boundaries=True, seed=SEED)
        col = RNNCollector(env, {a: RNNAgentPPO(id=a, steps_per_epoch=8, steps_per_episode=4) for a in range(A)}, 8, 4)
        assert col.use_glue and col.use_team_step is want
    env = RadSearchVec(16, number_agents=2, obstruction_count=0, enforce_grid_boundaries=True, seed=SEED)
    mixed = {0: RNNAgentPPO(id=0, actor_critic_args=_args(32, 64, 64, 16)), 1: RNNAgentPPO(id=1, actor_critic_args=_args(32, 48, 64, 16))}
    assert RNNCollector(env, mixed, 8, 4).use_team_step is False                          # one (hid, pol, val) for the whole team


@pytest.mark.parametrize("change_policy", [False, True], ids=["same_policy", "policy_changed_between_epochs"])
def test_captured_team_step_equals_the_per_agent_form(change_policy):
    """the same through the captured lock-step (use_graph=True), A = 2 at the default widths.  With the policy changed in place between
    the epochs the replayed launch must read the re-packed weights: it equals the eager per-agent form, which packs on every call, and
    its second epoch differs from the one the unchanged policy collects"""
    got = _collect(2, 2, "default", True, use_graph=True, change_policy=change_policy)
    _same_epochs(got, _collect(2, 2, "default", False, use_graph=False, change_policy=change_policy))
    if change_policy:
        plain = _collect(2, 2, "default", True, use_graph=True)
        assert torch.equal(got[0]["act"], plain[0]["act"]) and not torch.equal(got[1]["act"], plain[1]["act"])
        assert not torch.equal(got[1]["val"], plain[1]["val"])


# ------------------------------------------------------------------------------------------------------ the evaluation
E, R, L, SET_SEED = 6, 4, 30, 77
EVAL_WIDTHS = (40, 9, 8, 16)            # GRU tier 48, both head widths ragged, PFGRU 16
EVAL_SEED = 6                           # chosen on the GPU: among the E * R runs a source is found and a run reaches the step limit


def test_fused_sized_team_run_equals_the_composed_run_at_another_tier():
    """tests/test_rnn_team_eval_gpu.py's contract at (40, 9, 8, rec 16): the fused lock-step's policy round is rs_rnn_sized_team_step"""
    from radiation_ppo_amd.evaluate import run_test_environments_rnn_team, sample_test_environments
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    A, obst = 2, 0
    sets = sample_test_environments(E, obstruction_count=obst, seed=SET_SEED)
    team = {}
    for a in range(A):
        torch.manual_seed(9 + 101 * a)
        team[a] = RNNAgentPPO(id=a, steps_per_episode=L, actor_critic_args=_args(*EVAL_WIDTHS))
        with torch.no_grad():
            for p in team[a].agent.pi.parameters():
                p.mul_(4.0)
    assert all(ag.agent.sized_policy and ag.agent.sized_pfgru for ag in team.values())
    run = lambda fused: run_test_environments_rnn_team(team, sets, montecarlo_runs=R, steps_per_episode=L, obstruction_count=obst,
                                                       seed=EVAL_SEED, return_actions=True, carry_hidden_across_runs=True, fused=fused)
    res_f, sum_f, act_f = run(True)
    res_c, sum_c, act_c = run(False)
    assert act_f.dtype == act_c.dtype == np.int8 and act_f.shape[1:] == act_c.shape[1:] == (E, A)
    common = min(act_f.shape[0], act_c.shape[0])
    assert np.array_equal(act_f[:common], act_c[:common]), np.argwhere(act_f[:common] != act_c[:common])[:6]
    assert (act_f[common:] == 8).all() and (act_c[common:] == 8).all()
    assert int(act_f.min()) >= 0 and (act_f < 8).any()
    assert sum_f["completed_runs"] == sum_c["completed_runs"] == E * R and len(res_f) == E
    V.same_records(res_f, res_c, R)
    assert sum_f["success_rate"] == sum_c["success_rate"]
    n_success = sum(r.success_counter for r in res_f)
    timed_out = sum(l == L for r in res_f for l in r.unsuccessful.episode_length)
    assert 0 < n_success < E * R and timed_out > 0, (n_success, timed_out)


# ------------------------------------------------------------------------------------------------------ end to end
def test_train_ppo_runs_a_recurrent_team_on_the_team_step(tmp_path):
    from radiation_ppo_amd.envs import RadSearchVec
    from radiation_ppo_amd.train import train_PPO
    env = RadSearchVec(64, number_agents=2, obstruction_count=0, enforce_grid_boundaries=True, seed=2)
    sim = train_PPO(env=env, logger_kwargs=dict(output_dir=str(tmp_path)), ppo_kwargs=dict(train_pi_iters=2, train_pfgru_iters=1), seed=2,
                    number_of_agents=2, actor_critic_architecture="rnn", global_critic_flag=False, steps_per_epoch=24, steps_per_episode=8,
                    total_epochs=2)
    assert sim.collector.use_team_step is True
    sim.train()
    assert env.error_flags() == 0
    for a in range(2):
        rows = sim.loggers[a].rows
        assert len(rows) == 2
        for r in rows:
            for k in ("loss_policy", "loss_critic", "loss_predictor", "kl_divergence", "Entropy", "MeanVVals"):
                assert np.isfinite(float(r[k])), (a, k, r[k])
