"""CollectGlue's wiring, without a GPU: the rs_collect_state it builds over a stub env names, field by field, the tensor each kernel
must read or write, in the three configurations the collectors use; exactly the fields include/radsearch.h documents as optional for a
configuration are NULL; and building it loads no library.  A pointer in the wrong slot would be a silent wrong-buffer write on the
device, which only a GPU run could catch before."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from radiation_ppo_amd import _lib
from radiation_ppo_amd.ppo import CollectGlue, DeviceWelford, RolloutBuffer

N, A, T, L = 3, 2, 5, 4
POINTERS = [name for name, ctype in _lib.RsCollectState._fields_ if ctype is C.c_void_p]
INTEGERS = [name for name, ctype in _lib.RsCollectState._fields_ if ctype is not C.c_void_p]


def stub_env():
    fields = {"src_x": torch.zeros(N, dtype=torch.int32), "src_y": torch.zeros(N, dtype=torch.int32)}
    return SimpleNamespace(obs=torch.zeros(N, A, _lib.RS_OBS_DIM), reward=torch.zeros(N, A), team=torch.zeros(N),
                           done=torch.zeros(N, A, dtype=torch.uint8), oob=torch.zeros(N, A, dtype=torch.uint8), state=fields.__getitem__)


def build(monkeypatch, **varies):
    """(glue, what it was built from) with the library's cached handle unset around the construction."""
    monkeypatch.setattr(_lib, "_lib", None)
    c = SimpleNamespace(env=stub_env(), buf=RolloutBuffer(T, N, A, _lib.RS_OBS_DIM, "cpu"), obs=torch.zeros(N, A, _lib.RS_OBS_DIM),
                        ep_ret=torch.zeros(N, A), steps_in_ep=torch.zeros(N, dtype=torch.int32))
    g = CollectGlue(c.env, c.buf, c.obs, c.ep_ret, c.steps_in_ep, L, **varies)
    assert _lib._lib is None, "building the glue loaded the library"
    return g, c


def check(g, c, team_reward, named):
    """`named`: field -> tensor for the fields that vary; the rest is the same for every collector.  Every pointer field is compared:
    the ones in neither table must be NULL."""
    cs, env = g.cs, c.env
    assert INTEGERS == ["num_envs", "num_agents", "steps_per_episode", "team_reward"] and len(POINTERS) == 28
    assert (cs.num_envs, cs.num_agents, cs.steps_per_episode, cs.team_reward) == (N, A, L, team_reward)
    want = dict(env_obs=env.obs, env_reward=env.reward, env_team=env.team, env_done=env.done, obs=c.obs, ep_ret=c.ep_ret,
                steps_in_ep=c.steps_in_ep, reward_used=g.rew_used, over=g.flags[0], cut=g.flags[1], boot=g.flags[2], t=g.t, env_oob=env.oob,
                env_src_x=env.state("src_x"), env_src_y=env.state("src_y"), done_copy=g.done_oob[0], oob_copy=g.done_oob[1],
                src_copy=g.src_copy, **named)
    for name in POINTERS:
        got = getattr(cs, name)
        if name in want:
            assert got == want[name].data_ptr(), name
        else:
            assert got is None, f"{name} must be NULL in this configuration"
    assert len({t.data_ptr() for t in want.values()}) == len(want)          # no two fields share a buffer: the comparison can tell them apart
    # the views the lock-steps read are the rows the struct names, and the buffers have the kernels' shapes and types
    assert (g.over.data_ptr(), g.cut.data_ptr(), g.boot.data_ptr()) == (cs.over, cs.cut, cs.boot)
    assert (g.done.data_ptr(), g.oob.data_ptr()) == (cs.done_copy, cs.oob_copy)
    shapes = dict(flags=((3, N), torch.uint8), rew_used=((N, A), torch.float32), done_oob=((2, N, A), torch.uint8),
                  src_copy=((2, N), torch.int32), k_act=((A, N), torch.int64), k_f=((A, 3, N), torch.float32), t=((1,), torch.int64))
    for name, (shape, dtype) in shapes.items():
        t = getattr(g, name)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), name
    assert g.acc.oob.shape == (A,)


@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("team_reward", [False, True])
def test_feed_forward_team(monkeypatch, standardize, team_reward):
    """TeamCollector: the Welford state only with standardisation; no PFGRU, no GRU, no complete_len."""
    stat = DeviceWelford((N, A), "cpu")
    g, c = build(monkeypatch, team_reward=team_reward, stat=stat if standardize else None)
    named = dict(x=g.x, xb=g.xb)
    if standardize:
        named.update(w_count=stat.count, w_mean=stat.mean, w_sq=stat.sq, w_std=stat.std)
    check(g, c, int(team_reward), named)
    assert g.x.shape == g.xb.shape == (N, A, _lib.RS_OBS_DIM)


def test_rnn(monkeypatch):
    """RNNCollector: the predictor bank's draw counters and episodes_begun; no complete_len, never the team reward."""
    stat = DeviceWelford((N, A), "cpu")
    bank = SimpleNamespace(episode=torch.zeros(N, dtype=torch.int64), calls=torch.zeros(N, dtype=torch.int64))
    begun = torch.zeros(N, dtype=torch.int64)
    t = torch.zeros(1, dtype=torch.int64)                                    # the collector's own step counter, declared before start()
    g, c = build(monkeypatch, stat=stat, bank=bank, episodes_begun=begun, t=t)
    assert g.t is t
    check(g, c, 0, dict(x=g.x, xb=g.xb, w_count=stat.count, w_mean=stat.mean, w_sq=stat.sq, w_std=stat.std, pf_episode=bank.episode,
                        pf_calls=bank.calls, episodes_begun=begun))


@pytest.mark.parametrize("predictor", [True, False])
def test_cnn(monkeypatch, predictor):
    """CNNCollector: no statistics and no policy input (the networks read heat maps), complete_len, the predictor's counters if any."""
    bank = SimpleNamespace(episode=torch.zeros(N, dtype=torch.int64), calls=torch.zeros(N, dtype=torch.int64)) if predictor else None
    complete_len = torch.zeros(N, dtype=torch.int64)
    g, c = build(monkeypatch, team_reward=True, policy_input=False, bank=bank, complete_len=complete_len)
    named = dict(complete_len=complete_len)
    if predictor:
        named.update(pf_episode=bank.episode, pf_calls=bank.calls)
    check(g, c, 1, named)
    assert g.x is None and g.xb is None


def test_the_buffer_rows_are_the_rollout_buffers_own(monkeypatch):
    """store_rows' precomputed arguments: the glue's copies, then the buffer's eight pointers and N, A, T, in rs_store_rows' order."""
    g, c = build(monkeypatch)
    b, p = c.buf, lambda t: t.data_ptr()
    assert g._own_rows == (p(g.t), p(g.k_act), p(g.k_f), p(g.x), p(g.src_copy[0]), p(g.src_copy[1]), p(g.rew_used), p(g.cut), p(g.boot),
                           p(b.act), p(b.logp), p(b.val), p(b.last_val), p(b.obs), p(b.source_tar), p(b.rew), p(b.cut), N, A, T)
    other = torch.zeros(N, A, _lib.RS_OBS_DIM)
    assert g._rows(other)[3] == other.data_ptr() and g._rows(other)[:3] + g._rows(other)[4:] == g._own_rows[:3] + g._own_rows[4:]
