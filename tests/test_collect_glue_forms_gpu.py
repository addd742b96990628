"""The two forms of ppo.CollectGlue held to each other on the GPU: pre / post_step / store_rows / post_reset as one launch each (impl "hip")
and as their whole-tensor transcription (impl "torch") on two copies of one random state, every field bit for bit after every call.
N = 257 envs (two 256-thread blocks, the second with one live thread; rs_collect_pre and rs_store_rows run over N * A = 771 = three full
blocks and three threads) and A = 3; once as RNNCollector builds the glue (statistics, predictor bank, episodes_begun) and once as
CNNCollector does (complete_len, team reward, no policy input).  The torch form itself is held to the kernels' text on the CPU
(tests/test_collect_glue_torch_cpu.py)."""
from types import SimpleNamespace

import pytest
import torch

from radiation_ppo_amd import _lib
from radiation_ppo_amd.ppo import CollectGlue, DeviceWelford, RolloutBuffer

pytestmark = pytest.mark.gpu
N, A, T, L, D = 257, 3, 4, 5, _lib.RS_OBS_DIM


def state(seed, rnn):
    """everything a glue is built over, on the CPU, by name"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    readings = lambda: torch.rand(N, A, generator=g) * 300.0
    s = dict(env_obs=r(N, A, D), env_reward=r(N, A), env_team=r(N), env_done=(torch.rand(N, A, generator=g) < 0.15).to(torch.uint8),
             env_oob=(torch.rand(N, A, generator=g) < 0.5).to(torch.uint8), src_x=torch.randint(0, 2700, (1, N), generator=g, dtype=torch.int32),
             src_y=torch.randint(0, 2700, (1, N), generator=g, dtype=torch.int32), obs=r(N, A, D), ep_ret=r(N, A),
             steps_in_ep=torch.randint(0, L, (N,), generator=g, dtype=torch.int32), t=torch.full((1,), 2, dtype=torch.int64),
             k_act=torch.randint(0, 8, (A, N), generator=g), k_f=r(A, 3, N), x_own=r(N, A, D),
             pf_episode=torch.randint(1, 9, (N,), generator=g), pf_calls=torch.randint(0, 5, (N,), generator=g))
    s["env_obs"][..., 0], s["obs"][..., 0] = readings(), readings()
    if rnn:
        s.update(w_count=torch.randint(0, 6, (N, A), generator=g).double(), w_mean=readings().double(), w_sq=torch.rand(N, A, generator=g).double() * 5000.0,
                 w_std=1.0 + torch.rand(N, A, generator=g).double() * 40.0, begun=torch.randint(1, 9, (N,), generator=g))
    else:
        s["complete_len"] = torch.randint(0, 3, (N,), generator=g)
    return s, g


def build(s, rnn, impl):
    """(glue, every tensor a call may read or write by name) over a cuda copy of the state"""
    d = {k: v.cuda() for k, v in s.items()}
    fields = {"src_x": d["src_x"], "src_y": d["src_y"]}
    env = SimpleNamespace(obs=d["env_obs"], reward=d["env_reward"], team=d["env_team"], done=d["env_done"], oob=d["env_oob"], state=fields.__getitem__)
    buf = RolloutBuffer(T, N, A, D, "cuda")
    bank = SimpleNamespace(episode=d["pf_episode"], calls=d["pf_calls"])
    stat = None
    if rnn:
        stat = DeviceWelford((N, A), "cuda")
        for k in ("count", "mean", "sq", "std"):
            getattr(stat, k).copy_(d["w_" + k])
            d["w_" + k] = getattr(stat, k)
    glue = CollectGlue(env, buf, d["obs"], d["ep_ret"], d["steps_in_ep"], L, team_reward=not rnn, stat=stat, policy_input=rnn, bank=bank,
                       episodes_begun=d.get("begun"), complete_len=d.get("complete_len"), t=d["t"], impl=impl)
    assert glue.impl == impl
    glue.k_act.copy_(d["k_act"]); glue.k_f.copy_(d["k_f"])
    d.update(k_act=glue.k_act, k_f=glue.k_f, rew_used=glue.rew_used, flags=glue.flags, done_oob=glue.done_oob, src_copy=glue.src_copy,
             **{"buf_" + k: getattr(buf, k) for k in ("obs", "act", "rew", "val", "logp", "last_val", "cut", "source_tar")})
    if rnn:
        d.update(x=glue.x, xb=glue.xb)
    return glue, d


@pytest.mark.parametrize("epoch_ended", [False, True], ids=["mid-epoch", "epoch-end"])
@pytest.mark.parametrize("rnn", [True, False], ids=["statistics-bank-begun", "complete_len-team-reward"])
def test_the_two_forms_of_every_glue_call_are_bit_identical(rnn, epoch_ended):
    s, g = state(5 + int(rnn), rnn)
    (hip, dh), (tor, dt) = build(s, rnn, "hip"), build(s, rnn, "torch")
    after_reset = torch.randn(N, A, D, generator=g)
    after_reset[..., 0] = torch.rand(N, A, generator=g) * 300.0

    def same(what):
        torch.cuda.synchronize()
        assert sorted(dh) == sorted(dt)
        for k in dh:
            assert dh[k].dtype == dt[k].dtype and torch.equal(dh[k], dt[k]), (what, k)

    same("the state")
    if rnn:
        for glue in (hip, tor):
            glue.pre(glue.stream())
        same("pre")
    for glue in (hip, tor):
        glue.post_step(epoch_ended, glue.stream())
    same("post_step")
    cut = dh["flags"][1].bool()
    assert bool(cut.all()) if epoch_ended else (bool(cut.any()) and not bool(cut.all()))
    assert bool(dh["flags"][2].any()) and (epoch_ended or not torch.equal(dh["flags"][2], dh["flags"][1]))          # timeouts, and pure terminals
    for glue, d in ((hip, dh), (tor, dt)):
        glue.store_rows(glue.stream(), None if rnn else d["x_own"])
    same("store_rows")
    assert float(dh["buf_last_val"][2].abs().sum()) > 0 and float(dh["buf_obs"][[0, 1, 3]].abs().sum()) == 0          # row t and no other
    for glue, d in ((hip, dh), (tor, dt)):
        d["env_obs"].copy_(after_reset.cuda())                               # the env's reset: new rows everywhere, the glue takes the cut envs'
        glue.post_reset(not epoch_ended if rnn else True, glue.stream())      # as the collectors call it
    same("post_reset")
    assert int(dh["t"]) == 3 and (epoch_ended or not torch.equal(dh["obs"], dh["env_obs"]))
