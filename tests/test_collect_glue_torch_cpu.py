"""The torch form of ppo.CollectGlue, without a GPU: pre / post_step / store_rows / post_reset on whole tensors against a plain-Python
transcription, env by env and agent by agent, of the four kernels they stand for (csrc/rs_welford.hip: rs_collect_pre_kernel,
rs_collect_post_step_kernel, rs_store_rows_kernel, rs_collect_post_reset_kernel), in the three configurations the collectors use, over a stub env
shaped like tests/test_collect_glue_cpu.py's.  Float fields bit for bit, counters exact, and what a call must not touch untouched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from radiation_ppo_amd import _lib
from radiation_ppo_amd.ppo import CollectGlue, DeviceWelford, RolloutBuffer

N, A, T, L, D = 5, 2, 4, 3, _lib.RS_OBS_DIM
T_NOW = 2                                                   # the buffer row the step writes
# env: 0 terminal only (one agent's latch), 1 timeout only, 2 both, 3 neither, 4 neither with a fresh Welford stream (count 0)
DONE = [[0, 1], [0, 0], [1, 1], [0, 0], [0, 0]]
STEPS = [0, L - 1, L - 1, 1, 0]
MARK = -77.0


def setup(seed, stat, team_reward, policy_input, bank, begun, complete_len):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    src = {"src_x": torch.randint(0, 2700, (1, N), generator=g, dtype=torch.int32), "src_y": torch.randint(0, 2700, (1, N), generator=g, dtype=torch.int32)}
    env = SimpleNamespace(obs=r(N, A, D), reward=r(N, A), team=r(N), done=torch.tensor(DONE, dtype=torch.uint8),
                          oob=(torch.rand(N, A, generator=g) < 0.5).to(torch.uint8), state=src.__getitem__)
    env.obs[..., 0] = torch.rand(N, A, generator=g) * 300.0
    c = SimpleNamespace(env=env, buf=RolloutBuffer(T, N, A, D, "cpu"), obs=r(N, A, D), ep_ret=r(N, A), steps_in_ep=torch.tensor(STEPS, dtype=torch.int32),
                        stat=None, bank=None, begun=None, complete_len=None)
    c.obs[..., 0] = torch.rand(N, A, generator=g) * 300.0
    for k in ("obs", "act", "rew", "val", "logp", "last_val", "source_tar"):
        getattr(c.buf, k).fill_(MARK)                                        # (act: int64 -77)
    c.buf.cut.fill_(9)
    if stat:
        c.stat = DeviceWelford((N, A), "cpu")
        c.stat.count.copy_(torch.randint(1, 6, (N, A), generator=g).double()); c.stat.count[4] = 0.0
        c.stat.mean.copy_(torch.rand(N, A, generator=g).double() * 200.0); c.stat.sq.copy_(torch.rand(N, A, generator=g).double() * 5000.0)
        c.stat.std.copy_(1.0 + torch.rand(N, A, generator=g).double() * 40.0)
    if bank:
        c.bank = SimpleNamespace(episode=torch.randint(1, 9, (N,), generator=g), calls=torch.randint(0, 5, (N,), generator=g))
    if begun:
        c.begun = torch.randint(1, 9, (N,), generator=g)
    if complete_len:
        c.complete_len = torch.randint(0, T_NOW + 1, (N,), generator=g)
    glue = CollectGlue(env, c.buf, c.obs, c.ep_ret, c.steps_in_ep, L, team_reward=team_reward, stat=c.stat, policy_input=policy_input, bank=c.bank,
                       episodes_begun=c.begun, complete_len=c.complete_len, impl="torch")
    assert glue.impl == "torch"
    glue.t.fill_(T_NOW)
    glue.k_act.copy_(torch.randint(0, 8, (A, N), generator=g)); glue.k_f.copy_(r(A, 3, N))
    for t in (glue.rew_used, glue.done_oob, glue.src_copy, glue.flags) + (() if glue.x is None else (glue.x, glue.xb)):
        t.fill_(7)                                                           # whatever an earlier step left
    return glue, c, g


def fields(glue, c):
    """every tensor a call may write, by name"""
    f = dict(obs=c.obs, ep_ret=c.ep_ret, steps_in_ep=c.steps_in_ep, rew_used=glue.rew_used, flags=glue.flags, done_oob=glue.done_oob,
             src_copy=glue.src_copy, t=glue.t, k_act=glue.k_act, k_f=glue.k_f, env_obs=c.env.obs, env_reward=c.env.reward, env_done=c.env.done,
             **{"buf_" + k: getattr(c.buf, k) for k in ("obs", "act", "rew", "val", "logp", "last_val", "cut", "source_tar")})
    if glue.x is not None:
        f.update(x=glue.x, xb=glue.xb)
    if c.stat is not None:
        f.update(w_count=c.stat.count, w_mean=c.stat.mean, w_sq=c.stat.sq, w_std=c.stat.std)
    if c.bank is not None:
        f.update(pf_episode=c.bank.episode, pf_calls=c.bank.calls)
    if c.begun is not None:
        f["begun"] = c.begun
    if c.complete_len is not None:
        f["complete_len"] = c.complete_len
    return f


def snapshot(glue, c):
    return {k: v.detach().clone().numpy() for k, v in fields(glue, c).items()}


def same(glue, c, want, what):
    got = snapshot(glue, c)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (what, k)


# ------------------------------------------------------------------------------------------------ the kernels, thread by thread
def standardized(s, n, a, reading):
    return np.float32((np.float64(reading) - s["w_mean"][n, a]) / s["w_std"][n, a])


def standardized_row(s, n, a, src, dst):
    dst[n, a, 1:] = src[n, a, 1:]
    dst[n, a, 0] = standardized(s, n, a, src[n, a, 0]) if "w_count" in s else src[n, a, 0]


def welford_push(s, n, a, x):
    x = np.float64(x)
    c, m = s["w_count"][n, a] + 1.0, s["w_mean"][n, a]
    s["w_count"][n, a] = c
    if c == 1.0:
        s["w_mean"][n, a] = x
        return
    mn = m + (x - m) / c
    sq = s["w_sq"][n, a] + (x - m) * (x - mn)
    s["w_mean"][n, a], s["w_sq"][n, a] = mn, sq
    s["w_std"][n, a] = max(np.sqrt(sq / max(c - 1.0, 1.0)), 1.0)


def ref_pre(s):
    for n in range(N):
        for a in range(A):
            standardized_row(s, n, a, s["obs"], s["x"])


def ref_post_step(s, env_team, env_oob, env_src, team_reward, epoch_ended):
    over, cut, boot = s["flags"]
    for n in range(N):
        terminal = False
        for a in range(A):
            r = env_team[n] if team_reward else s["env_reward"][n, a]
            s["rew_used"][n, a] = r
            s["ep_ret"][n, a] += r
            terminal = terminal or s["env_done"][n, a] != 0
            s["done_oob"][0, n, a], s["done_oob"][1, n, a] = s["env_done"][n, a], env_oob[n, a]
        s["src_copy"][0, n], s["src_copy"][1, n] = env_src[0][n], env_src[1][n]
        st = s["steps_in_ep"][n] + 1
        s["steps_in_ep"][n] = st
        timeout = st == L
        o = terminal or timeout
        c = True if epoch_ended else o
        over[n], cut[n], boot[n] = int(o), int(c), int(c if epoch_ended else timeout)
        if "complete_len" in s and o:
            s["complete_len"][n] = s["t"][0] + 1
        for a in range(A):
            if "w_count" in s:
                welford_push(s, n, a, s["env_obs"][n, a, 0])
            s["obs"][n, a] = s["env_obs"][n, a]
            if "xb" in s:
                standardized_row(s, n, a, s["env_obs"], s["xb"])
        if "pf_calls" in s:
            s["pf_calls"][n] += 1


def ref_store_rows(s, x):
    t = int(s["t"][0])
    for n in range(N):
        for a in range(A):
            s["buf_act"][t, n, a] = s["k_act"][a, n]
            s["buf_logp"][t, n, a], s["buf_val"][t, n, a] = s["k_f"][a, 0, n], s["k_f"][a, 1, n]
            s["buf_last_val"][t, n, a] = s["k_f"][a, 2, n] if s["flags"][2, n] else np.float32(0.0)
            s["buf_rew"][t, n, a] = s["rew_used"][n, a]
            s["buf_cut"][t, n, a] = 1 if s["flags"][1, n] else 0
            s["buf_obs"][t, n, a] = x[n, a]
        s["buf_source_tar"][t, n] = np.float32(s["src_copy"][0, n]), np.float32(s["src_copy"][1, n])


def ref_post_reset(s, reset_hidden):
    s["t"][0] += 1
    for n in range(N):
        if "pf_calls" in s and s["flags"][2, n]:
            s["pf_calls"][n] += 1
        if not s["flags"][1, n]:
            continue
        for a in range(A):
            s["obs"][n, a] = s["env_obs"][n, a]
            s["ep_ret"][n, a] = 0.0
            if "w_count" in s:
                s["w_count"][n, a], s["w_mean"][n, a], s["w_sq"][n, a], s["w_std"][n, a] = 1.0, np.float64(s["env_obs"][n, a, 0]), 0.0, 1.0
        s["steps_in_ep"][n] = 0
        if reset_hidden:
            for k in ("pf_episode", "begun"):
                if k in s:
                    s[k][n] += 1
            if "pf_calls" in s:
                s["pf_calls"][n] = 0


# ------------------------------------------------------------------------------------------------ the comparison
CONFIGS = {
    "ff": dict(stat=True, team_reward=False, policy_input=True, bank=False, begun=False, complete_len=False),
    "ff-raw": dict(stat=False, team_reward=False, policy_input=True, bank=False, begun=False, complete_len=False),
    "ff-team-reward": dict(stat=True, team_reward=True, policy_input=True, bank=False, begun=False, complete_len=False),
    "rnn": dict(stat=True, team_reward=False, policy_input=True, bank=True, begun=True, complete_len=False),
    "cnn": dict(stat=False, team_reward=True, policy_input=False, bank=True, begun=False, complete_len=True),
    "cnn-no-predictor": dict(stat=False, team_reward=True, policy_input=False, bank=False, begun=False, complete_len=True),
}


@pytest.mark.parametrize("reset_hidden", [True, False], ids=["reset-hidden", "keep-hidden"])
@pytest.mark.parametrize("epoch_ended", [False, True], ids=["mid-epoch", "epoch-end"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_torch_form_equals_the_kernels_transcribed(config, epoch_ended, reset_hidden):
    cfg = CONFIGS[config]
    glue, c, g = setup(11 + list(CONFIGS).index(config), **cfg)
    env = c.env
    outside = lambda: dict(team=env.team.clone(), oob=env.oob.clone(), src_x=env.state("src_x").clone(), src_y=env.state("src_y").clone())
    before_env = outside()
    s = snapshot(glue, c)
    if cfg["policy_input"]:
        ref_pre(s)
        glue.pre(None)
        same(glue, c, s, "pre")
    ref_post_step(s, env.team.numpy(), env.oob.numpy(), (env.state("src_x").numpy()[0], env.state("src_y").numpy()[0]), cfg["team_reward"], epoch_ended)
    glue.post_step(epoch_ended, None)
    same(glue, c, s, "post_step")
    over, cut, boot = (glue.flags[i].tolist() for i in range(3))
    assert over == [1, 1, 1, 0, 0] and cut == ([1] * N if epoch_ended else over) and boot == ([1] * N if epoch_ended else [0, 1, 1, 0, 0])
    x_own = torch.randn(N, A, D, generator=g)                                # a collector's own observation rows (CNNCollector)
    x = None if cfg["policy_input"] else x_own
    ref_store_rows(s, s["x"] if x is None else x.numpy())
    glue.store_rows(None, x)
    same(glue, c, s, "store_rows")
    for k in ("obs", "act", "rew", "val", "logp", "last_val", "source_tar"):
        rows = getattr(c.buf, k)
        assert bool((rows[[0, 1, 3]] == MARK).all()) and not bool((rows[T_NOW] == MARK).any()), k    # row t and no other
    # the env's reset: new observation rows for every env (the kernel must take those of the cut envs only)
    env.obs.copy_(torch.randn(N, A, D, generator=g)); env.obs[..., 0] = torch.rand(N, A, generator=g) * 300.0
    s["env_obs"] = env.obs.numpy().copy()
    obs_stepped = c.obs.clone()
    counters = {k: s[k].copy() for k in ("pf_episode", "begun") if k in s}
    ref_post_reset(s, reset_hidden)
    glue.post_reset(reset_hidden, None)
    same(glue, c, s, "post_reset")
    assert int(glue.t) == T_NOW + 1
    if not reset_hidden:
        for k, v in counters.items():
            assert np.array_equal(s[k], v), k
    if not epoch_ended:                                                      # envs 3 and 4 go on: their rows stay, the others are the reset's
        assert torch.equal(c.obs[3:], obs_stepped[3:]) and not torch.equal(c.obs[3:], env.obs[3:]) and torch.equal(c.obs[:3], env.obs[:3])
    after_env = outside()
    for k in before_env:                                                     # the glue reads the env's rows, never writes them
        assert torch.equal(before_env[k], after_env[k]), k
    assert torch.equal(env.reward, torch.from_numpy(s["env_reward"])) and torch.equal(env.done, torch.from_numpy(s["env_done"]))
