"""rs_ff_eval_step and rs_eval_post_step at the C boundary, without a GPU: every invalid argument is refused with RS_ERR_INVALID_ARG.
This machine has no device, so a refusal here proves that the validation runs before any HIP call: a launch would have come back as
RS_ERR_HIP.  (Their signatures, rs_eval_state's layout and their export: tests/test_abi_cpu.py.)"""
import ctypes as C

import pytest

from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


# a valid policy round over fake (never dereferenced) addresses, then one argument spoilt per case
STEP_GOOD = dict(actors=True, num_agents=2, obs=0x1000, w_mean=0x2000, w_std=0x3000, u=0x4000, alive=0x5000, act8=0x6000, num_envs=64)
STEP_CASES = [("actors NULL", dict(actors=False)), ("obs NULL", dict(obs=None)), ("u NULL", dict(u=None)), ("alive NULL", dict(alive=None)),
              ("act8 NULL", dict(act8=None)), ("w_mean alone NULL", dict(w_mean=None)), ("w_std alone NULL", dict(w_std=None)),
              ("no agent", dict(num_agents=0)), ("negative agents", dict(num_agents=-1)), ("nine agents", dict(num_agents=9)),
              ("no env", dict(num_envs=0)), ("negative envs", dict(num_envs=-5)),
              ("no statistics, obs NULL", dict(w_mean=None, w_std=None, obs=None))]


@pytest.mark.parametrize("name,spoil", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_eval_step_refuses_invalid_arguments_before_any_hip_call(lib, name, spoil):
    from radiation_ppo_amd import _lib
    a = dict(STEP_GOOD, **spoil)
    nets = (_lib.RsMlpParams * _lib.RS_MAX_AGENTS)()               # NULL pointers inside: the entry must not get as far as reading them
    rc = lib.rs_ff_eval_step(nets if a["actors"] else None, a["num_agents"], a["obs"], a["w_mean"], a["w_std"], a["u"], a["alive"],
                             a["act8"], a["num_envs"], None)
    assert rc == RS_ERR_INVALID_ARG, (name, rc)


POST_GOOD = dict(N=64, A=2, use_team_reward=0, env_obs=0x1000, env_reward=0x2000, env_team=0x3000, env_done=0x4000, cur_obs=0x5000,
                 w_count=0x6000, w_mean=0x7000, w_sq=0x8000, w_std=0x9000, alive=0xa000, success=0xb000, ep_len=0xc000, ep_ret=0xd000,
                 finished=0xe000)
REQUIRED = ("env_obs", "env_reward", "env_team", "env_done", "cur_obs", "alive", "success", "ep_len", "ep_ret", "finished")
WELFORD = ("w_count", "w_mean", "w_sq", "w_std")
POST_CASES = ([(f"{k} NULL", {k: None}) for k in REQUIRED]
              + [(f"{k} alone NULL", {k: None}) for k in WELFORD]
              + [(f"{k} alone set", {j: None for j in WELFORD if j != k}) for k in WELFORD]
              + [("no agent", dict(A=0)), ("negative agents", dict(A=-1)), ("nine agents", dict(A=9)), ("no lane", dict(N=0)),
                 ("negative lanes", dict(N=-3)), ("no statistics, cur_obs NULL", dict(w_count=None, w_mean=None, w_sq=None, w_std=None,
                                                                                        cur_obs=None))])


@pytest.mark.parametrize("name,spoil", POST_CASES, ids=[c[0] for c in POST_CASES])
def test_eval_post_step_refuses_invalid_arguments_before_any_hip_call(lib, name, spoil):
    from radiation_ppo_amd import _lib
    s = _lib.RsEvalState(**dict(POST_GOOD, **spoil))
    assert lib.rs_eval_post_step(C.byref(s), None) == RS_ERR_INVALID_ARG, name


def test_eval_post_step_refuses_a_null_struct(lib):
    assert lib.rs_eval_post_step(None, None) == RS_ERR_INVALID_ARG
