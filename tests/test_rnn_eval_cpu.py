"""rs_rnn_eval_post_step and rs_rnn_eval_post_refresh at the C boundary, without a GPU: every invalid argument is refused with
RS_ERR_INVALID_ARG.  This machine has no device, so a refusal here proves that the validation runs before any HIP call: a launch would
have come back as RS_ERR_HIP.  (Their signatures, rs_rnn_eval_state's layout and their export: tests/test_abi_cpu.py.)"""
import ctypes as C

import pytest

from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG

ENTRIES = ("rs_rnn_eval_post_step", "rs_rnn_eval_post_refresh")


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


# a valid state over fake (never dereferenced) addresses, then one field spoilt per case
REQUIRED = ("env_obs", "env_reward", "env_done", "cur_obs", "x", "w_count", "w_mean", "w_sq", "w_std", "active", "again", "run", "steps", "ret",
            "rec_len", "rec_ret", "rec_suc", "finished")
OPTIONAL = ("pf_calls", "idle_act8")
GOOD = dict(N=64, runs_per_lane=3, steps_per_episode=30, **{k: 0x1000 * (i + 1) for i, k in enumerate(REQUIRED + OPTIONAL)})
CASES = ([(f"{k} NULL", {k: None}) for k in REQUIRED]
         + [("no lane", dict(N=0)), ("negative lanes", dict(N=-3)), ("no run", dict(runs_per_lane=0)), ("negative runs", dict(runs_per_lane=-1)),
            ("no step", dict(steps_per_episode=0)), ("negative steps", dict(steps_per_episode=-120)),
            ("optional pointers NULL, ret NULL", dict(pf_calls=None, idle_act8=None, ret=None))])


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,spoil", CASES, ids=[c[0] for c in CASES])
def test_entries_refuse_invalid_arguments_before_any_hip_call(lib, entry, name, spoil):
    from radiation_ppo_amd import _lib
    s = _lib.RsRnnEvalState(**dict(GOOD, **spoil))
    assert getattr(lib, entry)(C.byref(s), None) == RS_ERR_INVALID_ARG, name


@pytest.mark.parametrize("entry", ENTRIES)
def test_entries_refuse_a_null_struct(lib, entry):
    assert getattr(lib, entry)(None, None) == RS_ERR_INVALID_ARG
