"""rs_rnn_team_eval_step, rs_rnn_team_eval_post_step and rs_rnn_team_eval_post_refresh at the C boundary, without a GPU: every
invalid argument is refused with RS_ERR_INVALID_ARG.  This machine has no device, so a refusal here proves that the validation runs
before any HIP call: a launch would have come back as RS_ERR_HIP.  (Their signatures, rs_rnn_team_eval_state's layout and their
export: tests/test_abi_cpu.py.)"""
import ctypes as C

import pytest

from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG

STATE_ENTRIES = ("rs_rnn_team_eval_post_step", "rs_rnn_team_eval_post_refresh")


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
GOOD = dict(N=64, A=2, runs_per_lane=3, steps_per_episode=30, **{k: 0x1000 * (i + 1) for i, k in enumerate(REQUIRED + OPTIONAL)})
CASES = ([(f"{k} NULL", {k: None}) for k in REQUIRED]
         + [("no lane", dict(N=0)), ("negative lanes", dict(N=-3)), ("no agent", dict(A=0)), ("nine agents", dict(A=9)),
            ("negative agents", dict(A=-1)), ("no run", dict(runs_per_lane=0)), ("negative runs", dict(runs_per_lane=-1)),
            ("no step", dict(steps_per_episode=0)), ("negative steps", dict(steps_per_episode=-120)),
            ("optional pointers NULL, ret NULL", dict(pf_calls=None, idle_act8=None, ret=None))])


@pytest.mark.parametrize("entry", STATE_ENTRIES)
@pytest.mark.parametrize("name,spoil", CASES, ids=[c[0] for c in CASES])
def test_state_entries_refuse_invalid_arguments_before_any_hip_call(lib, entry, name, spoil):
    from radiation_ppo_amd import _lib
    s = _lib.RsRnnTeamEvalState(**dict(GOOD, **spoil))
    assert getattr(lib, entry)(C.byref(s), None) == RS_ERR_INVALID_ARG, name


@pytest.mark.parametrize("entry", STATE_ENTRIES)
def test_state_entries_refuse_a_null_struct(lib, entry):
    assert getattr(lib, entry)(None, None) == RS_ERR_INVALID_ARG


# rs_rnn_team_eval_step(weights, A, x, loc, h, u, active, act8, N, stream)
def _weights(A, null_at=None):
    return (C.c_void_p * 8)(*[None if a == null_at or a >= A else 0x100000 * (a + 1) for a in range(8)])


STEP_GOOD = dict(weights=_weights(3), A=3, x=0x1000, loc=0x2000, h=0x3000, u=0x4000, active=0x5000, act8=0x6000, N=70)
STEP_CASES = ([(f"{k} NULL", {k: None}) for k in ("weights", "x", "loc", "h", "u", "active", "act8")]
              + [(f"weight {a} of 3 NULL", dict(weights=_weights(3, null_at=a))) for a in range(3)]
              + [("no agent", dict(A=0)), ("nine agents", dict(A=9, weights=(C.c_void_p * 9)(*[0x100000] * 9))), ("negative agents", dict(A=-2)),
                 ("no lane", dict(N=0)), ("negative lanes", dict(N=-64))])


@pytest.mark.parametrize("name,spoil", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_the_step_entry_refuses_invalid_arguments_before_any_hip_call(lib, name, spoil):
    a = dict(STEP_GOOD, **spoil)
    got = lib.rs_rnn_team_eval_step(a["weights"], a["A"], a["x"], a["loc"], a["h"], a["u"], a["active"], a["act8"], a["N"], None)
    assert got == RS_ERR_INVALID_ARG, name
