"""rs_cnn_team_step_head and rs_cnn_team_critic_trunk_infer without a GPU: every invalid argument is refused with RS_ERR_INVALID_ARG
before any HIP call (this machine has no device: a launch would have come back as RS_ERR_HIP).  (Their signatures and their export:
tests/test_abi_cpu.py.)"""
import pytest

from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG, RS_OK


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


def _heads(n, null_at=None):
    from radiation_ppo_amd import _lib
    rows = []
    for i in range(n):
        f = [0x10000 * (i + 1) + 0x100 * k for k in range(6)]
        if null_at is not None and null_at[0] == i:
            f[null_at[1]] = None
        rows.append(_lib.RsCnnHeadParams(*f))
    return (_lib.RsCnnHeadParams * n)(*rows)


GOOD = dict(actors=True, num_agents=3, critics=True, num_critics=3, a2_actor=0x1000, a2_critic=0x2000, u=0x3000, act=0x4000, f=0x5000,
            act8=0x6000, mask=None, y1_out=None, num_envs=64)
BOOT = dict(GOOD, actors=False, a2_actor=None, u=None, act=None, act8=None, mask=0x7000)
CASES = ([(f"step round, {k} NULL", GOOD, {k: None}) for k in ("a2_actor", "a2_critic", "act", "f", "act8")]
         + [("step round, actors NULL", GOOD, dict(actors=False)), ("step round, critics NULL", GOOD, dict(critics=False)),
            ("no agent", GOOD, dict(num_agents=0, num_critics=1)), ("negative agents", GOOD, dict(num_agents=-1)),
            ("nine agents", GOOD, dict(num_agents=9, num_critics=9)), ("two critics for three agents", GOOD, dict(num_critics=2)),
            ("no critic", GOOD, dict(num_critics=0)), ("four critics for three agents", GOOD, dict(num_critics=4)),
            ("no env", GOOD, dict(num_envs=0)), ("negative envs", GOOD, dict(num_envs=-3)),
            ("bootstrap round without mask", BOOT, dict(mask=None)), ("bootstrap round without rows", BOOT, dict(f=None)),
            ("bootstrap round, critics NULL", BOOT, dict(critics=False)), ("bootstrap round, a2_critic NULL", BOOT, dict(a2_critic=None)),
            ("bootstrap round, no env", BOOT, dict(num_envs=0))])


def _call(lib, a, actors=None, critics=None):
    actors = actors if actors is not None else (_heads(8) if a["actors"] else None)
    critics = critics if critics is not None else (_heads(8) if a["critics"] else None)
    return lib.rs_cnn_team_step_head(actors, a["num_agents"], critics, a["num_critics"], a["a2_actor"], a["a2_critic"], a["u"], a["act"], a["f"],
                                     a["act8"], a["mask"], a["y1_out"], a["num_envs"], None)


@pytest.mark.parametrize("name,base,spoil", CASES, ids=[c[0] for c in CASES])
def test_step_head_refuses_invalid_arguments_before_any_hip_call(lib, name, base, spoil):
    assert _call(lib, dict(base, **spoil)) == RS_ERR_INVALID_ARG, name


@pytest.mark.parametrize("field", range(6))
def test_step_head_refuses_a_null_pointer_inside_a_struct(lib, field):
    assert _call(lib, GOOD, actors=_heads(3, null_at=(2, field))) == RS_ERR_INVALID_ARG
    assert _call(lib, GOOD, critics=_heads(3, null_at=(1, field))) == RS_ERR_INVALID_ARG
    assert _call(lib, dict(GOOD, num_critics=1), critics=_heads(1, null_at=(0, field))) == RS_ERR_INVALID_ARG
    assert _call(lib, BOOT, critics=_heads(3, null_at=(2, field))) == RS_ERR_INVALID_ARG


TRUNK_GOOD = dict(maps=0x1000, num_critics=3, num_samples=64, wscratch=0x2000, a2=0x3000)
TRUNK_CASES = ([(f"{k} NULL", {k: None}) for k in ("maps", "wscratch", "a2")]
               + [("no critic", dict(num_critics=0)), ("negative critics", dict(num_critics=-2)), ("nine critics", dict(num_critics=9)),
                  ("negative samples", dict(num_samples=-1)), ("no sample, a2 NULL", dict(num_samples=0, a2=None))])


@pytest.mark.parametrize("name,spoil", TRUNK_CASES, ids=[c[0] for c in TRUNK_CASES])
def test_critic_team_trunk_refuses_invalid_arguments_before_any_hip_call(lib, name, spoil):
    a = dict(TRUNK_GOOD, **spoil)
    assert lib.rs_cnn_team_critic_trunk_infer(a["maps"], a["num_critics"], a["num_samples"], a["wscratch"], a["a2"], None) == RS_ERR_INVALID_ARG


def test_critic_team_trunk_with_no_sample_is_ok_and_launches_nothing(lib):
    a = TRUNK_GOOD
    assert lib.rs_cnn_team_critic_trunk_infer(a["maps"], a["num_critics"], 0, a["wscratch"], a["a2"], None) == RS_OK
