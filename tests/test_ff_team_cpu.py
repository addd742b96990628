"""rs_ff_team_step at the C boundary, without a GPU: every invalid argument is refused with RS_ERR_INVALID_ARG.  This machine has no
device, so a refusal here proves that the validation runs before any HIP call: a launch would have come back as RS_ERR_HIP.  (Its
signature and its export: tests/test_abi_cpu.py.)"""
import pytest


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


# a valid step round over fake (never dereferenced) addresses, then one argument spoilt per case
GOOD = dict(actors=True, critics=True, num_agents=2, x=0x1000, u=0x2000, act=0x3000, f=0x4000, act8=0x5000, mask=None, num_envs=64)
CASES = [("actors NULL", dict(actors=False)), ("critics NULL", dict(critics=False)), ("x NULL", dict(x=None)),
         ("logp_val_boot NULL", dict(f=None)), ("no agent", dict(num_agents=0)), ("negative agents", dict(num_agents=-1)),
         ("nine agents", dict(num_agents=9)), ("no env", dict(num_envs=0)), ("negative envs", dict(num_envs=-5)),
         ("step round without act", dict(act=None)),
         ("bootstrap round, x NULL", dict(u=None, act=None, act8=None, x=None)),
         ("bootstrap round, logp_val_boot NULL", dict(u=None, act=None, act8=None, f=None))]


@pytest.mark.parametrize("name,spoil", CASES, ids=[c[0] for c in CASES])
def test_invalid_arguments_are_refused_before_any_hip_call(lib, name, spoil):
    from radiation_ppo_amd import _lib
    a = dict(GOOD, **spoil)
    nets = (_lib.RsMlpParams * _lib.RS_MAX_AGENTS)()               # NULL pointers inside: the entry must not get as far as reading them
    rc = lib.rs_ff_team_step(nets if a["actors"] else None, nets if a["critics"] else None, a["num_agents"], a["x"], a["u"], a["act"], a["f"],
                             a["act8"], a["mask"], a["num_envs"], None)
    assert rc == _lib.RS_ERR_INVALID_ARG, (name, rc)
