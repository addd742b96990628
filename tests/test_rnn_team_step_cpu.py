"""rs_rnn_team_step and rs_rnn_sized_team_step at the C boundary, without a GPU: every invalid argument is refused -- RS_ERR_INVALID_ARG
or, for widths the sized kernels do not serve, RS_ERR_UNSUPPORTED.  This machine has no device, so a refusal here proves that the
validation runs before any HIP call: a launch would have come back as RS_ERR_HIP.  (Their signatures and their export:
tests/test_abi_cpu.py.)"""
import ctypes as C

import pytest

from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG, RS_ERR_UNSUPPORTED

ENTRIES = ("rs_rnn_team_step", "rs_rnn_sized_team_step")


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


def _weights(A, null_at=None):
    return (C.c_void_p * 8)(*[None if a == null_at or a >= A else 0x100000 * (a + 1) for a in range(8)])


# non-NULL stand-ins that are never dereferenced; one argument spoilt per case
GOOD = dict(weights=_weights(3), A=3, x=0x1000, loc=0x2000, h=0x3000, u=0x4000, act=0x5000, f=0x6000, act8=0x7000, mask=0x8000, N=70)
CASES = ([(f"{k} NULL", {k: None}) for k in ("weights", "x", "loc", "h")]
         + [(f"weight {a} of 3 NULL", dict(weights=_weights(3, null_at=a))) for a in range(3)]
         + [("no agent", dict(A=0)), ("nine agents", dict(A=9, weights=(C.c_void_p * 9)(*[0x100000] * 9))), ("negative agents", dict(A=-2)),
            ("no env", dict(N=0)), ("negative envs", dict(N=-64)),
            ("step round with neither act nor act8", dict(act=None, act8=None)),
            ("step round with neither act nor act8, no value either", dict(act=None, act8=None, f=None)),
            ("bootstrap round without logp_val_boot", dict(u=None, f=None)),
            ("bootstrap round without logp_val_boot or actions", dict(u=None, f=None, act=None, act8=None))])


def _call(lib, entry, a, widths=(32, 64, 64)):
    tail = (a["x"], a["loc"], a["h"], a["u"], a["act"], a["f"], a["act8"], a["mask"], a["N"], None)
    if entry == "rs_rnn_team_step":
        return lib.rs_rnn_team_step(a["weights"], a["A"], *tail)
    return lib.rs_rnn_sized_team_step(a["weights"], a["A"], *widths, *tail)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name,spoil", CASES, ids=[c[0] for c in CASES])
def test_invalid_arguments_are_refused_before_any_hip_call(lib, entry, name, spoil):
    assert _call(lib, entry, dict(GOOD, **spoil)) == RS_ERR_INVALID_ARG, name


@pytest.mark.parametrize("widths", [(0, 32, 32), (65, 32, 32), (32, 1, 32), (32, 65, 32), (32, 32, 1), (32, 32, 65), (-1, -1, -1)])
def test_the_sized_entry_refuses_widths_it_does_not_serve(lib, widths):
    """as rs_rnn_sized_step: the widths are looked at first, so the answer is 4 with valid and with invalid other arguments"""
    assert _call(lib, "rs_rnn_sized_team_step", GOOD, widths) == RS_ERR_UNSUPPORTED
    assert _call(lib, "rs_rnn_sized_team_step", dict(GOOD, x=None), widths) == RS_ERR_UNSUPPORTED
