"""rs_cnn_sized_team_step_head, rs_cnn_sized_team_critic_infer and the two scratch functions without a GPU (their signatures and
their export: tests/test_abi_cpu.py): the slice length and the scratch size follow their
contract; every invalid argument is refused before any HIP call (this machine has no device: a launch would have come back as
RS_ERR_HIP)."""
import pytest

from radiation_ppo_amd._lib import RS_ERR_INVALID_ARG, RS_ERR_UNSUPPORTED, RS_OK

FLAT = 16 * 73 * 73


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


def test_slice_length_and_scratch_size(lib):
    sl = lib.rs_cnn_sized_team_head_slice_floats()
    assert sl > 0 and sl % 128 == 0
    for p in (4, 5, 15, 16, 73, 127, 128):
        flat = 16 * p * p
        for rows, N in ((1, 1), (2, 512), (16, 65), (4, 130)):
            assert lib.rs_cnn_sized_team_head_scratch_floats(flat, rows, N) == rows * -(-flat // sl) * N * 32, (p, rows, N)
    for flat in (0, -16, 16 * 9, 2704 + 16, 16 * 129 * 129, 16 * 73 * 73 + 16, 255, 257):
        assert lib.rs_cnn_sized_team_head_scratch_floats(flat, 2, 64) == 0, flat
    assert lib.rs_cnn_sized_team_head_scratch_floats(16 * 128 * 128, 16, 1 << 20) > 1 << 32        # an int64 result


def _heads(n, null_at=None):
    from radiation_ppo_amd import _lib
    rows = []
    for i in range(n):
        f = [0x10000 * (i + 1) + 0x100 * k for k in range(6)]
        if null_at is not None and null_at[0] == i:
            f[null_at[1]] = None
        rows.append(_lib.RsCnnHeadParams(*f))
    return (_lib.RsCnnHeadParams * n)(*rows)


GOOD = dict(actors=True, num_agents=3, critics=True, num_critics=3, flat=FLAT, a2_actor=0x1000, a2_critic=0x2000, u=0x3000, act=0x4000,
            f=0x5000, act8=0x6000, mask=None, y1_out=None, scratch=0x8000, scratch_floats=None, num_envs=64)
BOOT = dict(GOOD, actors=False, a2_actor=None, u=None, act=None, act8=None, mask=0x7000)
CASES = ([(f"step round, {k} NULL", GOOD, {k: None}) for k in ("a2_actor", "a2_critic", "act", "f", "act8", "scratch")]
         + [("step round, actors NULL", GOOD, dict(actors=False)), ("step round, critics NULL", GOOD, dict(critics=False)),
            ("no agent", GOOD, dict(num_agents=0, num_critics=1)), ("negative agents", GOOD, dict(num_agents=-1)),
            ("nine agents", GOOD, dict(num_agents=9, num_critics=9)), ("two critics for three agents", GOOD, dict(num_critics=2)),
            ("no critic", GOOD, dict(num_critics=0)), ("four critics for three agents", GOOD, dict(num_critics=4)),
            ("no env", GOOD, dict(num_envs=0)), ("negative envs", GOOD, dict(num_envs=-3)),
            ("16 short of a depth", GOOD, dict(flat=FLAT - 16)), ("p = 3", GOOD, dict(flat=144)), ("p = 129", GOOD, dict(flat=16 * 129 * 129)),
            ("flat 0", GOOD, dict(flat=0)), ("flat off by 16", GOOD, dict(flat=FLAT + 16)),
            ("scratch one float short", GOOD, dict(scratch_floats=-1)), ("scratch of the bootstrap round's size", GOOD, dict(scratch_floats=-2)),
            ("no scratch floats", GOOD, dict(scratch_floats=0)),
            ("bootstrap round without mask", BOOT, dict(mask=None)), ("bootstrap round without rows", BOOT, dict(f=None)),
            ("bootstrap round, critics NULL", BOOT, dict(critics=False)), ("bootstrap round, a2_critic NULL", BOOT, dict(a2_critic=None)),
            ("bootstrap round, no env", BOOT, dict(num_envs=0)), ("bootstrap round, scratch NULL", BOOT, dict(scratch=None)),
            ("bootstrap round, scratch one float short", BOOT, dict(scratch_floats=-1)), ("bootstrap round, bad flat", BOOT, dict(flat=FLAT + 16))])


def _call(lib, a, actors=None, critics=None):
    actors = actors if actors is not None else (_heads(8) if a["actors"] else None)
    critics = critics if critics is not None else (_heads(8) if a["critics"] else None)
    step = a["u"] is not None
    rows = a["num_agents"] + a["num_critics"] if step else a["num_critics"]
    need = lib.rs_cnn_sized_team_head_scratch_floats(FLAT, max(rows, 1), max(a["num_envs"], 1))
    sf = a["scratch_floats"]
    if sf is None:
        sf = need
    elif sf == -1:
        sf = need - 1
    elif sf == -2:                                                    # what the critic rows alone would need
        sf = lib.rs_cnn_sized_team_head_scratch_floats(FLAT, a["num_critics"], a["num_envs"])
    return lib.rs_cnn_sized_team_step_head(actors, a["num_agents"], critics, a["num_critics"], a["flat"], a["a2_actor"], a["a2_critic"], a["u"],
                                           a["act"], a["f"], a["act8"], a["mask"], a["y1_out"], a["scratch"], sf, a["num_envs"], None)


@pytest.mark.parametrize("name,base,spoil", CASES, ids=[c[0] for c in CASES])
def test_step_head_refuses_invalid_arguments_before_any_hip_call(lib, name, base, spoil):
    assert _call(lib, dict(base, **spoil)) == RS_ERR_INVALID_ARG, name


@pytest.mark.parametrize("field", range(6))
def test_step_head_refuses_a_null_pointer_inside_a_struct(lib, field):
    assert _call(lib, GOOD, actors=_heads(3, null_at=(2, field))) == RS_ERR_INVALID_ARG
    assert _call(lib, GOOD, critics=_heads(3, null_at=(1, field))) == RS_ERR_INVALID_ARG
    assert _call(lib, dict(GOOD, num_critics=1), critics=_heads(1, null_at=(0, field))) == RS_ERR_INVALID_ARG
    assert _call(lib, BOOT, critics=_heads(3, null_at=(2, field))) == RS_ERR_INVALID_ARG


def _convs(n, null_at=None):
    from radiation_ppo_amd import _lib
    rows = []
    for i in range(n):
        f = [0x10000 * (i + 1) + 0x100 * k for k in range(4)]
        if null_at is not None and null_at[0] == i:
            f[null_at[1]] = None
        rows.append(_lib.RsCnnConvParams(*f))
    return (_lib.RsCnnConvParams * n)(*rows)


TRUNK_GOOD = dict(maps=0x1000, num_critics=3, num_samples=64, map_side=147, convs=True, a2=0x3000)
TRUNK_CASES = ([(f"{k} NULL", {k: None}, RS_ERR_INVALID_ARG) for k in ("maps", "a2")]
               + [("convs NULL", dict(convs=False), RS_ERR_INVALID_ARG), ("no critic", dict(num_critics=0), RS_ERR_INVALID_ARG),
                  ("negative critics", dict(num_critics=-2), RS_ERR_INVALID_ARG), ("nine critics", dict(num_critics=9), RS_ERR_INVALID_ARG),
                  ("negative samples", dict(num_samples=-1), RS_ERR_INVALID_ARG),
                  ("no sample, a2 NULL", dict(num_samples=0, a2=None), RS_ERR_INVALID_ARG),
                  ("bad side, maps NULL", dict(map_side=7, maps=None), RS_ERR_INVALID_ARG)]
               + [(f"side {m}", dict(map_side=m), RS_ERR_UNSUPPORTED) for m in (7, 257, 0, -3)]
               + [("side 7, no sample", dict(map_side=7, num_samples=0), RS_ERR_UNSUPPORTED)])


@pytest.mark.parametrize("name,spoil,want", TRUNK_CASES, ids=[c[0] for c in TRUNK_CASES])
def test_critic_team_trunk_refuses_invalid_arguments_before_any_hip_call(lib, name, spoil, want):
    a = dict(TRUNK_GOOD, **spoil)
    convs = _convs(8) if a["convs"] else None
    assert lib.rs_cnn_sized_team_critic_infer(a["maps"], a["num_critics"], a["num_samples"], a["map_side"], convs, a["a2"], None) == want


@pytest.mark.parametrize("field", range(4))
def test_critic_team_trunk_refuses_a_null_pointer_inside_a_struct(lib, field):
    a = TRUNK_GOOD
    assert lib.rs_cnn_sized_team_critic_infer(a["maps"], 3, a["num_samples"], 147, _convs(3, null_at=(2, field)), a["a2"], None) == RS_ERR_INVALID_ARG
    assert lib.rs_cnn_sized_team_critic_infer(a["maps"], 1, a["num_samples"], 147, _convs(1, null_at=(0, field)), a["a2"], None) == RS_ERR_INVALID_ARG


def test_critic_team_trunk_with_no_sample_is_ok_and_launches_nothing(lib):
    a = TRUNK_GOOD
    for side in (8, 147, 256):
        assert lib.rs_cnn_sized_team_critic_infer(a["maps"], a["num_critics"], 0, side, _convs(3), a["a2"], None) == RS_OK
