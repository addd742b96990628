"""The occupancy-aware tiled CNN trunk on the GPU, through the C ABI and maps.SizedConvTrunk: rs_cnn_sized_occupancy against the flag
rule of tests/_cnn_sized_occ_ref.py, rs_cnn_sized_forward_occ bit for bit against rs_cnn_sized_forward, rs_cnn_sized_backward_occ
against the float64 trunk with the dense kernels' own method and tolerances (tests/test_cnn_sized_trunk_gpu.py: _check_trunk, _close),
its determinism and refusals, and the walls-off collector's update with the flags on and off."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _cnn_sized_occ_ref as R  # noqa: E402
from test_cnn_sized_trunk_gpu import SEED, _check_trunk, _close, _modules, _walls_off_collector  # noqa: E402

pytestmark = pytest.mark.gpu

A, AGENT = 2, 1
SHAPES = [(M, S) for M in (34, 35, 64, 147, 148) for S in (1, 3, 67)] + [(8, 2)]


def _inputs(M, S):
    """the CPU test's images (M = 8 is one unit: the all-zero and the dense image only)"""
    kinds = ("zero", "dense") if M == 8 else R.KINDS
    return R.occ_inputs(M, S, A, AGENT, seed=M * 100 + S, kinds=kinds)


_K5 = {}


def _k5_maps():
    """K5's own maps at 147 x 147, built as in test_sized_trunk_on_walls_off_maps: 48 envs, 2 owners, 3 obstructions, 30 lock-steps"""
    if not _K5:
        import numpy as np
        from radiation_ppo_amd.envs import RadSearchVec
        from radiation_ppo_amd.maps import HeatMaps
        N, L = 48, 120
        env = RadSearchVec(N, number_agents=A, obstruction_count=3, enforce_grid_boundaries=False, seed=SEED)
        hm = HeatMaps(env, steps_per_episode=L, enforce_boundaries=False)
        assert hm.map_dimensions == (147, 147)
        obs = env.reset()[0]
        rng = np.random.default_rng(5)
        for t in range(30):
            pred = torch.rand(N, A, 2, generator=torch.Generator().manual_seed(t)).cuda() * 1.2
            hm.update(obs, pred)
            acts = rng.integers(0, 9, size=(N, A)).astype(np.int8)
            acts[: N // 2, 0] = 0
            obs = env.step(torch.from_numpy(acts).cuda())[0]
        hm.update(obs)
        _K5["v"] = (hm.shared_maps().clone(), hm.field("cell").long().contiguous(), hm.field("pred_cell").long().contiguous())
    return _K5["v"]


def _cases():
    for M, S in SHAPES:
        yield f"M={M} S={S}", M, tuple(t.cuda() for t in _inputs(M, S))
    yield "K5 maps", 147, _k5_maps()


def _forward(lib, name, seq, maps, cells, pcells, agent, flags=None):
    S, M = maps.shape[0], maps.shape[-1]
    P = M // 2
    out = (torch.full((S, 16 * P * P), float("nan"), device="cuda"), torch.full((S, P * P, 8), float("nan"), device="cuda"),
           torch.full((S, P * P, 8), 77, dtype=torch.uint8, device="cuda"), torch.full((S, P * P), -1, dtype=torch.int16, device="cuda"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [maps.data_ptr(), cells.data_ptr() if agent >= 0 else None, pcells.data_ptr() if agent >= 0 else None, cells.shape[1] if agent >= 0 else 0,
            agent, S, M, seq[0].weight.data_ptr(), seq[0].bias.data_ptr(), seq[3].weight.data_ptr(), seq[3].bias.data_ptr()]
    args += [t.data_ptr() for t in out]
    from radiation_ppo_amd import _lib
    if flags is None:
        _lib.check(lib.rs_cnn_sized_forward(*args, st), name)
    else:
        _lib.check(lib.rs_cnn_sized_forward_occ(*args, flags.data_ptr(), st), name)
    return out


def test_flags_equal_the_reference():
    from radiation_ppo_amd.maps import sized_occupancy
    for name, M, (maps, cells, pcells) in _cases():
        want = R.flags_ref(maps.cpu())
        got = sized_occupancy(maps)
        assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got.cpu(), want), name
    # a NaN is not equal to zero, -0.0 is: an image holding one NaN, one holding only -0.0, at two and at five tiles a side
    for M in (64, 147):
        maps = torch.zeros(3, 4, M, M)
        maps[0, 2, 40, 10] = float("nan")
        maps[1] = -0.0
        maps[2, 3, M - 1, M - 1] = 1e-30
        want = R.flags_ref(maps)
        assert int(want[0].sum()) == 1 and int(want[1].sum()) == 0 and int(want[2].sum()) == 1
        assert torch.equal(sized_occupancy(maps.cuda()).cpu(), want), M


def test_forward_occ_is_bit_identical_to_the_dense_forward():
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import sized_occupancy
    lib = _lib.load()
    for name, M, (maps, cells, pcells) in _cases():
        actor, critic = _modules(M, seed=M)
        flags = sized_occupancy(maps)
        for seq, agent in ((actor.actor, AGENT), (actor.actor, 0), (critic.critic, -1)):
            dense = _forward(lib, "rs_cnn_sized_forward", seq, maps, cells, pcells, agent)
            occ = _forward(lib, "rs_cnn_sized_forward_occ", seq, maps, cells, pcells, agent, flags)
            for k, x, y in zip(("a2", "p1", "amax", "relu_mask"), occ, dense):
                assert torch.equal(x, y), (name, agent, k)
        if name != "M=8 S=2":                      # the shortcut ran: some units are empty for the critic
            assert int((flags == 0).sum()) > 0, name


def _check_trunk_occ(seq, maps, cells, pcells, agent, name):
    """_check_trunk with SizedConvTrunk taking the flags: its apply() is given the trailing occ for the duration of the check"""
    from radiation_ppo_amd import maps as maps_mod
    from radiation_ppo_amd.maps import actor_stack_from, sized_occupancy
    flags = sized_occupancy(maps)
    dense64 = (actor_stack_from(maps, cells, pcells, agent) if agent >= 0 else maps).double().cpu()
    plain = maps_mod.SizedConvTrunk.apply
    calls = []

    def with_flags(*args):
        calls.append(1)
        return plain(*args, flags)
    maps_mod.SizedConvTrunk.apply = with_flags
    try:
        _check_trunk(seq, maps, cells, pcells, agent, dense64, name)
    finally:
        del maps_mod.SizedConvTrunk.apply
    assert calls and maps_mod.SizedConvTrunk.apply == plain


@pytest.mark.parametrize("M,S", SHAPES)
def test_backward_occ_matches_float64(M, S):
    from radiation_ppo_amd import _lib
    maps, cells, pcells = (t.cuda() for t in _inputs(M, S))
    actor, critic = _modules(M, seed=M * 100 + S)
    _lib.EVENTS = {}
    try:
        _check_trunk_occ(actor.actor, maps, cells, pcells, AGENT, f"occ actor M={M} S={S}")
        _check_trunk_occ(critic.critic, maps, None, None, -1, f"occ critic M={M} S={S}")
        names = dict((k, len(v)) for k, v in _lib.EVENTS.items())
    finally:
        _lib.EVENTS = None
    assert names.get("rs_cnn_sized_forward_occ") == 2 and names.get("rs_cnn_sized_backward_occ") == 2, names
    assert "rs_cnn_sized_backward" not in names and "rs_cnn_sized_forward_train" not in names, names


def test_backward_occ_on_walls_off_maps():
    maps, cells, pcells = _k5_maps()
    actor, critic = _modules(147, seed=3)
    for a in range(A):
        _check_trunk_occ(actor.actor, maps, cells, pcells, a, f"occ K5 maps a={a}")
    _check_trunk_occ(critic.critic, maps, None, None, -1, "occ K5 maps critic")


def test_backward_occ_is_deterministic_and_refuses_a_short_slab():
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.maps import sized_occupancy
    lib = _lib.load()
    M, S = 147, 67
    maps, cells, pcells = (t.cuda() for t in _inputs(M, S))
    actor, _ = _modules(M, seed=1)
    seq = actor.actor
    flags = sized_occupancy(maps)
    a2, p1, amax, mask = _forward(lib, "rs_cnn_sized_forward_occ", seq, maps, cells, pcells, AGENT, flags)
    da2 = torch.randn_like(a2)
    rows = lib.rs_cnn_sized_slab_rows(S, M, 6)
    assert rows > 1
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(slab, n, fl):
        return lib.rs_cnn_sized_backward_occ(maps.data_ptr(), cells.data_ptr(), pcells.data_ptr(), A, AGENT, S, M, seq[3].weight.data_ptr(),
                                             da2.data_ptr(), mask.data_ptr(), p1.data_ptr(), amax.data_ptr(), slab.data_ptr(), n, fl, st)
    slabs = []
    for _ in range(2):
        slab = torch.full((rows, lib.rs_cnn_sized_slab_row(6)), float("nan"), device="cuda")
        _lib.check(call(slab, rows, flags.data_ptr()), "rs_cnn_sized_backward_occ")
        slabs.append(slab)
    assert torch.isfinite(slabs[0]).all() and torch.equal(slabs[0], slabs[1])
    assert call(slabs[0], rows - 1, flags.data_ptr()) == 1           # a slab with fewer rows than workgroups, as the dense entry
    assert call(slabs[0], rows, None) == 1                           # no flags
    # and the summed slab is the dense entry's to float32 summation order
    dense = torch.empty_like(slabs[0])
    _lib.check(lib.rs_cnn_sized_backward(maps.data_ptr(), cells.data_ptr(), pcells.data_ptr(), A, AGENT, S, M, seq[3].weight.data_ptr(),
                                         da2.data_ptr(), mask.data_ptr(), p1.data_ptr(), amax.data_ptr(), dense.data_ptr(), rows, st))
    _close(slabs[0].sum(dim=0), dense.double().sum(dim=0).cpu(), "occ slab against the dense slab", noise=1e-4)


def test_collector_update_with_and_without_the_flags():
    """One collect() + update() of the 31 x 31 walls-off collector with use_occupancy on and off, SGD in place of Adam (so that the
    comparison measures the gradients, as in test_walls_off_update_equals_the_library_path): the parameters agree to its bound; the
    update with the flags calls the occupancy pass once and the _occ entries, the one without calls neither."""
    from radiation_ppo_amd import _lib
    params, names = [], []
    for use in (True, False):
        col, agents = _walls_off_collector(N=16, A=2, T=8, L=4)
        assert col.maps.map_dimensions == (31, 31) and col.use_occupancy
        col.use_occupancy = use
        gc = agents[0].critic
        sgd = torch.optim.SGD(gc.parameters(), lr=0.05)
        for ag in agents.values():
            ag.pi_optimizer = torch.optim.SGD(ag.pi.parameters(), lr=0.05)
            ag.critic_optimizer = sgd
        start = [p.detach().clone() for ag in agents.values() for p in ag.pi.parameters()] + [p.detach().clone() for p in gc.parameters()]
        col.collect()
        _lib.EVENTS = {}
        try:
            col.update()
            names.append(dict((k, len(v)) for k, v in _lib.EVENTS.items()))
        finally:
            _lib.EVENTS = None
        params.append([p.detach().clone() for ag in agents.values() for p in ag.pi.parameters()] + [p.detach().clone() for p in gc.parameters()])
    on, off = names
    assert on.get("rs_cnn_sized_occupancy") == 1 and on.get("rs_cnn_sized_forward_occ", 0) > 0, on
    assert on["rs_cnn_sized_backward_occ"] == on["rs_cnn_sized_forward_occ"] and "rs_cnn_sized_backward" not in on, on
    assert not any(k.endswith("_occ") or k == "rs_cnn_sized_occupancy" for k in off) and off.get("rs_cnn_sized_backward", 0) > 0, off
    for x, y in zip(*params):
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-6), float((x - y).abs().max())
    assert any(not torch.equal(x, y) for x, y in zip(start, params[0]))         # the updates changed the parameters they are compared on
