"""The cold draw kernels (csrc/rs_draws.hip) exist once, with the width as an argument; the default exports (24 units) and the
width-taking ones are wrappers around them.  Each default export against its twin at width 24, bit for bit, into sentinel-filled
buffers: a wrapper that passes its arguments in another order, or another width, shows here.  The sizes leave the last workgroup
partial; the rows a mask leaves out must keep the sentinel."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from radiation_ppo_amd import _lib  # noqa: E402

SENTINEL = -7.0
H = 24


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _keys(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2 ** 52, shape, dtype=torch.int64, generator=g).cuda()


def test_pfgru_reset_twins_are_bit_identical_and_masked():
    N, A = 7, 2
    lib = _lib.load()
    base, episode, calls = _keys(A, N, seed=1), _keys(N, seed=2) % 1000, _keys(N, seed=3) % 120
    mask = torch.tensor([1, 0, 1, 1, 0, 1, 0], dtype=torch.uint8, device="cuda")
    out = []
    for sized in (False, True):
        h = torch.full((A, N, H // 4, 40, 4), SENTINEL, device="cuda")
        p = torch.full((A, N, 40), SENTINEL, device="cuda")
        args = (h.data_ptr(), p.data_ptr(), base.data_ptr(), episode.data_ptr(), calls.data_ptr(), mask.data_ptr(), N, A)
        if sized:
            _lib.check(lib.rs_pfgru_sized_reset(*args, H, _stream()), "rs_pfgru_sized_reset")
        else:
            _lib.check(lib.rs_pfgru_reset(*args, _stream()), "rs_pfgru_reset")
        out.append((h, p))
    (h0, p0), (h1, p1) = out
    assert torch.equal(h0, h1) and torch.equal(p0, p1)
    m = mask.bool()
    assert bool((h0[:, ~m] == SENTINEL).all()) and bool((p0[:, ~m] == SENTINEL).all())
    assert bool(((h0[:, m] >= 0.0) & (h0[:, m] < 1.0)).all()) and bool((p0[:, m] < -3.0).all())


def test_pfgru_draws_twins_are_bit_identical():
    E, L = 3, 2
    lib = _lib.load()
    keys = _keys(E, seed=4)
    out = []
    for sized in (False, True):
        h0 = torch.full((E, 40, H), SENTINEL, device="cuda")
        eps = torch.full((L, E, 40, H), SENTINEL, device="cuda")
        u = torch.full((L, E, 40), SENTINEL, dtype=torch.float64, device="cuda")
        if sized:
            _lib.check(lib.rs_pfgru_sized_draws(keys.data_ptr(), E, L, H, h0.data_ptr(), eps.data_ptr(), u.data_ptr(), _stream()),
                       "rs_pfgru_sized_draws")
        else:
            _lib.check(lib.rs_pfgru_draws(keys.data_ptr(), E, L, h0.data_ptr(), eps.data_ptr(), u.data_ptr(), _stream()), "rs_pfgru_draws")
        out.append((h0, eps, u))
    for a, b in zip(*out):
        assert torch.equal(a, b)
        assert not bool((a == SENTINEL).any())                     # every element was drawn


def test_gru_h0_twins_are_bit_identical_and_masked():
    N, A = 5, 2
    lib = _lib.load()
    base, begun = _keys(A, N, seed=5), _keys(N, seed=6) % 1000
    mask = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8, device="cuda")
    scale = 1.0 / H ** 0.5
    out = []
    for sized in (False, True):
        h = torch.full((A, N, H), SENTINEL, device="cuda")
        if sized:
            _lib.check(lib.rs_gru_h0_reset_sized(h.data_ptr(), base.data_ptr(), begun.data_ptr(), mask.data_ptr(), scale, H, N, A, _stream()),
                       "rs_gru_h0_reset_sized")
        else:
            _lib.check(lib.rs_gru_h0_reset(h.data_ptr(), base.data_ptr(), begun.data_ptr(), mask.data_ptr(), scale, N, A, _stream()),
                       "rs_gru_h0_reset")
        out.append(h)
    assert torch.equal(out[0], out[1])
    m = mask.bool()
    assert bool((out[0][:, ~m] == SENTINEL).all()) and bool((out[0][:, m].abs() <= scale).all())
