"""rs_bpf_a2c_eval_step on the GPU: the observation and the location it builds against the torch expressions bit for bit, the GRU
state and the action against rs_rnn_team_eval_step fed exactly those byte for byte, the predicted position against the controller's
table exactly, and finished lanes left alone.

Sizes: one lane, one short of a 64-lane group, one over, and two groups and a bit; teams of 1, 2 and 8.  The statistics are set by
hand: a third of the pairs still have the fresh std = 1 with the mean at the reading (the first step of a run: x[0] = 0), a few means
lie 20 and 30 counts off a reading with std = 1 so that the clip at +-8 bites on both sides, the rest have deviations up to 50.  alive
has holes, and from 65 lanes on one whole 64-lane group is dead (a wave that leaves at once, after parking its lanes on 8)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _bpf_a2c_ref as R2  # noqa: E402

pytestmark = pytest.mark.gpu

AREA_MAX = 2200.0
_agents = {}


def _team(A):
    from radiation_ppo_amd.rada2c import RNNAgentPPO
    for a in range(A):
        if a not in _agents:
            torch.manual_seed(900 + a)
            _agents[a] = RNNAgentPPO(id=a)
    wts = [_agents[a].policy_weights() for a in range(A)]
    return wts, (C.c_void_p * A)(*[w.data_ptr() for w in wts])


def _inputs(N, A, seed):
    from radiation_ppo_amd.envs import RadSearchVec
    vec = RadSearchVec(N, number_agents=A, obstruction_count=0, enforce_grid_boundaries=True, seed=seed)
    vec.reset()
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device="cuda")
    obs = vec.obs.clone()
    obs[..., 0] = torch.floor(r(N, A) * 3000.0)
    kind = torch.arange(N * A, device="cuda").view(N, A) % 6
    mean = obs[..., 0].double() - (r(N, A).double() - 0.5) * 200.0
    std = 1.0 + r(N, A).double() * 49.0
    fresh = kind < 2
    mean, std = torch.where(fresh, obs[..., 0].double(), mean), torch.where(fresh | (kind == 2) | (kind == 3), torch.ones_like(std), std)
    mean = torch.where(kind == 2, obs[..., 0].double() - 20.0, torch.where(kind == 3, obs[..., 0].double() + 30.0, mean))
    est = torch.stack([r(N, A).double() * 900.0 + 100.0, r(N, A).double() * 2900.0 - 200.0, r(N, A).double() * 2900.0 - 200.0], dim=-1).contiguous()
    hid = ((r(A, N, 24) * 2.0 - 1.0) * 0.2).contiguous()
    alive = torch.from_numpy((np.arange(N) % 5 != 3).astype(np.uint8)).cuda()
    if N >= 65:
        alive[(0 if N < 128 else 64):(64 if N < 128 else 128)] = 0
    return vec, obs, mean.contiguous(), std.contiguous(), est, hid, r(N, A).contiguous(), alive


@pytest.mark.parametrize("A", [1, 2, 8])
@pytest.mark.parametrize("N", [1, 63, 65, 130])
def test_policy_round(N, A):
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    wts, wp = _team(A)
    vec, obs, mean, std, est, hid, u, alive = _inputs(N, A, 1000 * N + A)
    p = lambda t: t.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h1 = hid.clone()
    a8 = torch.full((N, A), -7, dtype=torch.int8, device="cuda")
    sim = torch.full((N, A, 2), -1.5, dtype=torch.float64, device="cuda")
    x_out = torch.full((N, A, 11), -3.25, dtype=torch.float32, device="cuda")
    loc_out = torch.full((N, A, 2), -3.25, dtype=torch.float32, device="cuda")
    _lib.check(lib.rs_bpf_a2c_eval_step(vec._h, wp, A, p(obs), p(mean), p(std), p(est), AREA_MAX, p(h1), p(u), p(alive), p(a8), p(sim), p(x_out),
                                        p(loc_out), st), "rs_bpf_a2c_eval_step")
    # the torch expressions
    x = obs.clone()
    x[..., 0] = ((obs[..., 0].double() - mean) / std).float().clamp(-8.0, 8.0)
    loc = (est[..., 1:] / AREA_MAX).float().contiguous()
    live = alive.bool()
    clipped = (x[..., 0].abs() == 8.0) & live.view(N, 1)
    busy = int(live.sum()) * A >= 40                             # enough live pairs for every kind of statistics to occur
    if busy:
        assert bool((x[..., 0] == 8.0)[live].any()) and bool((x[..., 0] == -8.0)[live].any()) and bool(clipped.any())
        assert bool(((std == 1.0) & (x[..., 0] == 0.0))[live].any())
    lv3 = live.view(N, 1, 1)
    assert torch.equal(x_out.view(torch.int32), torch.where(lv3, x, torch.full_like(x, -3.25)).view(torch.int32))
    assert torch.equal(loc_out.view(torch.int32), torch.where(lv3, loc, torch.full_like(loc, -3.25)).view(torch.int32))
    # rs_rnn_team_eval_step fed those
    h2 = hid.clone()
    b8 = torch.full((N, A), 8, dtype=torch.int8, device="cuda")
    _lib.check(lib.rs_rnn_team_eval_step(wp, A, p(x), p(loc), p(h2), p(u), p(alive), p(b8), N, st), "rs_rnn_team_eval_step")
    torch.cuda.synchronize()
    assert torch.equal(h1.view(torch.int32), h2.view(torch.int32))
    assert torch.equal(h1[:, ~live], hid[:, ~live]) and (not bool(live.any()) or not torch.equal(h1[:, live], hid[:, live]))
    assert torch.equal(a8, b8) and bool((a8[~live] == 8).all()) and bool((a8[live] < 8).all())
    pos = torch.stack([vec.state("x").t(), vec.state("y").t()], dim=-1).double()
    table = torch.from_numpy(R2.ACTION).cuda()
    want = torch.where(lv3, pos + table[a8.long().clamp(0, 7)], torch.full_like(sim, -1.5))
    assert torch.equal(sim, want)
    if busy:
        assert len(set(a8[live].view(-1).tolist())) >= 4               # the draws spread over the moves


def test_the_optional_outputs_may_be_null():
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    N, A = 70, 2
    wts, wp = _team(A)
    vec, obs, mean, std, est, hid, u, alive = _inputs(N, A, 5)
    p = lambda t: t.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for with_outs in (True, False):
        h1, a8 = hid.clone(), torch.full((N, A), -7, dtype=torch.int8, device="cuda")
        sim = torch.zeros(N, A, 2, dtype=torch.float64, device="cuda")
        xo, lo = torch.zeros(N, A, 11, device="cuda"), torch.zeros(N, A, 2, device="cuda")
        _lib.check(lib.rs_bpf_a2c_eval_step(vec._h, wp, A, p(obs), p(mean), p(std), p(est), AREA_MAX, p(h1), p(u), p(alive), p(a8), p(sim),
                                            p(xo) if with_outs else None, p(lo) if with_outs else None, st), "rs_bpf_a2c_eval_step")
        torch.cuda.synchronize()
        outs.append((h1, a8, sim))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_refusals_with_a_handle():
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.envs import RadSearchVec
    lib = _lib.load()
    vec = RadSearchVec(2, number_agents=2, seed=1)
    w, bad = 4096, _lib.RS_ERR_INVALID_ARG                          # non-NULL stand-ins: every refusal comes before anything is touched
    wts = (C.c_void_p * 8)(*([w] * 8))
    hole = (C.c_void_p * 8)(w, None, w, w, w, w, w, w)
    step = lambda ws, A, *rest: lib.rs_bpf_a2c_eval_step(vec._h, ws, A, *rest, None, None, None)
    args = [w, w, w, w, AREA_MAX, w, w, w, w, w]
    assert step(None, 2, *args) == bad and step(hole, 2, *args) == bad
    for A in (0, 1, 3, 9):                                          # outside 1..8, or not the handle's
        assert step(wts, A, *args) == bad, A
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9):                           # every required pointer
        a = list(args)
        a[k] = None
        assert step(wts, 2, *a) == bad, k
