"""K6 (rs_rollout16_kernel, the fused rollout) draws an env's measurement with rs_poisson_group (csrc/rs_device.hpp): candidates
0..2 of the PTRS rejection loop evaluated side by side in three lanes of the env, the serial loop only from candidate 3 on, and one
Philox call per lock-step that also yields the action uniform.  The draw is a pure function of (candidate, t, episode, stream, key,
rate), so nothing a launch leaves behind may change.

Probe (rs_poisson_probe): 2^18 draws over rates on both sides of every branch (0, the multiplication method below 10, PTRS from
10 on up to 1e7) with varied t, episode and env id: the grouped sampler at 3 and at 4 candidates per trip returns the serial
sampler's integer for every draw, and by the probe's own count of the serial loop's candidates enough draws went past the third
and the fourth candidate to exercise the fallback (a condition on the inputs, not a tolerance: about 400 and 50 are expected).

Rollout: tests/golden/k6_poisson_bits.npz was recorded from the library with the serial draw by
tests/golden/make_k6_poisson_bits.py, which also builds the cases (64 envs, 60 steps per epoch, 20 per episode, with and without
obstacles, weights at two scales; 16 envs with falloff="inverse_square" and DEBUG=True, whose rates fall below 10), checks on the
CPU that draws of the 64-env cases need more than 3 candidates, and documents the fixture's layout.  Two collect() calls per case;
act, rew and obs[..., 0] are compared element by element, every field by its SHA-256 digest."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu
MP = K.maker("make_k6_poisson_bits")
RATES = (0.0, 3.5, 9.999, 10.0, 10.0001, 15.0, 60.0, 400.0, 1500.0, 5000.0, 1e5, 1e7)
DRAWS = 1 << 18
SEED = 20250


@pytest.fixture(scope="module")
def probe():
    """(rate, serial, group3, group4, candidates) of DRAWS draws, numpy arrays"""
    import torch
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(7)
    lam = np.tile(np.array(RATES), DRAWS // len(RATES) + 1)[:DRAWS].copy()
    t = rng.integers(0, 500, DRAWS).astype(np.uint32)
    ep = rng.integers(0, 1 << 20, DRAWS).astype(np.uint32)
    ep[::97] = 0xFFFFFFFF - rng.integers(0, 4, ep[::97].size).astype(np.uint32)       # counter words near the top as well
    env = rng.integers(0, 1 << 16, DRAWS).astype(np.uint32)
    dev = [torch.from_numpy(lam).cuda()] + [torch.from_numpy(a.view(np.int32)).cuda() for a in (t, ep, env)]
    out = [torch.full((DRAWS,), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
    cand = torch.full((DRAWS,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.rs_poisson_probe(*(d.data_ptr() for d in dev), DRAWS, SEED, *(o.data_ptr() for o in out), cand.data_ptr(), None),
               "rs_poisson_probe")
    torch.cuda.synchronize()
    return (lam,) + tuple(o.cpu().numpy() for o in out) + (cand.cpu().numpy(),)


def test_probe_grouped_draw_is_the_serial_draw(probe):
    lam, serial, g3, g4, cand = probe
    for r in RATES:
        m = lam == r
        print("rate", r, "draws", int(m.sum()), "mean", float(serial[m].mean()), "candidates max", int(cand[m].max()),
              "differ at 3 / 4 lanes:", int((g3[m] != serial[m]).sum()), int((g4[m] != serial[m]).sum()))
    assert (serial >= 0).all() and (serial[lam == 0.0] == 0).all()
    for r in RATES[1:]:                                                # the draws are Poisson at all: mean within 6 sigma
        m = lam == r
        assert abs(serial[m].mean() - r) < 6.0 * np.sqrt(r / m.sum()), r
    K.same_bits(g3, serial, "3 candidates per trip")
    K.same_bits(g4, serial, "4 candidates per trip")


def test_probe_inputs_reach_the_serial_fallback(probe):
    lam, _, _, _, cand = probe
    ptrs = lam >= 10.0
    assert (cand[~ptrs] == 0).all() and (cand[ptrs] >= 1).all()
    over3, over4 = int((cand[ptrs] > 3).sum()), int((cand[ptrs] > 4).sum())
    print("draws with rate >= 10:", int(ptrs.sum()), "needed > 1 / > 3 / > 4 candidates:", int((cand[ptrs] > 1).sum()), over3, over4)
    assert over3 >= 100 and over4 >= 10, (over3, over4)


@pytest.fixture(scope="module")
def golden():
    return K.golden("k6_poisson_bits.npz")


def test_golden_holds_every_case(golden):
    want = [f"{c[0]}/dig" for c in MP.CASES] + [f"{c[0]}/{launch}_{k}" for c in MP.CASES for launch in range(2) for k in MP.RAW]
    assert sorted(golden.files) == sorted(want)
    assert {(c[1], c[2]) for c in MP.CASES} == {(64, 0), (64, -1), (16, 0)} and {c[6] for c in MP.CASES} == {1.0, 4.0}
    assert [c[3:5] for c in MP.CASES if c[1] == 16] == [("inverse_square", True)]


def _words(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name,N,obst,falloff,debug,seed,scale", MP.CASES, ids=[c[0] for c in MP.CASES])
def test_k6_rollout_bitwise(golden, name, N, obst, falloff, debug, seed, scale):
    got = MP.run(N, obst, falloff, debug, seed, scale)
    for launch in range(2):                                            # element by element first: a failure names the draw
        for k in MP.RAW:
            K.same_bits(_words(MP.raw(got, launch, k)), _words(golden[f"{name}/{launch}_{k}"]), (name, launch, k))
    dig = MP.digests(got)
    want = golden[f"{name}/dig"]
    assert dig.shape == want.shape and dig.dtype == want.dtype
    bad = [MP.MK.FIELDS[i] for i in np.flatnonzero((dig != want).any(axis=1))]
    print(name, "fields", len(got), "cuts", int(got["0_buf_cut"].sum()), "err", int(got["1_err"][0]))
    assert not bad, bad
