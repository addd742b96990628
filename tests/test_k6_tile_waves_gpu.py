"""K6 (rs_rollout16_kernel, the fused rollout) computes the actor's two hidden layers on four waves, one 16-unit output tile each,
and exchanges the tiles through LDS between workgroup barriers (csrc/rs_rollout16.hpp, "Tile waves").  Every accumulator keeps
its order of sums, so nothing a launch leaves behind may change: tests/golden/k6_tile_waves_bits.npz was recorded from the library
in which wave 0 computed all four tiles, by tests/golden/make_k6_tile_waves_bits.py, which also builds the cases and documents the
fixture: 16 envs with T = 1 (the shortest launch: message -1 and one lock-step), T = 2 and 3 (both parities of the mailbox slot),
32 envs with T = 7 and L = 3 at weight scales 1 and 4 (cuts inside the launch and on its last step), the same with staggered
episode clocks (cut and uncut envs in one wave: post-reset and pre-reset rows side by side), the obstacle template, and 4112 envs,
one workgroup more than there are CUs, where the library launches two-wave workgroups instead (rs_rollout16_wide_kernel).  Two
collect() calls per case.  act, rew and obs are compared element by element (up to 64 envs), then every field (the buffer: obs, act, logp, val, rew,
last_val, cut, source_tar, adv, ret; the collect statistics and the Welford carry; the env arrays; error_flags()) by its SHA-256
digest after each launch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu
MT = K.maker("make_k6_tile_waves_bits")


@pytest.fixture(scope="module")
def golden():
    return K.golden("k6_tile_waves_bits.npz")


def test_golden_holds_every_case(golden):
    want = [f"{c[0]}/dig" for c in MT.CASES] + [f"{c[0]}/{launch}_{k}" for c in MT.CASES if c[1] <= MT.RAW_MAX_N for launch in range(2)
                                                for k in MT.RAW]
    assert sorted(golden.files) == sorted(want)
    shapes = {c[1:5] for c in MT.CASES}                                # (N, T, L, obstruction_count)
    assert {(16, 1, 1, 0), (16, 2, 120, 0), (16, 3, 120, 0), (32, 7, 3, 0), (16, 7, 3, -1), (4112, 3, 2, 0)} == shapes
    assert {c[6] for c in MT.CASES if c[1:5] == (32, 7, 3, 0)} == {1.0, 4.0}
    assert [c[0] for c in MT.CASES if c[7]] == ["n32_t7_l3_stag"]
    for f in ("obs", "act", "logp", "val", "rew", "last_val", "cut", "source_tar"):
        assert f"0_buf_{f}" in MT.MK.FIELDS and f"1_buf_{f}" in MT.MK.FIELDS
    assert all(f"1_col_{f}" in MT.MK.FIELDS for f in ("w_count", "w_mean", "w_sq", "w_std", "ep_count", "ep_ret_sum"))


def _words(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name,N,T,L,obst,seed,scale,stagger", MT.CASES, ids=[c[0] for c in MT.CASES])
def test_k6_rollout_bitwise(golden, name, N, T, L, obst, seed, scale, stagger):
    got = MT.run(N, T, L, obst, seed, scale, stagger)
    for launch in range(2 if N <= MT.RAW_MAX_N else 0):                # element by element first: a failure names the sample
        for k in MT.RAW:
            K.same_bits(_words(MT.raw(got, launch, k)), _words(golden[f"{name}/{launch}_{k}"]), (name, launch, k))
    dig = MT.digests(got)
    want = golden[f"{name}/dig"]
    assert dig.shape == want.shape and dig.dtype == want.dtype
    bad = [MT.MK.FIELDS[i] for i in np.flatnonzero((dig != want).any(axis=1))]
    print(name, "fields", len(got), "cuts", int(got["0_buf_cut"].sum()), "err", int(got["1_err"][0]))
    assert not bad, bad
