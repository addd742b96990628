"""K6 (rs_rollout16_kernel, the fused rollout) keeps the actor's MFMA operands and the env state in registers across its lock-steps
and computes the actor's output layer on 4x4x1 MFMA chains; everything a launch leaves behind must be, bit for bit, what the kernel
left when it read its weights from LDS, summed the output layer on the VALU and went through the env arrays in every lock-step.
tests/golden/k6_rollout_bits.npz was recorded from that earlier library by tests/golden/make_k6_rollout_bits.py, which also builds
the cases: 16 and 48 envs, walls on and off, obstruction_count 0 and -1 (both templates), two seeds with the weights at two scales,
23 steps per epoch with 5 per episode, and two collect() calls in a row so that the carried state crosses a launch.  Compared as
bytes after each launch: every rollout buffer field, cur_obs, the Welford and episode-statistic carries, the env state arrays and
error_flags()."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu
MK = K.maker("make_k6_rollout_bits")


@pytest.fixture(scope="module")
def golden():
    return K.golden("k6_rollout_bits.npz")


def test_golden_holds_every_case_and_field(golden):
    assert sorted(golden.files) == sorted(c[0] for c in MK.CASES)
    assert len(MK.FIELDS) == 2 * (len(MK.BUF) + len(MK.COL) + len(MK.ENV) + 1)
    assert {c[1] for c in MK.CASES} == {16, 48} and {c[2] for c in MK.CASES} == {True, False} and {c[3] for c in MK.CASES} == {0, -1}
    assert len({c[4] for c in MK.CASES}) == 2 and len({c[5] for c in MK.CASES}) == 2


@pytest.mark.parametrize("name,N,walls,obst,seed,scale", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_k6_rollout_bitwise(golden, name, N, walls, obst, seed, scale):
    got = MK.run(N, walls, obst, seed, scale)
    want_all = golden[name]
    assert want_all.dtype == np.uint8 and want_all.shape == MK.blob(got).shape, (name, want_all.shape)
    bad, at = [], 0
    for k in MK.FIELDS:                                               # field by field, so that a failure names what differs
        have = MK.pack(got[k])
        want = want_all[at:at + have.size].reshape(have.shape)
        at += have.size
        diff = np.flatnonzero((have != want).any(axis=0))             # elements with a differing byte
        if diff.size:
            bad.append((k, int(diff.size), "of", int(have.shape[1]), "first", diff[:4].tolist()))
    assert at == want_all.size
    print(name, "fields", len(got), "cuts", int(got["0_buf_cut"].sum()), "err", int(got["1_err"][0]))
    assert not bad, bad
