"""K7's critic pass has a sample-group loop of its own (rs_ppo_grad2_body<1>); it must reproduce, bit for bit, what the body it
shared with the actor computed.  tests/golden/k7_critic_bits.npz holds the critic's part of the gradient bucket (the sum of its
workgroup slabs) and the value-loss statistic as recorded from that earlier library (tests/golden/make_k7_critic_bits.py).

Cases, each as a pair launch and as one launch per network: M = 1 (one clamped group, every other wave runs a zero-weight trip),
M = 33 (a ragged second group), M = 32 * 2048 + 5 (some of the 2048 waves take a second trip, with a ragged tail), and one step with
the stop flag set (zeros are published, the filler in the bucket is overwritten)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu
MK = K.maker("make_k7_critic_bits")


@pytest.fixture(scope="module")
def golden():
    return K.golden("k7_critic_bits.npz")


@pytest.mark.parametrize("form", MK.FORMS)
@pytest.mark.parametrize("name,M,seed,stop", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_k7_critic_bitwise(golden, name, M, seed, stop, form):
    g, s, bucket = MK.run(M, seed, stop, form)
    ge, se = golden["g_" + name], golden["s_" + name]
    assert g.dtype == ge.dtype and g.shape == ge.shape == (4993,) and se.shape == (1,)
    K.same_bits(g.view(np.uint32), ge.view(np.uint32), (name, form, "critic gradients"))
    v = s[K.STAT_VALUE_LOSS:K.STAT_VALUE_LOSS + 1]
    K.same_bits(v.view(np.uint64), se.view(np.uint64), (name, form, "value loss", v.tolist(), se.tolist()))
    if stop:
        assert not bucket.any() and not s.any()
    else:
        assert g.any() and v[0] > 0.0
