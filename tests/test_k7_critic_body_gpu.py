"""K7's critic pass has a sample-group loop of its own (rs_ppo_grad2_body<1>); it must reproduce, bit for bit, what the body it
shared with the actor computed.  tests/golden/k7_critic_bits.npz holds the critic's part of the gradient bucket (the sum of its
workgroup slabs) and the value-loss statistic as recorded from that earlier library (tests/golden/make_k7_critic_bits.py).

Cases, each as a pair launch and as one launch per network: M = 1 (one clamped group, every other wave runs a zero-weight trip),
M = 33 (a ragged second group), M = 32 * 2048 + 5 (some of the 2048 waves take a second trip, with a ragged tail), and one step with
the stop flag set (zeros are published, the filler in the bucket is overwritten)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maker():
    spec = importlib.util.spec_from_file_location("make_k7_critic_bits", os.path.join(ROOT, "tests", "golden", "make_k7_critic_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _maker()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "k7_critic_bits.npz"))


@pytest.mark.parametrize("form", MK.FORMS)
@pytest.mark.parametrize("name,M,seed,stop", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_k7_critic_bitwise(golden, name, M, seed, stop, form):
    g, s, bucket = MK.run(M, seed, stop, form)
    ge, se = golden["g_" + name], golden["s_" + name]
    assert g.dtype == ge.dtype and g.shape == ge.shape == (4993,) and se.shape == (1,)
    bad = np.flatnonzero(g.view(np.uint32) != ge.view(np.uint32))
    assert bad.size == 0, (name, form, bad.size, bad[:8].tolist(), g[bad[:4]].tolist(), ge[bad[:4]].tolist())
    v = s[MK.STAT_VALUE_LOSS:MK.STAT_VALUE_LOSS + 1]
    assert np.array_equal(v.view(np.uint64), se.view(np.uint64)), (name, form, v.tolist(), se.tolist())
    if stop:
        assert not bucket.any() and not s.any()
    else:
        assert g.any() and v[0] > 0.0
