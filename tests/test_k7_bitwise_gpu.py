"""K7 (rs_ppo_grad) reproduces tests/golden/k7_bits.npz bit for bit: the gradient bucket (gradients + the statistics' (hi, lo)
tail) and the five float64 statistics, for ragged batch sizes, BASELINE config 2's batch and the stop-flag path (zeros).
Exact equality: any layout or instruction change of the kernels must leave every bit where it was."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu
MK = K.maker("make_k7_bits")


@pytest.fixture(scope="module")
def golden():
    return K.golden("k7_bits.npz")


@pytest.mark.parametrize("name,M,seed,stop", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_k7_bitwise(golden, name, M, seed, stop):
    g, s = MK.run(name, M, seed, stop)
    ge, se = golden["g_" + name], golden["s_" + name]
    assert g.dtype == ge.dtype and g.shape == ge.shape and s.shape == se.shape
    K.same_bits(g.view(np.uint32), ge.view(np.uint32), (name, "gradient bucket"))
    K.same_bits(s.view(np.uint64), se.view(np.uint64), (name, "statistics", s.tolist(), se.tolist()))
    if stop:
        assert not g.any() and not s.any()
