"""K7 (rs_ppo_grad) reproduces tests/golden/k7_bits.npz bit for bit: the gradient bucket (gradients + the statistics' (hi, lo)
tail) and the five float64 statistics, for ragged batch sizes, BASELINE config 2's batch and the stop-flag path (zeros).
Exact equality: any layout or instruction change of the kernels must leave every bit where it was."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maker():
    spec = importlib.util.spec_from_file_location("make_k7_bits", os.path.join(ROOT, "tests", "golden", "make_k7_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _maker()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "k7_bits.npz"))


@pytest.mark.parametrize("name,M,seed,stop", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_k7_bitwise(golden, name, M, seed, stop):
    g, s = MK.run(name, M, seed, stop)
    ge, se = golden["g_" + name], golden["s_" + name]
    assert g.dtype == ge.dtype and g.shape == ge.shape and s.shape == se.shape
    bad = np.flatnonzero(g.view(np.uint32) != ge.view(np.uint32))
    assert bad.size == 0, (name, bad.size, bad[:8].tolist(), g[bad[:4]].tolist(), ge[bad[:4]].tolist())
    assert np.array_equal(s.view(np.uint64), se.view(np.uint64)), (name, s.tolist(), se.tolist())
    if stop:
        assert not g.any() and not s.any()
