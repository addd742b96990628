"""K7's actor pass computes its output layer as two chains of 32 v_mfma_f32_4x4x1_16b_f32 (rs_ppo_grad2_body<8>); it must reproduce,
bit for bit, what the VALU fmaf chains computed.  tests/golden/k7_actor_bits.npz holds the actor's gradients, the five statistics
and the parameters after one Adam step as recorded from that earlier library (tests/golden/make_k7_actor_bits.py, which also
builds the inputs and describes the cases): (a) M = 1, 31, 32, 33 and 65536 + 33, (b) a W3 with a magnitude of its own per
(output, unit), (c) a W3 of subnormal scale, inputs of about 1e-30, a NaN row and two infinite rows.  Every case runs through
rs_ppo_grad and through rs_ppo_update_step as a pair launch and as one launch per network.  Equality is on the raw bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu
MK = K.maker("make_k7_actor_bits")


@pytest.fixture(scope="module")
def golden():
    return K.golden("k7_actor_bits.npz")


def test_golden_inputs_are_the_generators(golden):
    """the stored inputs of the small cases are what inputs() builds today (the large case is rebuilt from its seed only)"""
    for name, M, seed, variant in MK.CASES:
        if M > MK.STORE_INPUTS_UP_TO:
            continue
        pv, bv = MK.inputs(M, seed, variant)
        for k, v in list(zip(K.PARAM_NAMES[:6], pv[:6])) + list(zip(K.BATCH_NAMES, bv)):
            want = golden[f"in_{name}_{k}"]
            assert v.dtype == want.dtype and v.tobytes() == want.tobytes(), (name, k)


@pytest.mark.parametrize("path", MK.PATHS)
@pytest.mark.parametrize("name,M,seed,variant", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_k7_actor_bitwise(golden, name, M, seed, variant, path):
    g, s, p = MK.run(M, seed, variant, path)
    want = K.expected(golden, name, path, MK.KINDS)
    ge, se, pe = want["g"], want["s"], want.get("p")
    print(name, path, "finite gradients", int(np.isfinite(g).sum()), "of", g.size, "statistics", s.tolist())
    assert ge.shape == (K.ACTOR_PARAMS,) and se.shape == (5,)
    K.same_bits(g.view(np.uint32), ge, (name, path, "actor gradients"))
    K.same_bits(s.view(np.uint64), se, (name, path, "statistics"))
    if path != "grad":
        assert pe.shape == (K.N_PARAMS,)
        K.same_bits(p.view(np.uint32), pe, (name, path, "parameters after Adam"))
    if variant in ("plain", "w3_distinct", "w3_denorm", "x_tiny"):
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(s))
