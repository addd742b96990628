"""K7's actor pass sums dW3, db3 and the four statistics over a group's samples as chains of v_mfma_f32_4x4x1_16b_f32, and both networks
run their tanh / tanh' chains on packed pairs (rs_ppo_grad2_body); they must reproduce, bit for bit, what the 16x16x4 tiles and the
scalar chains computed.  tests/golden/k7_actor_dw3_bits.npz holds the actor's gradients, the five statistics and the parameters after
one Adam step as recorded from that earlier library (tests/golden/make_k7_actor_dw3_bits.py, which also builds the inputs and
describes the cases): M = 1, 3, 4, 5, 15, 16, 17, 31, 32, 33 and 65536 + 17; advantages over twelve decades; all eight actions in
every group; zero-weight and clipped rows; a NaN row, two infinite rows; a W3 of subnormal scale.  Every case runs through
rs_ppo_grad and through rs_ppo_update_step as a pair launch and as one launch per network.  Equality is on the raw bits (the
critic's parameters after Adam: on their SHA-256 digest)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _k7_bits as K  # noqa: E402

pytestmark = pytest.mark.gpu
MK = K.maker("make_k7_actor_dw3_bits")


@pytest.fixture(scope="module")
def golden():
    return K.golden("k7_actor_dw3_bits.npz")


def test_golden_inputs_are_the_generators(golden):
    """the stored parameters and the stored batches of the small cases are what inputs() builds today (the large case is rebuilt
    from its seed only)"""
    for name, M, seed, variant in MK.CASES:
        if M > MK.STORE_INPUTS_UP_TO:
            continue
        pv, bv = MK.inputs(M, seed, variant)
        for k, v in zip(K.PARAM_NAMES, pv):
            own = f"in_{name}_{k}"
            want = golden[own] if own in golden.files else golden[f"in_params_{k}"]
            assert v.dtype == want.dtype and v.tobytes() == want.tobytes(), (name, k)
        for k, v in zip(K.BATCH_NAMES, bv):
            want = golden[f"in_{name}_{k}"]
            assert v.dtype == want.dtype and v.tobytes() == want.tobytes(), (name, k)


def test_golden_sees_the_summation_order(golden):
    """as recorded: reversing the rows of every group changed dW3, db3 and statistics words in every finite case from M = 15 up"""
    for name, M, seed, variant in MK.CASES:
        if variant in MK.FINITE and M >= MK.REV_ASSERT_FROM:
            n = golden[f"rev_{name}"]
            assert n.shape == (3,) and np.all(n > 0), (name, n.tolist())


@pytest.mark.parametrize("path", MK.PATHS)
@pytest.mark.parametrize("name,M,seed,variant", MK.CASES, ids=[c[0] for c in MK.CASES])
def test_k7_actor_dw3_bitwise(golden, name, M, seed, variant, path):
    g, s, p = MK.run(M, seed, variant, path)
    got, want = MK.words(g, s, p), K.expected(golden, name, path, MK.KINDS)
    print(name, path, "finite gradients", int(np.isfinite(g).sum()), "of", g.size, "statistics", s.tolist())
    assert want["g"].shape == (K.ACTOR_PARAMS,) and want["s"].shape == (5,) and sorted(got) == sorted(want)
    K.same_bits(got["g"], want["g"], (name, path, "actor gradients"))
    K.same_bits(got["s"], want["s"], (name, path, "statistics"))
    if path != "grad":
        K.same_bits(got["p"], want["p"], (name, path, "actor parameters after Adam"))
        K.same_bits(got["c"], want["c"], (name, path, "digest of the critic's parameters after Adam"))
    if variant in MK.FINITE:
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(s))


def test_reversed_rows_still_differ(golden):
    """the library under test sees the order too: with the rows of every group reversed, m33 gives other dW3, db3 and statistics words
    than the golden's forward order"""
    name, M, seed, variant = next(c for c in MK.CASES if c[0] == "m33")
    g, s, _ = MK.run(M, seed, variant, "grad", reverse=True)
    fwd = MK.order_words(golden[f"g_{name}_grad"].view(np.float32), golden[f"s_{name}_grad"].view(np.float64))
    n = [int((a != b).sum()) for a, b in zip(MK.order_words(g, s), fwd)]
    print("m33 reversed: dW3 / db3 / statistics words that differ", n, "recorded", golden[f"rev_{name}"].tolist())
    assert all(v > 0 for v in n), n
    assert n == golden[f"rev_{name}"].tolist()
