"""The sized RAD-A2C kernels (rs_rnn_sized.hip) from the code objects inside the built library, without a GPU: no scratch, no VGPR
spills, VGPRs within the occupancy DESIGN.md states for every GRU tier; and the C ABI's argument checks, which return before anything is
launched."""
import os
import sys

import pytest

from radiation_ppo_amd import build

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

# waves per SIMD DESIGN.md section 3 states, by kernel and GRU tier (16, 32, 48, 64 units)
WAVES = {
    "rs_rnn_sized_step_kernel": (4, 3, 2, 1),
    "rs_gru_sized_fwd_kernel": (4, 3, 1, 1),
    "rs_gru_sized_bwd_kernel": (4, 3, 2, 2),
    "rs_a2c_sized_heads_kernel": (4, 2, 2, 1),
}


@pytest.mark.parametrize("kernel", sorted(WAVES))
def test_sized_rnn_kernels_fit_their_occupancy(kernel):
    for tier, waves in zip((16, 32, 48, 64), WAVES[kernel]):
        k = M.one(M.library_kernels(), kernel + f"ILi{tier}E")
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert M.waves_by_vgpr(k["vgpr"]) >= waves, (k, waves)


def test_sized_h0_kernel_has_no_scratch():
    k = M.one(M.library_kernels(), "rs_gru_h0_kernel")
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k


def test_sized_rnn_entry_points_check_their_arguments():
    from radiation_ppo_amd import _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.rs_rnn_sized_weight_floats(32, 64, 64) > 0 and lib.rs_rnn_sized_weight_floats(1, 2, 2) > 0
    for hid, pol, val in ((0, 32, 32), (65, 32, 32), (32, 1, 32), (32, 32, 1), (32, 65, 32), (32, 32, 65), (-1, -1, -1)):
        assert lib.rs_rnn_sized_weight_floats(hid, pol, val) == 0
    assert lib.rs_gru_sized_weight_floats(0) == 0 and lib.rs_gru_sized_weight_floats(65) == 0 and lib.rs_gru_sized_weight_floats(64) > 0
    assert lib.rs_gru_sized_gate_floats(13) == 64 and lib.rs_gru_sized_gate_floats(64) == 256 and lib.rs_gru_sized_gate_floats(65) == 0
    w = 4096                                                   # non-NULL stand-ins: nothing is touched before the checks fail
    for hid, pol, val in ((65, 32, 32), (0, 32, 32), (32, 1, 32), (32, 32, 65)):
        assert lib.rs_rnn_sized_step(w, hid, pol, val, w, 11, w, 2, w, w, 1, w, None, w, w, w, None, 1, None, 16, None) == 4
        assert lib.rs_a2c_sized_heads_loss(w, hid, pol, val, w, w, w, w, w, w, w, w, w, w, 64, 0.2, 0.01, None) == 4
    for hid in (0, 65):
        assert lib.rs_gru_sized_forward(w, w, w, w, w, hid, 4, 16, None) == 4
        assert lib.rs_gru_sized_backward(w, w, w, w, w, w, w, hid, 4, 16, None) == 4
        assert lib.rs_gru_h0_reset_sized(w, w, w, None, 0.2, hid, 16, 1, None) == 4
    assert lib.rs_rnn_sized_step(None, 32, 64, 64, w, 11, w, 2, w, w, 1, w, None, w, w, w, None, 1, None, 16, None) == 1
    assert lib.rs_rnn_sized_step(w, 32, 64, 64, w, 11, w, 2, w, None, 1, w, None, w, w, w, None, 1, None, 16, None) == 1    # act without u
    assert lib.rs_rnn_sized_step(w, 32, 64, 64, w, 10, w, 2, w, w, 1, w, None, w, w, w, None, 1, None, 16, None) == 1    # x stride < 11
    assert lib.rs_rnn_sized_step(w, 32, 64, 64, w, 11, w, 2, w, w, 1, w, None, w, w, w, None, 1, None, 0, None) == 1     # no envs
    assert lib.rs_gru_sized_forward(None, w, w, w, w, 32, 4, 16, None) == 1
    assert lib.rs_gru_sized_backward(w, w, w, w, w, w, w, 32, 0, 16, None) == 1
    assert lib.rs_a2c_sized_heads_loss(w, 32, 64, 64, None, w, w, w, w, w, w, w, w, w, 64, 0.2, 0.01, None) == 1
    assert lib.rs_a2c_sized_heads_loss(w, 32, 64, 64, w, w, w, w, w, w, w, w, w, w, 0, 0.2, 0.01, None) == 1
    assert lib.rs_gru_h0_reset_sized(None, w, w, None, 0.2, 32, 16, 1, None) == 1
    assert lib.rs_gru_h0_reset_sized(w, w, w, None, 0.2, 32, 0, 1, None) == 1
