"""The sized PFGRU kernels (rs_pfgru_sized.hip) from the code objects inside the built library, without a GPU: no scratch, no VGPR
spills, VGPRs and LDS within the occupancy DESIGN.md section 3 states for every width; the C ABI's argument checks, which return
before anything is launched; the packed-weight size against the packer."""
import os
import sys

import pytest

from radiation_ppo_amd import build

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

# waves per SIMD DESIGN.md section 3 states by width (one 256-thread workgroup = one wave per SIMD)
WAVES = {8: 4, 16: 4, 24: 3, 32: 3, 40: 2, 48: 2, 56: 2, 64: 1}


@pytest.mark.parametrize("rec", [0, 1])
@pytest.mark.parametrize("H", sorted(WAVES))
def test_sized_pfgru_kernels_fit_their_occupancy(H, rec):
    k = M.one(M.library_kernels(), f"rs_pfgru_sized_kernelILi{H}ELb{rec}E")
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert M.waves_by_vgpr(k["vgpr"]) >= WAVES[H], k
    assert M.workgroups_by_lds(k["lds"]) >= WAVES[H], k                  # LDS does not cut the occupancy below the stated one


def test_sized_pfgru_reset_has_no_scratch():
    k = M.one(M.library_kernels(), "rs_pfgru_reset_kernelILi0E")
    assert k["scratch"] == 0, k


def test_sized_pfgru_entry_points_check_their_arguments():
    from radiation_ppo_amd import _lib
    from radiation_ppo_amd.pfgru import PFGRUCell, SIZED_WIDTHS, pack_sized_weights
    build.build(verbose=False)
    lib = _lib.load()
    for H in SIZED_WIDTHS:
        assert lib.rs_pfgru_sized_weight_floats(H) == pack_sized_weights([PFGRUCell(hidden_size=H)]).shape[1]
    w = 4096                                                   # non-NULL stand-ins: nothing is touched before the checks fail
    alive = (C_INT * 3)(4, 4, 2)
    for H in (0, 4, 12, 20, 65, 72, -8):
        assert lib.rs_pfgru_sized_weight_floats(H) == 0
        assert lib.rs_pfgru_sized_step(w, w, w, w, w, w, w, None, 1, 0.7, w, 16, 1, H, None) == 4
        assert lib.rs_pfgru_sized_step_recorded(w, w, w, w, w, w, None, 1, 0.7, w, 16, 1, H, None) == 4
        assert lib.rs_pfgru_sized_reset(w, w, w, w, w, None, 16, 1, H, None) == 4
        assert lib.rs_pfgru_sized_pass(w, w, w, w, w, w, w, 0.7, w, alive, 3, 4, H, None) == 4
    assert lib.rs_pfgru_sized_step(None, w, w, w, w, w, w, None, 1, 0.7, w, 16, 1, 64, None) == 1
    assert lib.rs_pfgru_sized_step(w, w, w, w, w, w, w, None, 1, 0.7, w, 0, 1, 64, None) == 1         # no envs
    assert lib.rs_pfgru_sized_step(w, w, w, w, w, w, w, None, 1, 0.7, w, 16, 9, 64, None) == 1        # more than 8 owners
    assert lib.rs_pfgru_sized_step(w, w, w, w, w, w, w, None, 1, 0.7, w, 16, 0, 64, None) == 1
    assert lib.rs_pfgru_sized_step_recorded(w, w, w, w, None, w, None, 1, 0.7, w, 16, 1, 16, None) == 1
    assert lib.rs_pfgru_sized_reset(w, w, None, w, w, None, 16, 1, 32, None) == 1
    assert lib.rs_pfgru_sized_reset(w, w, w, w, w, None, 16, 9, 32, None) == 1
    assert lib.rs_pfgru_sized_pass(w, w, w, w, w, w, w, 0.7, w, alive, 0, 4, 64, None) == 1           # no steps
    assert lib.rs_pfgru_sized_pass(w, w, w, w, w, w, w, 0.7, w, None, 3, 4, 64, None) == 1
    rising = (C_INT * 3)(2, 4, 4)
    assert lib.rs_pfgru_sized_pass(w, w, w, w, w, w, w, 0.7, w, rising, 3, 4, 64, None) == 1         # alive[] not descending


C_INT = __import__("ctypes").c_int32
