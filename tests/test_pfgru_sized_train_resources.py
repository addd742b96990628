"""The training-pass kernels of the sized PFGRU (rs_pfgru_sized_train.hip) from the code objects inside the built library, without a
GPU: per instantiation the VGPR count and the LDS bytes within what the file header states, no scratch and no VGPR spill (the header
claims 0 at every width; DESIGN.md section 3 records it)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

WIDTHS = (8, 16, 24, 32, 40, 48, 56, 64)
# csrc/rs_pfgru_sized_train.hip, "Resources per width": (VGPR bound, LDS KB bound, waves per SIMD = workgroups per CU) per walk
FWD = {8: (128, 9.3, 4), 16: (128, 16.8, 4), 24: (128, 24.3, 4), 32: (128, 31.8, 4), 40: (128, 39.3, 4), 48: (128, 46.8, 3),
       56: (128, 54.3, 2), 64: (128, 61.8, 2)}
BWD = {8: (128, 21.4, 4), 16: (128, 31.5, 4), 24: (128, 39.0, 4), 32: (168, 49.1, 3), 40: (168, 56.6, 2), 48: (256, 66.6, 2),
       56: (256, 74.1, 2), 64: (256, 84.2, 1)}


@pytest.mark.parametrize("walk", ["fwd", "bwd"])
@pytest.mark.parametrize("H", WIDTHS)
def test_sized_train_kernels_fit_their_stated_resources(H, walk):
    k = M.one(M.library_kernels(), f"rs_pfgru_sized_train_{walk}_kernelILi{H}E")
    vgpr, lds_kb, waves = (FWD if walk == "fwd" else BWD)[H]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["vgpr"] <= vgpr and k["agpr"] == 0, k
    assert k["lds"] <= lds_kb * 1024, k
    assert min(M.workgroups_by_lds(k["lds"]), M.waves_by_vgpr(k["vgpr"])) >= waves, k      # the stated occupancy is reachable


def test_sized_draws_kernel_has_no_scratch():
    k = M.one(M.library_kernels(), "rs_pfgru_draws_kernelILi0E")
    assert k["scratch"] == 0 and k["lds"] == 0, k
