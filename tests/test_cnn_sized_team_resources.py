"""The two kernels of the walls-off RAD-TEAM evaluation (rs_sized_team_fwd in rs_cnn_sized.hip, rs_cnn_sized_team_eval_head_kernel in
rs_cnn_eval.hip) from the code objects inside the built library, without a GPU: no scratch, no VGPR spills, VGPRs within the occupancy
their header comments state (the trunk three waves per SIMD as rs_sized_trunk_fwd, the head two) and LDS for at least two workgroups per
CU.  The kernels they share code with keep their figures: tests/test_cnn_sized_resources.py, tests/test_cnn_team_eval_cpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402


@pytest.mark.parametrize("part,max_vgpr,min_waves,min_wg", [
    ("rs_sized_team_fwd", 168, 3, 2),
    ("rs_cnn_sized_team_eval_head_kernel", 256, 2, 2),
])
def test_sized_team_kernels_fit_their_occupancy(part, max_vgpr, min_waves, min_wg):
    k = M.one(M.library_kernels(), part)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["vgpr"] <= max_vgpr and M.waves_by_vgpr(k["vgpr"]) >= min_waves, k      # vgpr: the unified count, accumulators included
    assert M.workgroups_by_lds(k["lds"]) >= min_wg, k


def test_sized_team_head_shares_the_2704_kernels_lds_layout():
    kernels = M.library_kernels()
    assert M.one(kernels, "rs_cnn_sized_team_eval_head_kernel")["lds"] == M.one(kernels, "rs_cnn_team_eval_head_kernel")["lds"] == 4 * 64 * 36 * 4
