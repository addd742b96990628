"""The three kernels of the walls-off RAD-TEAM training round (sk_first_layer_kernel and sk_heads_kernel in rs_cnn_eval.hip: the
k-split first layer and the heads behind it; rs_sized_critics_fwd in rs_cnn_sized.hip: every critic's tiled trunk) from the code objects
inside the built library, without a GPU: no scratch, no spilled VGPRs; stage 1 at least two waves per SIMD by registers (VGPRs and
AGPRs are one file) and two workgroups per CU by LDS; the critic trunk the three waves per SIMD that rs_sized_team_fwd holds, with its
LDS."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402


@pytest.mark.parametrize("part,max_vgpr,min_waves,min_wg", [
    ("sk_first_layer_kernel", 256, 2, 2),
    ("sk_heads_kernel", 128, 4, 2),
    ("rs_sized_critics_fwd", 168, 3, 2),
])
def test_sized_team_step_kernels_fit_their_occupancy(part, max_vgpr, min_waves, min_wg):
    k = M.one(M.library_kernels(), part)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["vgpr"] <= max_vgpr and M.waves_by_vgpr(k["vgpr"]) >= min_waves, k      # vgpr: the unified count, accumulators included
    assert M.workgroups_by_lds(k["lds"]) >= min_wg, k


def test_stage_one_shares_the_evaluation_heads_lds_layout_and_the_critic_trunk_the_team_trunks():
    kernels = M.library_kernels()
    assert M.one(kernels, "sk_first_layer_kernel")["lds"] == M.one(kernels, "rs_cnn_team_eval_head_kernel")["lds"] == 4 * 64 * 36 * 4
    c, t = M.one(kernels, "rs_sized_critics_fwd"), M.one(kernels, "rs_sized_team_fwd")
    assert c["lds"] == t["lds"] and M.waves_by_vgpr(c["vgpr"]) >= M.waves_by_vgpr(t["vgpr"]) >= 3, (c, t)
