"""The two kernels of the RAD-TEAM training round (rs_cnn_team_step_head_kernel in rs_cnn_eval.hip, rs_cnn_team_critic_fwd_kernel in
rs_cnn.hip) from the code objects inside the built library, without a GPU: registers (VGPRs and AGPRs, one file) within 256 for the
head -- two waves per SIMD -- and within K9's 128 for the trunk, no scratch, no spilled VGPRs, the head's LDS no more than the
evaluation head's.  The kernels they share code with keep their figures: the evaluation heads the 164 and 196 registers DESIGN.md
states, K9 (4 and 6 channels) and the team trunk 127 / 128 / 128 as before the two kernels were added, none with scratch."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

EVAL_HEAD_LDS = 4 * 64 * 36 * 4


def test_step_head_fits_two_waves_per_simd_without_scratch():
    kernels = M.library_kernels()
    k = M.one(kernels, "rs_cnn_team_step_head_kernel")
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["vgpr"] <= 256 and M.waves_by_vgpr(k["vgpr"]) >= 2, k                  # vgpr: the unified count, accumulators included
    assert k["lds"] <= M.one(kernels, "rs_cnn_team_eval_head_kernel")["lds"] == EVAL_HEAD_LDS, k
    assert M.workgroups_by_lds(k["lds"]) >= 2, k


def test_critic_team_trunk_keeps_k9s_four_waves_per_simd():
    kernels = M.library_kernels()
    k = M.one(kernels, "rs_cnn_team_critic_fwd_kernel")
    k9 = M.one(kernels, "rs_cnn_fwd_kernelILi4E")
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["vgpr"] <= 128 and M.waves_by_vgpr(k["vgpr"]) >= 4, k
    assert k["vgpr"] == k9["vgpr"] and k["lds"] == k9["lds"], (k, k9)               # the same body


@pytest.mark.parametrize("part,vgpr,lds", [
    ("rs_cnn_team_eval_head_kernel", 164, EVAL_HEAD_LDS),
    ("rs_cnn_sized_team_eval_head_kernel", 196, EVAL_HEAD_LDS),
    ("rs_cnn_fwd_kernelILi4E", 127, 0),
    ("rs_cnn_fwd_kernelILi6E", 128, 0),
    ("rs_cnn_team_fwd_kernel", 128, 0),
])
def test_the_kernels_next_to_them_keep_their_figures(part, vgpr, lds):
    k = M.one(M.library_kernels(), part)
    assert k["vgpr"] == vgpr and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == lds, k
