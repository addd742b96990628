"""The look-ahead kernels (rs_lookahead.hip: rs_peek_kernel, rs_gs_eval_step_kernel) from the code objects inside the built library,
without a GPU: the obstacle-free instantiations use no scratch, the obstacle instantiations no more than rs_step's obstacle kernel
of the same build (rs_step4_kernel, the kernel that runs the same shortest-path and intersection code)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402


@pytest.mark.parametrize("kernel", ["rs_peek_kernel", "rs_gs_eval_step_kernel"])
def test_lookahead_kernels_stay_within_the_env_step_s_scratch(kernel):
    kernels = M.library_kernels()
    free, obst, yard = M.one(kernels, kernel + "ILb0E"), M.one(kernels, kernel + "ILb1E"), M.one(kernels, "rs_step4_kernel")
    print(kernel, {k: (free[k], obst[k]) for k in ("vgpr", "scratch", "lds")}, "rs_step4_kernel", {k: yard[k] for k in ("vgpr", "scratch", "lds")})
    assert free["scratch"] == 0 and free["vgpr_spill"] == 0, free
    assert obst["scratch"] <= yard["scratch"], (obst, yard)
