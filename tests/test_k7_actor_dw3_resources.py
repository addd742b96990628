"""The actor's dW3 / db3 / statistics phase on 4x4x1 MFMA chains and the packed tanh / tanh' pairs of both networks must not cost K7
its occupancy: rs_ppo_grad2_kernel<8>, <1> and the pair kernel (whose register count is the maximum of both bodies) stay without
scratch, without VGPR or SGPR spills and at or below 256 VGPRs, i.e. two waves per SIMD.  None has static LDS; the dynamic size,
rs_grad2_lds_floats(), did not change.  All numbers are read from the kernel metadata of the built code object
(tests/_kernel_meta.py's reader)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

MAX_VGPR = 256             # 512 registers per lane and SIMD / 2 waves


@pytest.mark.parametrize("name", ["rs_ppo_grad2_kernelILi8E", "rs_ppo_grad2_kernelILi1E", "rs_ppo_grad2_pair_kernel"])
def test_k7_actor_dw3_keeps_the_budget(name):
    k = M.one(M.library_kernels(), name)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["vgpr"] + k["agpr"] <= MAX_VGPR and M.waves_by_vgpr(k["vgpr"]) >= 2, k
    assert k["lds"] == 0, k
