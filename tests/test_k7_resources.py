"""K7's register budget, read from the built code object like tests/test_kernel_resources.py (tests/_kernel_meta.py's reader): both
instantiations of rs_ppo_grad2_kernel run two waves per SIMD (<= 256 VGPRs), without scratch or spills, and their workgroup
fits the CU's 160 KB of LDS (the dynamic part by a static_assert next to the launch)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402


@pytest.mark.parametrize("nout", [8, 1])
def test_k7_two_waves_per_simd_without_scratch(nout):
    k = M.one(M.library_kernels(), f"rs_ppo_grad2_kernelILi{nout}E")
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["vgpr"] <= 256, k


@pytest.mark.parametrize("nout", [8, 1])
def test_k7_no_static_lds(nout):
    """all of K7's LDS is dynamic: its size, rs_grad2_lds_floats(nout) floats, is held to the CU's 160 KB by a static_assert"""
    assert M.one(M.library_kernels(), f"rs_ppo_grad2_kernelILi{nout}E")["lds"] == 0
