"""The critic's own sample-group loop (rs_ppo_grad2_body<1>) must not cost K7 its occupancy: the critic kernel and the pair kernel
(whose register count is the maximum of both bodies) stay without scratch or spills and at or below the 256 VGPRs both had when the
critic still ran the actor's body, i.e. two waves per SIMD.  Neither kernel has static LDS; the dynamic size, rs_grad2_lds_floats(),
did not change and is held to the CU's 160 KB by a static_assert next to the launch.  All numbers are read from the kernel metadata
of the built code object (tests/_kernel_meta.py's reader)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

PARENT_VGPR = 256          # rs_ppo_grad2_kernel<1> and rs_ppo_grad2_pair_kernel before the critic had a body of its own


@pytest.mark.parametrize("name", ["rs_ppo_grad2_kernelILi1E", "rs_ppo_grad2_pair_kernel"])
def test_k7_critic_body_keeps_the_budget(name):
    k = M.one(M.library_kernels(), name)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["vgpr"] <= PARENT_VGPR, k
    assert k["lds"] == 0, k
