"""Resources of the kernels behind the PPO update's pair launch and its preparation (rs_ppo_grad2_pair_kernel in rs_ppo.hip, the three
rs_ppo_prepare kernels in rs_env.hip), from the kernel metadata of the built library's code objects (no GPU needed): no scratch, no
spills, at most 256 VGPRs -- the pair kernel keeps K7's two waves per SIMD -- and the pair kernel's LDS is all dynamic, like K7's."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402


def _lean(k):
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["vgpr"] <= 256, k


def test_pair_kernel_keeps_two_waves_per_simd():
    k = M.one(M.library_kernels(), "rs_ppo_grad2_pair_kernel")
    _lean(k)
    assert k["lds"] == 0, k          # all dynamic, held to 160 KB by the static_assert next to the launch


@pytest.mark.parametrize("kernel", ["rs_ppo_prepare_cols_kernel", "rs_ppo_prepare_sq_kernel", "rs_ppo_prepare_norm_kernel"])
def test_prepare_kernels_are_lean(kernel):
    k = M.one(M.library_kernels(), kernel)
    _lean(k)
    assert k["lds"] <= 4096, k
