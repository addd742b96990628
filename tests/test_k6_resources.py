"""K6 (rs_rollout16_kernel) runs one workgroup of two waves per CU, one wave per SIMD, so each wave may use the whole 512-entry
register file.  The no-obstacle template holds the actor's MFMA operands and the env state in registers for the launch: that must
fit without spills and without more stack than the 64 bytes its out-of-line samplers had before.  The obstacle template was at the
limit already (18 spilled VGPRs, 80 bytes); what it took over from the other template must not add to either.  All numbers are
read from the kernel metadata of the built code object (tests/_kernel_meta.py's reader)."""
import os
import sys

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

PARENT_SCRATCH = 64                       # rs_rollout16_kernel<false> before
PARENT_OBS_SPILL, PARENT_OBS_SCRATCH = 18, 80          # rs_rollout16_kernel<true> before


def test_k6_plain_template_holds_its_operands_in_registers():
    k = M.one(M.library_kernels(), "rs_rollout16_kernelILb0E")
    assert k["vgpr_spill"] == 0, k
    assert k["vgpr"] <= 512 and k["agpr"] <= k["vgpr"], k          # vgpr_count is the total of the unified file: VGPRs + AGPRs
    assert k["scratch"] <= PARENT_SCRATCH, k


def test_k6_obstacle_template_is_no_worse():
    k = M.one(M.library_kernels(), "rs_rollout16_kernelILb1E")
    assert k["vgpr_spill"] <= PARENT_OBS_SPILL, k
    assert k["scratch"] <= PARENT_OBS_SCRATCH, k
    assert k["vgpr"] <= 512 and k["agpr"] <= k["vgpr"], k
