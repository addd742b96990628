"""The two kernels BPF-A2C and the Fisher analysis add (rs_bpf.hip: rs_bpf_fim_kernel in its two forms; rs_rnn_policy.hip:
rs_bpf_a2c_step_kernel) from the code objects inside the built library, without a GPU: no scratch memory, no spilled registers
(vector or scalar), static LDS within a workgroup's 64 KiB -- rs_bpf_fim's is the reduction's four doubles at any particle count, the
policy round has none --, and registers for two waves per SIMD at least."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

LDS_LIMIT = 64 * 1024


@pytest.mark.parametrize("parts", [("rs_bpf_fim_kernel", "ILb0E"), ("rs_bpf_fim_kernel", "ILb1E"), ("rs_bpf_a2c_step_kernel",)])
def test_new_kernels_use_no_scratch_and_fit(parts):
    k = M.one(M.library_kernels(), *parts)
    print(parts, {key: k[key] for key in ("vgpr", "agpr", "scratch", "sgpr_spill", "lds")})
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["lds"] <= LDS_LIMIT, k
    assert M.waves_by_vgpr(k["vgpr"] + k["agpr"]) >= 2, k
