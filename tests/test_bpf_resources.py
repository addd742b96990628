"""The particle-filter kernels (rs_bpf.hip: rs_bpf_track_kernel, rs_ridfim_eval_step_kernel, rs_bpf_draws_kernel) from the code objects
inside the built library, without a GPU: no scratch memory, no spilled registers, and static LDS within a workgroup's 64 KiB -- the
kernels' LDS does not grow with the particle count (the resampler stages 512 chain steps at a time, the controller's tables are sized by
RS_BPF_MAX_WINDOW), so the figure holds at NP = 6000 as at any other."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

LDS_LIMIT = 64 * 1024


@pytest.mark.parametrize("parts", [("rs_bpf_track_kernel",), ("rs_ridfim_eval_step_kernel", "ILb0E"), ("rs_ridfim_eval_step_kernel", "ILb1E"),
                                   ("rs_bpf_draws_kernel",)])
def test_bpf_kernels_use_no_scratch_and_fit_lds(parts):
    k = M.one(M.library_kernels(), *parts)
    print(parts, {key: k[key] for key in ("vgpr", "agpr", "scratch", "lds")})
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["lds"] <= LDS_LIMIT, k
    assert M.waves_by_vgpr(k["vgpr"] + k["agpr"]) >= 2, k           # two 4-wave workgroups per CU at least
