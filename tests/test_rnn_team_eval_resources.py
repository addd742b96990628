"""Resources of the three kernels of the recurrent team's evaluation lock-step (csrc/rs_rnn_policy.hip: the team's policy round;
csrc/rs_eval.hip: the two bookkeeping kernels), read from the built code object (tests/_kernel_meta.py).  Conditions, not
measurements: the lock-step is launch-bound, so none of the three may keep anything in scratch, spill a register or hold static LDS,
and the policy round -- K14's arithmetic for every agent of the team -- may not fit fewer waves on a SIMD than K14 itself."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

KERNELS = ["rs_rnn_team_step_kernel", "rs_rnn_team_post_step_kernel", "rs_rnn_team_post_refresh_kernel"]
#          key            bound
EXACT = [("scratch",      0),
         ("vgpr_spill",   0),
         ("sgpr_spill",   0),
         ("lds",          0)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key,bound", EXACT, ids=[k for k, _ in EXACT])
def test_rnn_team_eval_kernels_exact(kernel, key, bound):
    k = M.one(M.library_kernels(), kernel)
    assert k[key] == bound, k


def test_the_team_step_fits_as_many_waves_as_k14():
    kernels = M.library_kernels()
    team, k14 = M.one(kernels, "rs_rnn_team_step_kernel"), M.one(kernels, "rs_rnn_policy_kernel")
    assert M.waves_by_vgpr(team["vgpr"] + team["agpr"]) >= M.waves_by_vgpr(k14["vgpr"] + k14["agpr"]), (team, k14)
