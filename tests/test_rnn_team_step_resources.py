"""Resources of the two kernels behind rs_rnn_team_step / rs_rnn_sized_team_step (csrc/rs_rnn_policy.hip: rs_rnn_team_collect_kernel;
csrc/rs_rnn_sized.hip: rs_rnn_sized_team_kernel, one instantiation per GRU tier), read from the built code object
(tests/_kernel_meta.py).  Conditions, not measurements: a team's policy round is one serial chain per lane, so neither kernel may keep
anything in scratch, spill a vector register or hold static LDS, and neither may fit fewer waves on a SIMD than the per-agent kernel
whose arithmetic it repeats -- K14 (rs_rnn_policy_kernel) and rs_rnn_sized_step_kernel of the same tier, whose numbers are read from
the same library at test time."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

TIERS = (16, 32, 48, 64)
NEW = ["rs_rnn_team_collect_kernel"] + [f"rs_rnn_sized_team_kernelILi{t}E" for t in TIERS]
#          key            bound
EXACT = [("scratch",      0),
         ("vgpr_spill",   0),
         ("lds",          0)]


def _waves(k):
    return M.waves_by_vgpr(k["vgpr"] + k["agpr"])


@pytest.mark.parametrize("kernel", NEW)
@pytest.mark.parametrize("key,bound", EXACT, ids=[k for k, _ in EXACT])
def test_rnn_team_step_kernels_exact(kernel, key, bound):
    k = M.one(M.library_kernels(), kernel)
    assert k[key] == bound, k


def test_the_default_kernel_fits_as_many_waves_as_k14_and_spills_no_more_sgprs():
    kernels = M.library_kernels()
    team, k14 = M.one(kernels, "rs_rnn_team_collect_kernel"), M.one(kernels, "rs_rnn_policy_kernel")
    assert _waves(team) >= _waves(k14), (team, k14)
    assert team["sgpr_spill"] <= k14["sgpr_spill"], (team, k14)


@pytest.mark.parametrize("tier", TIERS)
def test_each_sized_tier_fits_as_many_waves_as_the_per_agent_step(tier):
    kernels = M.library_kernels()
    team, step = M.one(kernels, f"rs_rnn_sized_team_kernelILi{tier}E"), M.one(kernels, f"rs_rnn_sized_step_kernelILi{tier}E")
    assert _waves(team) >= _waves(step), (team, step)
