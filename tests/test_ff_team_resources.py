"""rs_ff_team_step_kernel's resources, read from the built code object (tests/_kernel_meta.py).  These are conditions, not
measurements: its workgroup is ONE wave that first fills 42.3 KB of LDS with its agent's weights, so it needs a neighbour on its SIMD
to hide that fill -- two waves per SIMD by registers (VGPRs + AGPRs <= 256) -- and nothing of the forward pass may live in scratch."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

KERNEL = "rs_ff_team_step_kernel"
#          key            bound
EXACT = [("scratch",      0),
         ("vgpr_spill",   0),
         ("sgpr_spill",   0),
         ("lds",          0)]                  # static LDS: none, the weights' LDS is dynamic (rs_mlp_lds_floats, 42.3 KB at most)
MIN_WAVES_BY_VGPR = 2


@pytest.mark.parametrize("key,bound", EXACT, ids=[k for k, _ in EXACT])
def test_ff_team_step_kernel_exact(key, bound):
    k = M.one(M.library_kernels(), KERNEL)
    assert k[key] == bound, k


def test_ff_team_step_kernel_leaves_room_for_a_second_wave():
    k = M.one(M.library_kernels(), KERNEL)
    assert M.waves_by_vgpr(k["vgpr"] + k["agpr"]) >= MIN_WAVES_BY_VGPR, k
