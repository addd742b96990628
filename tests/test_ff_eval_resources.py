"""Resources of the two evaluation kernels (csrc/rs_eval.hip), read from the built code object (tests/_kernel_meta.py).  Conditions,
not measurements: rs_ff_eval_step_kernel's workgroup is ONE wave that first fills 21.8 KB of LDS with its agent's actor, so it needs
a neighbour on its SIMD to hide that fill -- two waves per SIMD by registers (VGPRs + AGPRs <= 256), as its sibling
rs_ff_team_step_kernel -- and neither kernel may keep anything in scratch or in static LDS."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

KERNELS = ["rs_ff_eval_step_kernel", "rs_eval_post_step_kernel"]
#          key            bound
EXACT = [("scratch",      0),
         ("vgpr_spill",   0),
         ("sgpr_spill",   0),
         ("lds",          0)]                  # static LDS: none, the actor's LDS is dynamic (rs_mlp_lds_floats(8), 21.8 KB)
MIN_WAVES_BY_VGPR = 2


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key,bound", EXACT, ids=[k for k, _ in EXACT])
def test_eval_kernels_exact(kernel, key, bound):
    k = M.one(M.library_kernels(), kernel)
    assert k[key] == bound, k


def test_eval_step_kernel_leaves_room_for_a_second_wave():
    k = M.one(M.library_kernels(), "rs_ff_eval_step_kernel")
    assert M.waves_by_vgpr(k["vgpr"] + k["agpr"]) >= MIN_WAVES_BY_VGPR, k
