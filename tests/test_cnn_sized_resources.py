"""The tiled CNN trunk kernels (rs_cnn_sized.hip) from the code objects inside the built library, without a GPU: no scratch, no VGPR
spills, VGPRs within the occupancy DESIGN.md states (forward three waves per SIMD, backward two) and LDS for at least two workgroups per
CU; and the C ABI's argument checks, which return before anything is launched."""
import os
import sys

import pytest

from radiation_ppo_amd import build

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402


@pytest.mark.parametrize("part,variants,max_vgpr,min_wg", [
    ("rs_sized_trunk_fwd", ("ILi6ELb1E", "ILi6ELb0E", "ILi4ELb1E", "ILi4ELb0E"), 168, 3),    # three waves per SIMD
    ("rs_sized_trunk_bwd", ("ILi6E", "ILi4E"), 256, 2),                                      # two waves per SIMD
])
def test_sized_trunk_kernels_fit_their_occupancy(part, variants, max_vgpr, min_wg):
    for v in variants:
        k = M.one(M.library_kernels(), part + v)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgpr"] <= max_vgpr, k
        assert M.workgroups_by_lds(k["lds"]) >= min_wg, k


def test_sized_entry_points_check_their_arguments():
    from radiation_ppo_amd import _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.rs_cnn_sized_slab_row(6) == lib.rs_cnn_trunk_slab_row(6) and lib.rs_cnn_sized_slab_row(4) == lib.rs_cnn_trunk_slab_row(4)
    assert lib.rs_cnn_sized_slab_row(5) == 0
    for M in (7, 257, 0, -3):                          # outside [8, 256]: no slab, RS_ERR_UNSUPPORTED
        assert lib.rs_cnn_sized_slab_rows(16, M, 6) == 0
        w = 4096                                       # non-NULL stand-ins: the side is refused before anything is touched
        assert lib.rs_cnn_sized_forward(w, w, w, 2, 0, 16, M, w, w, w, w, w, None, None, None, None) == 4
        assert lib.rs_cnn_sized_infer(w, None, None, 0, -1, 16, M, w, w, w, w, w, None) == 4
        assert lib.rs_cnn_sized_backward(w, w, w, 2, 1, 16, M, w, w, w, w, w, w, 1 << 20, None) == 4
    assert lib.rs_cnn_sized_forward(None, None, None, 0, -1, 16, 147, None, None, None, None, None, None, None, None, None) == 1
    w = 4096
    assert lib.rs_cnn_sized_forward(w, w, w, 2, 2, 16, 147, w, w, w, w, w, None, None, None, None) == 1     # agent >= num_agents
    assert lib.rs_cnn_sized_forward(w, None, None, 0, -1, 16, 147, w, w, w, w, w, w, None, w, None) == 1    # p1 / amax / mask: all or none
    assert lib.rs_cnn_sized_backward(w, w, w, 2, 0, 0, 147, w, w, w, w, w, w, 1 << 20, None) == 1           # no samples
