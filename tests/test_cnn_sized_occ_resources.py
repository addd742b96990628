"""The occupancy-aware tiled trunk kernels (rs_cnn_sized.hip: rs_sized_trunk_fwd_occ, rs_sized_trunk_bwd_occ, rs_sized_occupancy)
from the code objects inside the built library, without a GPU: no scratch, no VGPR spills, registers within the dense kernels'
occupancy (forward three workgroups of four waves per CU = three waves per SIMD, backward two) and LDS no larger than the dense
kernels'; and the new entries' argument checks, which return before anything is launched."""
import os
import sys

import pytest

from radiation_ppo_amd import build

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402


@pytest.mark.parametrize("part,dense,variants,min_wg", [
    ("rs_sized_trunk_fwd_occ", "rs_sized_trunk_fwd", (("ILi6E", "ILi6ELb1E"), ("ILi4E", "ILi4ELb1E")), 3),
    ("rs_sized_trunk_bwd_occ", "rs_sized_trunk_bwd", (("ILi6E", "ILi6E"), ("ILi4E", "ILi4E")), 2),
])
def test_occupancy_aware_kernels_fit_the_dense_kernels_occupancy(part, dense, variants, min_wg):
    kernels = M.library_kernels()
    for v, dv in variants:
        k, d = M.one(kernels, part + v), M.one(kernels, dense + dv)
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert M.waves_by_vgpr(k["vgpr"] + k["agpr"]) >= min_wg, k             # a 256-thread workgroup is one wave per SIMD
        assert M.workgroups_by_lds(k["lds"]) >= min_wg, k
        assert k["lds"] <= d["lds"], (k, d)


def test_occupancy_pass_is_light():
    k = M.one(M.library_kernels(), "rs_sized_occupancy")
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] <= 64 and k["lds"] <= 1024, k


def test_occupancy_entry_points_check_their_arguments():
    from radiation_ppo_amd import _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert [lib.rs_cnn_sized_tiles(m) for m in (8, 31, 32, 33, 34, 65, 66, 147, 148, 256)] == [1, 1, 1, 1, 4, 4, 9, 25, 25, 64]
    w = 4096                                           # non-NULL stand-ins: every refusal below comes before anything is touched
    for m in (7, 257, 0, -3):                          # outside [8, 256]
        assert lib.rs_cnn_sized_tiles(m) == 0
        assert lib.rs_cnn_sized_occupancy(w, 16, m, w, None) == 4
        assert lib.rs_cnn_sized_forward_occ(w, w, w, 2, 0, 16, m, w, w, w, w, w, w, w, w, w, None) == 4
        assert lib.rs_cnn_sized_backward_occ(w, w, w, 2, 1, 16, m, w, w, w, w, w, w, 1 << 20, w, None) == 4
    assert lib.rs_cnn_sized_occupancy(None, 16, 147, w, None) == 1 and lib.rs_cnn_sized_occupancy(w, 16, 147, None, None) == 1
    assert lib.rs_cnn_sized_forward_occ(w, w, w, 2, 0, 16, 147, w, w, w, w, w, w, w, w, None, None) == 1            # no flags
    assert lib.rs_cnn_sized_forward_occ(w, w, w, 2, 0, 16, 147, w, w, w, w, w, None, None, None, w, None) == 1      # a training pass: p1, amax, mask
    assert lib.rs_cnn_sized_forward_occ(w, w, w, 2, 2, 16, 147, w, w, w, w, w, w, w, w, w, None) == 1               # agent >= num_agents
    assert lib.rs_cnn_sized_backward_occ(w, w, w, 2, 0, 16, 147, w, w, w, w, w, w, 1 << 20, None, None) == 1        # no flags
    assert lib.rs_cnn_sized_backward_occ(w, w, w, 2, 0, 0, 147, w, w, w, w, w, w, 1 << 20, w, None) == 1            # no samples
