"""Register / scratch budgets of the hot kernels, read from the code objects inside the built library (no GPU, no recompilation):
DESIGN.md's occupancy statements (K11 three waves per SIMD without spills, K13's backward walk and K10 without scratch, ...) are
claims about exactly these numbers (tests/_kernel_meta.py reads them)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402


@pytest.mark.parametrize("parts,max_vgpr", [
    (("rs_pfgru_kernelILb0ELi1E",), 168),            # K11 collector step: three waves per SIMD (512 / 3, granule 8)
    (("rs_pfgru_kernelILb0ELi4E",), 168),            # K11 pass (four steps per launch)
    (("rs_pfgru_kernelILb1ELi1E",), 168),            # K11 with recorded draws
    (("rs_pfgru_train_fwd_kernelILb1E",), 256),      # K13 forward walk (draws hashed in the kernel): two waves per SIMD
    (("rs_pfgru_train_fwd_kernelILb0E",), 256),      # K13 forward walk (draws read)
    (("rs_pfgru_train_kernel",), 512),               # K13 backward walk: one wave per SIMD
    (("rs_cnn_fwd_kernelILi6E",), 128),              # K9: four waves per SIMD
    (("rs_cnn_fwd_kernelILi4E",), 128),
    (("rs_cnn_bwd_kernelILi6E",), 168),              # K10: three waves per SIMD
    (("rs_cnn_bwd_kernelILi4E",), 168),
    (("rs_gru_fwd_kernel",), 512),
    (("rs_gru_bwd_kernel",), 512),
    (("rs_a2c_heads_kernel",), 512),
])
def test_hot_kernels_fit_their_occupancy_without_scratch(parts, max_vgpr):
    k = M.one(M.library_kernels(), *parts)
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
    assert k["vgpr"] <= max_vgpr, k


def test_lds_budgets():
    """workgroups per CU by LDS (160 KB): K13's backward walk 4 (one wave per SIMD), K10 3, K9 2, K11 >= 3"""
    kernels = M.library_kernels()
    assert M.workgroups_by_lds(M.one(kernels, "rs_pfgru_train_kernel")["lds"]) == 4
    assert M.workgroups_by_lds(M.one(kernels, "rs_pfgru_kernelILb0ELi4E")["lds"]) >= 3
    assert M.workgroups_by_lds(M.one(kernels, "rs_pfgru_train_fwd_kernelILb1E")["lds"]) >= 2
