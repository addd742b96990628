"""K6's template without obstacles (rs_rollout16_kernel<false>) runs a workgroup of four waves, one per SIMD, each with one output
tile of the actor's hidden layers (csrc/rs_rollout16.hpp, "Tile waves").  All four waves get the kernel's register allocation, so it
must still fit a SIMD's file alone, without spills and without more stack than the 64 bytes the kernel had with two waves; and the
two exchange arrays must leave the workgroup's dynamic LDS within the 160 KiB of a CU, which is what one workgroup may have.
Registers from the kernel metadata of the built code object (tests/_kernel_meta.py's reader), the LDS bytes from the library's own
rs_rollout_lds_bytes(), which is what rs_rollout passes to the launch."""
import os
import sys

sys.path.insert(0, os.path.dirname(__file__))
import _kernel_meta as M  # noqa: E402

PARENT_SCRATCH = 64                       # rs_rollout16_kernel<false> with two waves
LDS_LIMIT = 160 * 1024                    # a CU's LDS: the most one workgroup can be given
EXCHANGE = 2 * 4 * 64 * 16                # two arrays of [4 tiles][64 lanes] float4


def test_k6_plain_template_fits_one_wave_per_simd():
    k = M.one(M.library_kernels(), "rs_rollout16_kernelILb0E")
    assert k["vgpr_spill"] == 0, k
    assert k["scratch"] <= PARENT_SCRATCH, k
    assert k["vgpr"] <= 512 and k["agpr"] <= k["vgpr"], k             # vgpr_count is the total of the unified file: VGPRs + AGPRs
    assert M.waves_by_vgpr(k["vgpr"]) == 1, k                          # four waves of a workgroup are then four SIMDs: one CU
    assert k["lds"] == 0, k                                            # all of its LDS is the launch's dynamic segment


def test_k6_dynamic_lds_within_a_launch():
    M.build.build(verbose=False)
    from radiation_ppo_amd import _lib
    lib = _lib.load()
    plain, obs = lib.rs_rollout_lds_bytes(0), lib.rs_rollout_lds_bytes(1)
    print("dynamic LDS bytes: no obstacles", plain, "obstacles", obs)
    assert EXCHANGE < plain <= LDS_LIMIT, plain
    assert 0 < obs <= LDS_LIMIT, obs
