"""Resources of the kernels behind the PPO update's pair launch and its preparation (rs_ppo_grad2_pair_kernel in rs_ppo.hip, the three
rs_ppo_prepare kernels in rs_env.hip), from the kernel metadata of a cross-compile to gfx950 assembly (no GPU needed): no scratch, no
spills, at most 256 VGPRs -- the pair kernel keeps K7's two waves per SIMD -- and the pair kernel's LDS is all dynamic, like K7's."""
import os
import re
import subprocess

import pytest

from radiation_ppo_amd import build as rs_build


def _metadata(tmp_path_factory, source):
    try:
        cc = rs_build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / source.replace(".hip", ".s"))
    cmd = [cc] + rs_build.CFLAGS + rs_build.EXTRA_CFLAGS.get(source, []) + ["--cuda-device-only", "-S", os.path.join(rs_build.CSRC, source),
                                                                             "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    with open(out) as f:
        text = f.read()
    kernels = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        kernels[name] = {k: get(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                             "group_segment_fixed_size")}
    return kernels


@pytest.fixture(scope="module")
def ppo_kernels(tmp_path_factory):
    return _metadata(tmp_path_factory, "rs_ppo.hip")


@pytest.fixture(scope="module")
def env_kernels(tmp_path_factory):
    return _metadata(tmp_path_factory, "rs_env.hip")


def _one(kernels, part):
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    return kernels[hits[0]]


def _lean(k):
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= 256, k


def test_pair_kernel_keeps_two_waves_per_simd(ppo_kernels):
    k = _one(ppo_kernels, "rs_ppo_grad2_pair_kernel")
    _lean(k)
    assert k["group_segment_fixed_size"] == 0, k          # all dynamic, held to 160 KB by the static_assert next to the launch


@pytest.mark.parametrize("kernel", ["rs_ppo_prepare_cols_kernel", "rs_ppo_prepare_sq_kernel", "rs_ppo_prepare_norm_kernel"])
def test_prepare_kernels_are_lean(env_kernels, kernel):
    k = _one(env_kernels, kernel)
    _lean(k)
    assert k["group_segment_fixed_size"] <= 4096, k
