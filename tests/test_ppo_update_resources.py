"""Resources of the PPO update's kernels, from a cross-compile of rs_ppo.hip to gfx950 assembly (no GPU needed): both K7 kernels keep
two waves per SIMD (no scratch, at most 256 VGPRs) with the parallel epilogue, the translation unit still compiles (the static_asserts on
K7's LDS size hold), and the fused tail kernel writes memory with vector instructions only."""
import os
import re
import subprocess

import pytest

from radiation_ppo_amd import build as rs_build

SRC = os.path.join(rs_build.CSRC, "rs_ppo.hip")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    try:
        cc = rs_build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "rs_ppo.s")
    cmd = [cc] + rs_build.CFLAGS + rs_build.EXTRA_CFLAGS.get("rs_ppo.hip", []) + ["--cuda-device-only", "-S", SRC, "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)       # a failing static_assert fails here
    with open(out) as f:
        return f.read()


def _body(isa, mangled_part):
    """instruction lines of the one kernel whose mangled name contains `mangled_part`"""
    m = re.search(r"^(_Z\w*" + re.escape(mangled_part) + r"\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", isa, re.S | re.M)
    assert m, mangled_part
    return m.group(1), m.group(2)


def _meta(isa, name):
    """the kernel's entry in the amdhsa.kernels metadata"""
    blocks = [b for b in isa.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+" + re.escape(name) + r"\s", b)]
    assert len(blocks) == 1, name
    get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blocks[0]).group(1))
    return {k: get(k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}


@pytest.mark.parametrize("nout", [8, 1])
def test_k7_keeps_two_waves_per_simd(isa, nout):
    name, body = _body(isa, f"rs_ppo_grad2_kernelILi{nout}E")
    k = _meta(isa, name)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= 256, k
    assert k["group_segment_fixed_size"] == 0, k          # all dynamic, held to 160 KB by the static_assert next to the launch
    assert not re.search(r"^\s*scratch_", body, re.M)


@pytest.mark.parametrize("kernel", ["rs_ppo_tail_kernel", "rs_ppo_grad2_kernelILi8E", "rs_ppo_grad2_kernelILi1E"])
def test_no_scalar_memory_writes(isa, kernel):
    name, body = _body(isa, kernel)
    k = _meta(isa, name)
    assert k["private_segment_fixed_size"] == 0, k
    # any scalar-unit instruction that stores, does an atomic, or writes back / drops the scalar data cache
    bad = re.compile(r"^\s*s_\w*(store|atomic)\w*|^\s*s_d" + r"cache_\w+", re.M)
    hits = [m.group(0).strip() for m in bad.finditer(body)]
    assert not hits, hits
    assert re.search(r"^\s*global_store_", body, re.M)      # and it does write, through the vector memory path
