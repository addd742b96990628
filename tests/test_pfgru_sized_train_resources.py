"""The training-pass kernels of the sized PFGRU (rs_pfgru_sized_train.hip) from the code objects inside the built library, without a
GPU: per instantiation the VGPR count and the LDS bytes within what the file header states, no scratch and no VGPR spill (the header
claims 0 at every width; DESIGN.md section 3 records it)."""
import os
import re
import subprocess
import tempfile

import pytest

from radiation_ppo_amd import build

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
LDS_PER_CU = 160 * 1024
WIDTHS = (8, 16, 24, 32, 40, 48, 56, 64)
# csrc/rs_pfgru_sized_train.hip, "Resources per width": (VGPR bound, LDS KB bound, waves per SIMD = workgroups per CU) per walk
FWD = {8: (128, 9.3, 4), 16: (128, 16.8, 4), 24: (128, 24.3, 4), 32: (128, 31.8, 4), 40: (128, 39.3, 4), 48: (128, 46.8, 3),
       56: (128, 54.3, 2), 64: (128, 61.8, 2)}
BWD = {8: (128, 21.4, 4), 16: (128, 31.5, 4), 24: (128, 39.0, 4), 32: (168, 49.1, 3), 40: (168, 56.6, 2), 48: (256, 66.6, 2),
       56: (256, 74.1, 2), 64: (256, 84.2, 1)}


@pytest.fixture(scope="module")
def train_kernels():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    from test_rnn_sized_resources import _code_objects
    lib = build.build(verbose=False)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n, co in enumerate(_code_objects(open(lib, "rb").read())):
            path = os.path.join(tmp, f"co{n}.elf")
            with open(path, "wb") as f:
                f.write(co)
            notes = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                if "rs_pfgru_sized_train_" not in name and "rs_pfgru_sized_draws_" not in name:
                    continue
                val = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                out[name] = dict(vgpr=val("vgpr_count"), agpr=int(re.match(r"\s*(\d+)", block).group(1)), scratch=val("private_segment_fixed_size"),
                                 vgpr_spill=val("vgpr_spill_count"), lds=val("group_segment_fixed_size"))
    return out


@pytest.mark.parametrize("walk", ["fwd", "bwd"])
@pytest.mark.parametrize("H", WIDTHS)
def test_sized_train_kernels_fit_their_stated_resources(train_kernels, H, walk):
    hits = [k for k in train_kernels if f"rs_pfgru_sized_train_{walk}_kernelILi{H}E" in k]
    assert len(hits) == 1, (H, walk, sorted(train_kernels))
    k = train_kernels[hits[0]]
    vgpr, lds_kb, waves = (FWD if walk == "fwd" else BWD)[H]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (hits[0], k)
    assert k["vgpr"] <= vgpr and k["agpr"] == 0, (hits[0], k)
    assert k["lds"] <= lds_kb * 1024, (hits[0], k)
    assert min(LDS_PER_CU // k["lds"], 512 // ((k["vgpr"] + 7) // 8 * 8)) >= waves, (hits[0], k)      # the stated occupancy is reachable


def test_sized_draws_kernel_has_no_scratch(train_kernels):
    hits = [k for k in train_kernels if "rs_pfgru_sized_draws_kernel" in k]
    assert len(hits) == 1 and train_kernels[hits[0]]["scratch"] == 0 and train_kernels[hits[0]]["lds"] == 0
