"""The tiled CNN trunk kernels (rs_cnn_sized.hip) from the code objects inside the built library, without a GPU: no scratch, no VGPR
spills, VGPRs within the occupancy DESIGN.md states (forward three waves per SIMD, backward two) and LDS for at least two workgroups per
CU; and the C ABI's argument checks, which return before anything is launched."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

from radiation_ppo_amd import build

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _code_objects(blob: bytes):
    pos = 0
    while True:
        i = blob.find(b"\x7fELF", pos)
        if i < 0:
            return
        pos = i + 4
        if struct.unpack_from("<H", blob, i + 18)[0] != 224:             # EM_AMDGPU
            continue
        shoff, = struct.unpack_from("<Q", blob, i + 40)
        shentsize, shnum = struct.unpack_from("<HH", blob, i + 58)
        yield blob[i:i + shoff + shentsize * shnum]


@pytest.fixture(scope="module")
def sized_kernels():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
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
                if "rs_sized_trunk_" not in name:
                    continue
                val = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                out[name] = dict(vgpr=val("vgpr_count"), scratch=val("private_segment_fixed_size"), lds=val("group_segment_fixed_size"),
                                 vgpr_spill=val("vgpr_spill_count"))
    return out


@pytest.mark.parametrize("part,variants,max_vgpr,min_wg", [
    ("rs_sized_trunk_fwd", ("ILi6ELb1E", "ILi6ELb0E", "ILi4ELb1E", "ILi4ELb0E"), 168, 3),    # three waves per SIMD
    ("rs_sized_trunk_bwd", ("ILi6E", "ILi4E"), 256, 2),                                      # two waves per SIMD
])
def test_sized_trunk_kernels_fit_their_occupancy(sized_kernels, part, variants, max_vgpr, min_wg):
    for v in variants:
        hits = [k for k in sized_kernels if part + v in k]
        assert len(hits) == 1, (part + v, sorted(sized_kernels))
        k = sized_kernels[hits[0]]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (hits[0], k)
        assert k["vgpr"] <= max_vgpr, (hits[0], k)
        assert (160 * 1024) // k["lds"] >= min_wg, (hits[0], k)


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
