"""Kernel metadata for the tests/test_*_resources.py files, read without a GPU from the code objects inside the built library: the
library is a host ELF carrying one AMDGPU ELF per translation unit; each is cut out and its amdhsa.kernels notes are read with
llvm-readelf --notes.  Numbers only: nothing here returns or scans a kernel's instructions.

A resource test for a new kernel: state the bound in a table in your test file, call library_kernels(), and look the kernel up
with one()."""
import functools
import os
import re
import struct
import subprocess
import tempfile

import pytest

from radiation_ppo_amd import build

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KEYS = dict(vgpr="vgpr_count", agpr="agpr_count", scratch="private_segment_fixed_size", vgpr_spill="vgpr_spill_count",
            sgpr_spill="sgpr_spill_count", lds="group_segment_fixed_size")


class Record(dict):
    """a kernel's numbers; a dict under another name, because pytest cuts a plain dict in an assert's message to four entries"""


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


def _records(metadata: str):
    """amdhsa.kernels entries (every entry starts with its .agpr_count) -> {mangled name: Record}; a record carries its name, so
    that an assert which prints the record names the kernel"""
    out = {}
    for block in metadata.split("- .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = Record({k: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1)) for k, key in KEYS.items()}, name=name)
    return out


@functools.lru_cache(maxsize=None)
def library_kernels():
    """{mangled name: {vgpr, agpr, scratch, vgpr_spill, sgpr_spill, lds, name}} of every kernel in the built library"""
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    lib = build.build(verbose=False)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n, co in enumerate(_code_objects(open(lib, "rb").read())):
            path = os.path.join(tmp, f"co{n}.elf")
            with open(path, "wb") as f:
                f.write(co)
            out.update(_records(subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout))
    assert len(out) > 40
    return out


def one(kernels, *parts):
    """the record of the single kernel whose mangled name contains every part"""
    hits = [k for k in kernels if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, hits or sorted(kernels))
    return kernels[hits[0]]


def waves_by_vgpr(vgpr: int) -> int:
    """VGPRs and AGPRs are one 512-entry-per-lane file per SIMD, allocated in granules of 8 registers per lane: waves per SIMD
    allowed by registers = min(8, 512 // alloc), alloc = vgpr rounded up to the granule"""
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def workgroups_by_lds(lds: int) -> int:
    """workgroups per CU <= 160 KiB / LDS per workgroup (lds: the kernel's static bytes)"""
    return (160 * 1024) // lds
