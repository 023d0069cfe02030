"""The resource budget of the default pair kernel, read from the code object's metadata on the host (no GPU).

k_rdf_pencil<0, true, 0, true, 2> - same set, orthorhombic periodic cell, one histogram per block, folded pop: the kernel of the default
benchmark line - runs eight waves per SIMD.  That holds while it needs at most 64 VGPRs, no scratch, and little enough LDS for eight
blocks of four waves on a CU (160 KB / 8 = 20 KB).  The figures are the kernel's .vgpr_count, .private_segment_fixed_size and
.group_segment_fixed_size in the AMDGPU metadata note of the gfx950 code object embedded in the library; resource metadata only, no
instructions are looked at."""
import os
import re
import shutil
import struct
import subprocess

import pytest

KERNEL = "_Z12k_rdf_pencilILi0ELb1ELi0ELb1ELi2EEv17vmd_pair_params_t"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _readelf():
    for exe in (shutil.which("llvm-readelf"), "/opt/rocm/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-readelf"):
        if exe and os.path.exists(exe):
            return exe
    return None


def _section(elf, name):
    """bytes of one section of a little-endian ELF64 image"""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)

    def header(i):
        sh_name, _, _, _, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize)
        return sh_name, off, size

    _, stroff, strsize = header(shstrndx)
    strtab = elf[stroff:stroff + strsize]
    for i in range(shnum):
        sh_name, off, size = header(i)
        if strtab[sh_name:strtab.index(b"\0", sh_name)] == name.encode():
            return elf[off:off + size]
    raise AssertionError(f"no section {name}")


def _gfx950_code_objects(fatbin):
    """the device images for gfx950 of every offload bundle in .hip_fatbin (one bundle per HIP translation unit)"""
    out = []
    pos = fatbin.find(BUNDLE_MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fatbin, pos + len(BUNDLE_MAGIC))
        p = pos + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, p)
            triple = fatbin[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(fatbin[pos + off:pos + off + size])
        pos = fatbin.find(BUNDLE_MAGIC, pos + 1)
    return out


def _kernel_metadata(tmp_path):
    """{field: value} of KERNEL from the metadata notes, as llvm-readelf prints them"""
    from viamd_amd import build as vb
    lib = vb.build()
    objs = _gfx950_code_objects(_section(open(lib, "rb").read(), ".hip_fatbin"))
    assert objs, "the library embeds no gfx950 code object"
    for i, co in enumerate(objs):
        path = tmp_path / f"gfx950_{i}.co"
        path.write_bytes(co)
        notes = subprocess.run([_readelf(), "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        # one YAML mapping per kernel under amdhsa.kernels: its first line is "- .key:" two columns left of the other keys' indent
        name = re.search(r"^( +)\.name:\s+" + re.escape(KERNEL) + r"\s*$", notes, re.M)
        if not name:
            continue
        opener = "\n" + " " * (len(name.group(1)) - 2) + "- "
        beg = notes.rfind(opener, 0, name.start())
        end = notes.find(opener, name.end())
        block = notes[beg:end if end >= 0 else len(notes)]
        return {k: v for k, v in re.findall(r"^ +(?:- )?\.(\w+):[ \t]+(\S+)[ \t]*$", block, re.M)}
    raise AssertionError(f"{KERNEL} is not in the library's gfx950 code objects")


@pytest.mark.skipif(_readelf() is None, reason="no llvm-readelf to read the code object's notes with")
def test_default_pair_kernel_keeps_the_budget_of_eight_waves(tmp_path):
    md = _kernel_metadata(tmp_path)
    print({k: md[k] for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "sgpr_count")})
    assert int(md["vgpr_count"]) <= 64, "more than 64 VGPRs: the eighth wave per SIMD is gone"
    assert int(md["private_segment_fixed_size"]) == 0, "the kernel spills to scratch"
    assert int(md["group_segment_fixed_size"]) <= 20 * 1024, "more LDS than eight blocks per CU can have"
