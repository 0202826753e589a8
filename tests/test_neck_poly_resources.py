"""Register / LDS budget of the float32 neck's polyphase kernel (csrc/vd3d_conv_poly.hip) from hipcc's own metadata for gfx950.  No GPU needed."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


def _census(src):
    """tests/test_kernel_resources.py's census, with the private segment (scratch) as well."""
    flags = None
    for ln in open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "Makefile")):
        if ln.startswith("FLAGS"):
            flags = ln.split("=", 1)[1].replace("$(ARCH)", "gfx950").split()
    assert flags and "-fno-slp-vectorize" in flags and "-ffp-contract=off" in flags
    d = tempfile.mkdtemp()
    try:
        subprocess.run([HIPCC, *[f for f in flags if f != "-Wall"], "-I" + os.path.join(ROOT, "visiondepth3d_amd", "csrc"), "-c",
                        os.path.join(ROOT, "visiondepth3d_amd", "csrc", src), "-o", "x.o", "--save-temps"], cwd=d, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = open(glob.glob(os.path.join(d, "*gfx950.s"))[0]).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count: (\d+)", asm, re.S):
        out[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_poly_kernel_fits_two_workgroups_per_cu():
    """256-thread workgroups (one wave per SIMD each), launched to run two per CU: at most 256 registers per lane -- C_OUT / 32 sixteen-register accumulators for the
    block and as many for the phase's total (128 for 128 output channels), the next slot's B operand and weight share under the MFMAs (16 + 16), the current B operand
    (16) and the A fragments of a step (16).  No spill, no private segment.  Static LDS only: the double-buffered weight slot, 2 x KS / 8 x 2 x C_OUT x 16 bytes =
    32 768 for (96 | 192) -> 128, 16 384 for 96 -> 64, 8 192 for 48 -> 64; two workgroups stay far below a CU's 160 KB."""
    k = _census("vd3d_conv_poly.hip")
    mains = {n: v for n, v in k.items() if n.startswith("_Z15k_conv_poly_f32")}
    assert len(mains) == 4, sorted(k)
    lds = {"ILi96ELi128ELi4E": 32768, "ILi192ELi128ELi2E": 32768, "ILi48ELi64ELi4E": 8192, "ILi96ELi64ELi2E": 16384}
    for n, v in mains.items():
        want = next(b for t, b in lds.items() if t in n)
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 256 and v["lds"] == want and 2 * v["lds"] <= 160 * 1024, (n, v)
    src = open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "vd3d_conv_poly.hip")).read()
    assert "2 * SLOT_F * 4 <= 65536" in src          # the plan the source asserts at compile time
    pack = next(v for n, v in k.items() if n.startswith("_Z16k_conv_poly_pack"))
    assert pack["spill"] == 0 and pack["scratch"] == 0 and pack["lds"] == 0
