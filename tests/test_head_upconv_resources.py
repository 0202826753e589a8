"""Register / LDS budget of the head's fine gather kernel (csrc/vd3d_head_upconv.hip) from hipcc's own metadata for gfx950.  No GPU needed."""
import os
import re

import pytest

from conftest import ROOT
from test_neck_poly_resources import HIPCC, _census


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_gather_kernel_fits_two_workgroups_per_cu():
    """256-thread workgroups, planned to run TWO per CU (one loads its window while the other sums): the staged window is dynamic LDS, HU_CY x HU_CX coarse pixels x
    9 taps x 8 channels x 4 bytes = 12 x 20 x 288 = 69 120 bytes, plus the static row / column tap tables (8 arrays of 18 | 34 entries: under 1 KB), so two
    workgroups take under 140 KB of a CU's 160 KB.  Two workgroups of 4 waves are 2 waves per SIMD (LDS is what bounds the occupancy): 256 registers per lane would do; the kernel
    stages its window with 17 sixteen-byte loads per lane in one batch (68 registers were they all in flight) and stays at or below 128.  No spill, no private segment (a partially written register array once went to scratch)."""
    k = _census("vd3d_head_upconv.hip")
    mains = {n: v for n, v in k.items() if n.startswith("_Z24k_head_upconv_gather_f32")}
    assert len(mains) == 2 and any("ILi64E" in n for n in mains) and any("ILi32E" in n for n in mains), sorted(k)
    src = open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "vd3d_head_upconv.hip")).read()
    geo = {n: int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("HU_TH", "HU_TW", "HU_CY", "HU_CX", "HU_CC", "HU_NT")}
    assert geo == dict(HU_TH=16, HU_TW=32, HU_CY=12, HU_CX=20, HU_CC=8, HU_NT=256)
    dyn = geo["HU_CY"] * geo["HU_CX"] * 9 * geo["HU_CC"] * 4
    assert dyn == 69120 and "hu_lds()" in src and "<= 160 * 1024" in src      # the plan the source asserts at compile time
    for n, v in mains.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 128, (n, v)
        assert v["lds"] <= 1024 and 2 * (v["lds"] + dyn) <= 160 * 1024, (n, v)
