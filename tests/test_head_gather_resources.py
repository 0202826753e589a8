"""Register / LDS budget of the head's coarse GEMM + in-LDS gather kernel (csrc/vd3d_head_gather.hip) from hipcc's own metadata for gfx950.  No GPU needed."""
import os
import re

import pytest

from conftest import ROOT
from test_neck_poly_resources import HIPCC, _census


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_gather_kernel_fits_one_workgroup_per_cu():
    """512-thread workgroups, one per CU: two waves per SIMD, so at most 256 registers per lane -- the A operand of the wave's groups (NG x C_in / 2), the fine
    pixels' accumulators (PPL x 32), one group's MFMA accumulators (16), a corner's eight 16-byte reads.  No spill, no private segment.  LDS is dynamic only (one
    object): two Z buffers of (448 | 256) rows x 36 floats, two weight buffers of C_in x 128 bytes and the row / column tables, 160 KB at most."""
    k = _census("vd3d_head_gather.hip")
    mains = {n: v for n, v in k.items() if n.startswith("_Z22k_head_conv_gather_f32")}
    assert len(mains) == 3 and all(any("ILi%dE" % c in n for n in mains) for c in (32, 64, 128)), sorted(k)
    src = open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "vd3d_head_gather.hip")).read()
    assert "hg_lds(64) == 146496 && hg_lds(32) == 138304 && hg_lds(128) == 107584 && hg_lds(64) <= 160 * 1024" in src      # the plan the source asserts at compile time
    dyn = {32: 2 * 448 * 36 * 4 + 2 * 32 * 128 + 8 * 34 * 4, 64: 2 * 448 * 36 * 4 + 2 * 64 * 128 + 8 * 34 * 4, 128: 2 * 256 * 36 * 4 + 2 * 128 * 128 + 8 * 34 * 4}
    assert dyn == {32: 138304, 64: 146496, 128: 107584}
    for n, v in mains.items():
        c = next(c for c in (32, 64, 128) if "ILi%dE" % c in n)
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 256, (n, v)
        assert v["lds"] == 0 and dyn[c] <= 160 * 1024, (n, v)
    pack = next(v for n, v in k.items() if n.startswith("_Z23k_head_conv_gather_pack"))
    assert pack["spill"] == 0 and pack["scratch"] == 0 and pack["lds"] == 0
