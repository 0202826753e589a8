"""Register / scratch / LDS census of the BiT-prefix kernels (csrc/vd3d_bit.hip: im2col in its vector and scalar form, the max-pool, GroupNorm's two statistics
passes and its apply pass), read offline from hipcc's own metadata with the Makefile's flags (no GPU needed).  None may spill or use scratch.  All six are memory-bound 256-thread workgroups (one
wave per SIMD each): at most 96 registers keeps five of them resident per CU (5 x 96 <= 512), and the GroupNorm kernels' LDS (per-group statistics, the pixel
rows' partials; the apply pass keeps rstd in float64) is at most 6 KB."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _census(src):
    flags = None
    for ln in open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "Makefile")):
        if ln.startswith("FLAGS"):
            flags = ln.split("=", 1)[1].replace("$(ARCH)", "gfx950").split()
    assert flags and "-ffp-contract=off" in flags
    d = tempfile.mkdtemp()
    try:
        subprocess.run([HIPCC, *[f for f in flags if f != "-Wall"], "-I" + os.path.join(ROOT, "visiondepth3d_amd", "csrc"), "-c",
                        os.path.join(ROOT, "visiondepth3d_amd", "csrc", src), "-o", "x.o", "--save-temps"], cwd=d, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = open(glob.glob(os.path.join(d, "*gfx950.s"))[0]).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+).*?\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)"
                         r".*?\.vgpr_spill_count: (\d+)", asm, re.S):
        out[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), sgpr=int(m.group(4)), vgpr=int(m.group(5)), spill=int(m.group(6)))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_bit_stem_kernels_use_no_scratch_and_fit_five_workgroups_per_cu():
    k = _census("vd3d_bit.hip")
    names = {"im2col_vec": "_Z8k_im2colILb1E", "im2col_scalar": "_Z8k_im2colILb0E", "maxpool": "_Z15k_maxpool3x3_s2", "gn_sum": "_Z10k_gn_statsILi0E",
             "gn_sq": "_Z10k_gn_statsILi1E", "gn_apply": "_Z10k_gn_apply"}
    assert len(k) == len(names), sorted(k)
    for what, prefix in names.items():
        v = next(v for n, v in k.items() if n.startswith(prefix))
        print("BIT_STEM_RESOURCES", what, v)
        assert v["spill"] == 0 and v["scratch"] == 0, (what, v)
        assert 5 * ((v["vgpr"] + 7) // 8 * 8) <= 512, (what, v)
        assert v["lds"] <= (6144 if what.startswith("gn_") else 0), (what, v)
