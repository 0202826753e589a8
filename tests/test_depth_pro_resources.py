"""Register / scratch / LDS census of DepthPro's kernels (csrc/vd3d_depthpro.hip: the front end and the post-process in its 16-byte and 4-byte store form), read offline from hipcc's own metadata with the Makefile's flags (no GPU needed).  None may spill or use scratch.  All are
memory-bound 256-thread workgroups (one wave per SIMD each) whose launch code assumes nothing but that plenty of them are resident: at most 64 registers keeps
eight workgroups per CU (8 x 64 <= 512).  Only the front end uses LDS: its 3 x 256-entry table of the byte, 3 KB.  Resources only -- nothing else in the code
object is looked at."""
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
def test_depth_pro_kernels_use_no_scratch_and_fit_eight_workgroups_per_cu():
    k = _census("vd3d_depthpro.hip")
    names = {"preprocess": "_Z15k_dp_preprocess", "post_vec": "_Z9k_dp_postILb1E", "post_scalar": "_Z9k_dp_postILb0E"}
    assert len(k) == len(names), sorted(k)
    for what, prefix in names.items():
        v = next(v for n, v in k.items() if n.startswith(prefix))
        print("DEPTH_PRO_RESOURCES", what, v)
        assert v["spill"] == 0 and v["scratch"] == 0, (what, v)
        assert 8 * ((v["vgpr"] + 7) // 8 * 8) <= 512, (what, v)
        assert v["lds"] == (3 * 256 * 4 if what == "preprocess" else 0), (what, v)
