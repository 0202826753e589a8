"""Register / LDS budget of the two kernels behind DepthPipe(decoder=...) -- k_conv_epi (csrc/vd3d_conv_epi.hip: vd3d_conv_x3.h's body with EPI 2) and
k_depthpro_head (csrc/vd3d_depthpro_head.hip: EPI 3) -- checked offline from hipcc's own metadata and the Makefile's flags (no GPU needed): 512-thread
workgroups, two waves per SIMD, so at most 256 registers per lane; nothing spilled, no scratch, no static LDS; and the dynamic LDS they ask for is the plan of
the mode's bias-free kernels (cx_lds_m), read from the launchers.  The VGPR counts are recorded in profiles/r29_depth_pro_decoder.md."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visiondepth3d_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LDS_PLAN = {0: 155392, 1: 100864}   # cx_lds_m(mode, 128): the largest request of the mode's existing kernels (vd3d_conv_x3.hip, vd3d_conv_x2t.hip)


def _census(src):
    flags = None
    for ln in open(os.path.join(CSRC, "Makefile")):
        if ln.startswith("FLAGS"):
            flags = ln.split("=", 1)[1].replace("$(ARCH)", "gfx950").split()
    assert flags and "-ffp-contract=off" in flags       # the bit contract of vd3d_conv3x3_epi rests on it
    d = tempfile.mkdtemp()
    try:
        subprocess.run([HIPCC, *[f for f in flags if f != "-Wall"], "-I" + CSRC, "-c", os.path.join(CSRC, src), "-o", "x.o", "--save-temps"], cwd=d, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = open(glob.glob(os.path.join(d, "*gfx950.s"))[0]).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+).*?\.sgpr_spill_count: (\d+).*?\.vgpr_count:\s+(\d+).*?"
                         r"\.vgpr_spill_count: (\d+)", asm, re.S):
        out[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), sspill=int(m.group(4)), vgpr=int(m.group(5)), spill=int(m.group(6)))
    return out


def _cx_lds_m(mode, ck):
    """vd3d_conv_x3.h's plan, restated: two chunk images of `terms` x 2 planes of 340 pixels x 16 bytes, the 24 576-byte staging buffer, four weight stages."""
    terms = 3 if mode == 0 else 2
    stage = (terms * 2 * ck * 16 + 8191) // 8192 * 8192
    return 2 * terms * 2 * 340 * 16 + 24576 + 4 * stage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_conv_epi_instantiations_fit_two_waves_per_simd():
    k = _census("vd3d_conv_epi.hip")
    # mode 0 / 1 with 32 (8 x 1 waves), 64 (4 x 2, one N tile) and 128 / 256 (4 x 2, two N tiles; 256 as two slices) output channels
    want = [f"_Z10k_conv_epiILi{mode}ELi{wm}ELi{nwn}EE" for mode in (0, 1) for wm, nwn in ((8, 1), (4, 1), (4, 2))]
    assert sorted(k) == sorted(n for n in k if any(n.startswith(w) for w in want)) and len(k) == 6, sorted(k)
    for n, v in k.items():
        print("DECODER_RESOURCES", n, v)
        assert v["spill"] == 0 and v["sspill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 256 and v["lds"] == 0, (n, v)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_depthpro_head_instantiations_fit_two_waves_per_simd():
    k = _census("vd3d_depthpro_head.hip")
    heads = {n: v for n, v in k.items() if n.startswith("_Z15k_depthpro_headILi")}
    assert sorted(heads) == ["_Z15k_depthpro_headILi0EEv10vd_cx_args", "_Z15k_depthpro_headILi1EEv10vd_cx_args"], sorted(k)
    for n, v in k.items():                       # the two head kernels, the packer in both modes and the scale kernel
        print("DECODER_RESOURCES", n, v)
        assert v["spill"] == 0 and v["sspill"] == 0 and v["scratch"] == 0 and v["lds"] == 0, (n, v)
    for v in heads.values():
        assert v["vgpr"] <= 128, v               # 32 output channels: 2 x 16 accumulator registers -- room for four waves per SIMD


def test_the_launchers_ask_for_no_more_lds_than_the_modes_plan():
    """The dynamic LDS of a launch is its third launch argument: every request in the two translation units is cx_lds_m(MODE, CK) with CK <= 128."""
    assert _cx_lds_m(0, 128) == LDS_PLAN[0] and _cx_lds_m(1, 128) == LDS_PLAN[1]
    for src, cks in (("vd3d_conv_epi.hip", {"32", "64", "128"}), ("vd3d_depthpro_head.hip", {"32"})):
        text = open(os.path.join(CSRC, src)).read()
        launches = re.findall(r"hipLaunchKernelGGL\(\(?k_(?:conv_epi|depthpro_head)<[^)]*\)?, grid, dim3\(CX_NT\), (\w+)\((\w+), (\d+)\)", text)
        assert launches and {ck for _, _, ck in launches} == cks, launches
        for fn, mode, ck in launches:
            assert fn == "cx_lds_m" and mode in ("MODE", "0", "1")
            for m in ((0, 1) if mode == "MODE" else (int(mode),)):
                assert _cx_lds_m(m, int(ck)) <= LDS_PLAN[m] <= 160 * 1024
