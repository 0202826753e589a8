"""Host-side tests (no GPU) of the bf16x3 3 x 3 convolution (vd3d_conv3x3_x3, csrc/vd3d_conv_x3.hip) and of DepthPipe(conv="bf16x3"): the shape rule of the
host-only weight-bytes call, the constructor's argument checks, and the kernel's register / LDS census from hipcc's own metadata."""
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


def test_weight_bytes_rule():
    """C_in a positive multiple of 16, C_out 32 / 64 / 128 / 256; the image is the dense K-step images (96 C_out bytes per 16-channel chunk and tap) + the zero page."""
    from visiondepth3d_amd import _lib
    L = _lib.lib()
    for cin in (16, 48, 96, 256, 768, 1024):
        for cout in (32, 64, 128, 256):
            nb = L.vd3d_conv3x3_x3_weight_bytes(cin, cout)
            assert nb > 0 and nb >= cin * cout * 9 * 6 and nb % 16 == 0, (cin, cout, nb)   # three bf16 terms per weight
    for cin, cout in ((64, 16), (64, 512), (20, 64), (0, 64), (-16, 64), (8, 64), (64, 0), (64, 96)):
        assert L.vd3d_conv3x3_x3_weight_bytes(cin, cout) < 0, (cin, cout)


def test_constructor_validates_conv_before_it_touches_a_device():
    torch = pytest.importorskip("torch")
    from visiondepth3d_amd.depth import DepthPipe
    with pytest.raises(ValueError, match="conv"):
        DepthPipe("depth-anything-v2-small", device="cpu", dtype=torch.float32, gemm="f32", conv="bf16x3")
    with pytest.raises(ValueError):
        DepthPipe("depth-anything-v2-small", device="cpu", dtype=torch.float32, gemm="fp16x2", conv="bf16x3")
    with pytest.raises(ValueError, match="conv"):
        DepthPipe("depth-anything-v2-small", device="cpu", dtype=torch.float32, conv="nonsense")
    with pytest.raises(ValueError, match="conv"):
        DepthPipe("depth-anything-v2-small", device="cpu", dtype=torch.float32, gemm="bf16x3", conv="fp16x2")
    with pytest.raises(ValueError, match="gemm"):   # the existing order: an unknown gemm is named first
        DepthPipe("depth-anything-v2-small", device="cpu", dtype=torch.float32, gemm="nonsense", conv="nonsense")
    with pytest.raises(ValueError, match="renderer"):   # a valid pair still needs the GPU and a renderer
        DepthPipe("depth-anything-v2-small", device="cpu", dtype=torch.float32, gemm="bf16x3", conv="bf16x3")


def _census(src):
    """tests/test_kernel_resources.py's census (the Makefile's flags, --save-temps), plus the saved ISA itself."""
    flags = None
    for ln in open(os.path.join(CSRC, "Makefile")):
        if ln.startswith("FLAGS"):
            flags = ln.split("=", 1)[1].replace("$(ARCH)", "gfx950").split()
    assert flags and "-fno-slp-vectorize" in flags
    d = tempfile.mkdtemp()
    try:
        subprocess.run([HIPCC, *[f for f in flags if f != "-Wall"], "-I" + CSRC, "-c", os.path.join(CSRC, src), "-o", "x.o", "--save-temps"], cwd=d, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = open(glob.glob(os.path.join(d, "*gfx950.s"))[0]).read()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.sgpr_spill_count: (\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count: (\d+)", asm, re.S):
        out[m.group(2)] = dict(lds=int(m.group(1)), sgpr_spill=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    return out, asm


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_conv3x3_x3_census():
    """512-thread workgroups, two waves per SIMD: at most 256 registers, none spilled (vector or scalar); no static LDS in front of the dynamic array (or a
    multiple of 16: the fragments are ds_read_b128); bf16 MFMAs only; the launcher's dynamic LDS request within what a workgroup can have."""
    k, asm = _census("vd3d_conv_x3.hip")
    convs = {n: v for n, v in k.items() if n.startswith("_Z9k_conv_x3ILi")}
    plain = {n: v for n, v in convs.items() if re.match(r"_Z9k_conv_x3ILi0ELi\dELi\dELb0E", n)}   # K3S1 without epilogue options: this entry point's
    assert len(plain) == 3, sorted(k)   # 32, 64 and 128 output channels per workgroup (256 runs as two 128-channel halves)
    assert sum(n.startswith("_Z9k_conv_x3ILi0ELi4ELi2ELb0E") for n in plain) == 1 and len(convs) == 12, sorted(k)
    for n, c in convs.items():
        assert c["spill"] == 0 and c["sgpr_spill"] == 0 and c["vgpr"] <= 256 and c["lds"] % 16 == 0, (n, c)
    assert "v_mfma_f32_32x32x16_bf16" in asm and "v_mfma_f32_32x32x2_f32" not in asm
    assert "scratch_" not in asm
    src = open(os.path.join(CSRC, "vd3d_conv_x3.hip")).read()
    lds_max = int(re.search(r"#define CX_LDS_MAX (\d+)", src).group(1))
    assert "static_assert(cx_lds(128) == CX_LDS_MAX" in src   # the constant is tied to the launcher's own formula at compile time
    assert 0 < lds_max <= 163840
    # the same plan, from the layout constants: two A images, the float32 staging buffer, the four-stage ring of the 128-channel kernel
    a_img, stg, ring = 3 * 2 * (10 * 34) * 16, 3 * 512 * 16, 4 * 16384
    assert 2 * a_img + stg + ring == lds_max
