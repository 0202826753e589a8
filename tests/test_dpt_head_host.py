"""Host-side checks of the fused DPT head kernel (csrc/vd3d_conv_head.hip, vd3d_dpt_head_conv_f32): weight image layout, register / LDS budget from hipcc's
own metadata, and the C boundary.  No GPU needed."""
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from visiondepth3d_amd import _abi, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
BUILT = ((32, 32), (64, 32), (128, 32), (128, 64))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def pack_restated(w):
    """The weight image of vd3d_dpt_head_conv_pack_weights restated: [Cout][Cin][3][3] -> [chunk Cin / 16][tap 9][quad 4][oc Cout][4 floats], channel
    chunk * 16 + quad * 4 + e of tap ky * 3 + kx."""
    import torch
    Cout, Cin = w.shape[:2]
    return w.reshape(Cout, Cin // 16, 4, 4, 9).permute(1, 4, 2, 0, 3).contiguous().reshape(-1)


def test_weight_image_layout_round_trips():
    """The restated layout against the index formula the kernel reads with (A fragment of tap t, quad q, channel oc at ((t * 4 + q) * Cout + oc) * 4 floats
    inside a chunk of 9 * 4 * Cout * 4 floats), and back to the weight."""
    import torch
    for Cin, Cout in BUILT:
        w = torch.arange(Cout * Cin * 9, dtype=torch.float32).reshape(Cout, Cin, 3, 3)
        img = pack_restated(w)
        assert img.numel() * 4 == Cin * 9 * Cout * 4
        rng = np.random.default_rng(Cin + Cout)
        for _ in range(200):
            oc, ci, tap = int(rng.integers(Cout)), int(rng.integers(Cin)), int(rng.integers(9))
            chunk, q, e = ci // 16, (ci % 16) // 4, ci % 4
            at = chunk * (9 * 4 * Cout * 4) + ((tap * 4 + q) * Cout + oc) * 4 + e
            assert float(img[at]) == float(w[oc, ci, tap // 3, tap % 3])
        back = img.reshape(Cin // 16, 9, 4, Cout, 4).permute(3, 0, 2, 4, 1).reshape(Cout, Cin, 3, 3)
        assert torch.equal(back, w)


def test_weight_bytes_names_the_built_shapes(L):
    for Cin in (16, 32, 48, 64, 96, 128, 256):
        for Cout in (16, 32, 64, 128):
            nb = L.vd3d_dpt_head_conv_weight_bytes(Cin, Cout)
            assert nb == (Cin * 9 * Cout * 4 if (Cin, Cout) in BUILT else -1), (Cin, Cout, nb)


def _census(src):
    spec = importlib.util.spec_from_file_location("_vd3d_kernel_census", os.path.join(HERE, "test_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._census(src)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_head_kernel_fits_two_waves_per_simd():
    """512-thread workgroups, one per CU (97 - 129 KB of dynamic LDS), so two waves per SIMD: the kernel is designed for that occupancy, at most 256
    registers per lane.  They hold 3 (C_OUT 32) or 6 (C_OUT 64) sixteen-register accumulators (the running total and the two chains of a chunk), the next
    chunk's 12 + W_ITERS sixteen-byte loads under the MFMAs (64 / 72 registers) and the chunk-invariant interpolation geometry; measured 158 - 187 (C_OUT
    32) and 254 (C_OUT 64).  No spills, no private segment, no static LDS (the images are dynamic LDS: 2 x 24 832 + 2 x 24 576 = 98 816 bytes for 32 output
    channels, 2 x 24 832 + 2 x 40 960 = 131 584 for 64, set per device through the > 64 KB opt-in)."""
    k = _census("vd3d_conv_head.hip")
    mains = {n: v for n, v in k.items() if n.startswith("_Z16k_conv3x3_up_f32")}
    assert len(mains) == 4, sorted(k)
    for n, v in mains.items():
        assert v["spill"] == 0 and v["vgpr"] <= 256 and v["lds"] == 0, (n, v)
    src = open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "vd3d_conv_head.hip")).read()
    assert "ch_lds(32) == 98816 && ch_lds(64) == 131584" in src                 # the plan the source asserts at compile time
    assert 131584 <= 160 * 1024


def test_header_abi_and_exports_agree(L):
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    declared = set(re.findall(r"\b(vd3d_[a-z0-9_]+)\s*\(", hdr))
    new = {"vd3d_dpt_head_conv_weight_bytes", "vd3d_dpt_head_conv_pack_weights", "vd3d_dpt_head_conv_f32"}
    assert new <= declared and new <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    for n in new:
        assert hasattr(L, n), n
    assert _abi.ABI_VERSION == 6 and L.vd3d_abi_version() == 6
    assert re.search(r"#define\s+VD3D_ABI_VERSION\s+6\b", hdr)
    # pure host refusals: no context is needed to be told that a shape is not built
    assert L.vd3d_dpt_head_conv_pack_weights(None, None, 64, 32, None) == _abi.E_INVALID
    assert L.vd3d_dpt_head_conv_f32(None, None, None, 1, 5, 7, 9, 13, 64, None, 32, None, None, 0.0, 1.0, None) == _abi.E_INVALID
