"""CPU-only checks of the RRDB (RealESRGAN_x4plus) kernel path: the weight-fragment image against an index-by-index restatement of the layout
include/vd3d.h documents, the two new entry points in the header and the export list, the register / LDS budget of k_conv3x3_dense_f16 from hipcc's
own metadata, and the rule that without a GPU the network stays the module graph."""
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
PAIRS = [(64, 32), (96, 32), (128, 32), (160, 32), (192, 64), (64, 64)]


def _census(src):
    spec = importlib.util.spec_from_file_location("_vd3d_kernel_census", os.path.join(HERE, "test_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._census(src)


def _restated(w):
    """[step][t][l][j] = W[32t + (l & 31)][32c + 16kc + 8(l >> 5) + j][kh][kw], step = (c*9 + kh*3 + kw)*2 + kc: one element at a time."""
    co, ci = w.shape[:2]
    out = np.zeros((ci // 32 * 18, co // 32, 64, 8), np.float16)
    for c in range(ci // 32):
        for kh in range(3):
            for kw in range(3):
                for kc in range(2):
                    step = (c * 9 + kh * 3 + kw) * 2 + kc
                    for t in range(co // 32):
                        for l in range(64):
                            for j in range(8):
                                out[step, t, l, j] = w[32 * t + (l & 31), 32 * c + 16 * kc + 8 * (l >> 5) + j, kh, kw]
    return out


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_dense_weight_fragments_follow_the_documented_layout(cin, cout):
    from visiondepth3d_amd.upscale import dense_weight_fragments
    gen = torch.Generator().manual_seed(cin * 100 + cout)
    w = torch.randn(cout, cin, 3, 3, generator=gen).half()          # asymmetric in every index
    got = dense_weight_fragments(w)
    assert got.dtype == torch.float16 and got.is_contiguous() and tuple(got.shape) == (cin // 32 * 18, cout // 32, 64, 8)
    assert np.array_equal(got.numpy(), _restated(w.numpy()))


def test_dense_fragment_order_differs_from_the_c64_kernel_and_holds_the_same_elements():
    """The K order here is 32-channel-chunk-major (the channels are streamed through LDS in chunks of 32), that of conv_weight_fragments tap-major: for a
    [64,64,3,3] weight the two images are permutations of each other, step (c*9 + tap)*2 + kc here = step tap*4 + 2c + kc there."""
    from visiondepth3d_amd.upscale import conv_weight_fragments, dense_weight_fragments
    w = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(1)).half()
    a, b = dense_weight_fragments(w), conv_weight_fragments(w)
    assert tuple(a.shape) == tuple(b.shape) == (36, 2, 64, 8) and not torch.equal(a, b)
    for c in range(2):
        for tap in range(9):
            for kc in range(2):
                assert torch.equal(a[(c * 9 + tap) * 2 + kc], b[tap * 4 + 2 * c + kc])


def test_dense_weight_fragments_refuse_other_shapes():
    from visiondepth3d_amd.upscale import dense_weight_fragments
    for shape in [(48, 64, 3, 3), (64, 80, 3, 3), (64, 64, 1, 1)]:
        with pytest.raises(AssertionError):
            dense_weight_fragments(torch.zeros(shape))


def test_header_declares_and_exports_list_the_new_entry_points():
    from visiondepth3d_amd import _abi, _lib
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    for name in ("vd3d_conv3x3_dense_f16", "vd3d_nhwc_f16_to_planar3_f32"):
        assert re.search(r"\bint " + name + r"\(vd3d_ctx\* ctx,", hdr), name
        assert name in _lib.EXPORTS
    assert _abi.ABI_VERSION == 6 and "#define VD3D_ABI_VERSION 6" in hdr          # additive change


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_dense_kernel_fits_three_workgroups_per_cu():
    """The header comment of vd3d_conv_rdb.hip claims three resident workgroups per CU: 12 waves = 3 per SIMD, so at most 512 / 3 -> 168 registers per lane
    (allocation granule 8), nothing spilled, and no static LDS next to the 45 568-byte dynamic ring (3 x 45 568 <= 160 KB)."""
    k = _census("vd3d_conv_rdb.hip")
    dense = {n: v for n, v in k.items() if n.startswith("_Z19k_conv3x3_dense_f16")}
    assert len(dense) == 3, sorted(k)                                # C_out 32, C_out 64, C_out 64 with up2
    for n, v in dense.items():
        assert v["spill"] == 0 and v["vgpr"] <= 168 and v["lds"] == 0, (n, v)
    src = open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "vd3d_conv_rdb.hip")).read()
    assert "THREE workgroups per CU" in src and 3 * (2 * 4 * 5664 + 256) <= 160 * 1024
    for n, v in k.items():
        assert v["spill"] == 0, (n, v)


def test_on_the_cpu_the_rrdb_network_stays_the_module_graph():
    from visiondepth3d_amd.upscale import RRDBNet, Upscaler

    class _R:
        device = torch.device("cpu")
    torch.manual_seed(0)
    up = Upscaler(_R(), "RealESRGAN_x4_fp16", dtype=torch.float32, rrdb_hip=True)
    assert isinstance(up.net, RRDBNet) and up._rrdb is None and up._body is None
    up.net.body = torch.nn.Sequential(*list(up.net.body)[:1])       # one block is enough to see the graph run
    y = up._forward(torch.rand(1, 3, 6, 8))
    assert tuple(y.shape) == (1, 3, 24, 32) and y.dtype == torch.float32
    # the keyword exists with either value and fp16 on the CPU does not engage the kernels either
    assert Upscaler(_R(), "RealESRGAN_x4_fp16", dtype=torch.float16, rrdb_hip=True)._rrdb is None
    assert Upscaler(_R(), "RealESRGAN_x4_fp16", rrdb_hip=False)._rrdb is None
