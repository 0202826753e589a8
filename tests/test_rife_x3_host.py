"""CPU-only checks of RifeSession(conv="bf16x3"): the weight rewrites (channel padding, merged heads, the transposed convolution as four phases) and the whole
operation list against torch in float64, the new entry points in the header and the export list, the register / LDS budget of csrc/vd3d_conv_x3.hip from
hipcc's own metadata, and the construction rules (no GPU, no renderer: ValueError, never a fall-back)."""
import importlib.util
import os
import re

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")
F = torch.nn.functional
HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ("vd3d_conv_ifn_weight_bytes", "vd3d_conv_ifn_pack_weights", "vd3d_conv_ifn", "vd3d_rife_warp_pack", "vd3d_rife_update", "vd3d_rife_blend")


def _census(src):
    spec = importlib.util.spec_from_file_location("_vd3d_kernel_census", os.path.join(HERE, "test_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._census(src)


@pytest.fixture(scope="module")
def net():
    from visiondepth3d_amd.rife import RifeNet, synthetic_weights_
    n = RifeNet()
    synthetic_weights_(n, 0)
    with torch.no_grad():                      # distinct PReLU slopes per channel, so that a permuted or dropped slope shows
        for name, p in n.named_parameters():
            if p.ndim == 1 and not name.endswith("bias"):
                p.copy_(torch.linspace(-0.3, 0.6, p.numel()))
    return n.double().eval()


def test_four_phase_form_equals_conv_transpose2d():
    from visiondepth3d_amd.rife import conv_transpose_4phase
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(6, 5, 4, 4, generator=g, dtype=torch.float64)          # asymmetric in every index
    b = torch.randn(5, generator=g, dtype=torch.float64)
    assert float((conv_transpose_4phase(x, w, b) - F.conv_transpose2d(x, w, b, 2, 1)).abs().max()) <= 1e-12
    assert float((conv_transpose_4phase(x, w, None) - F.conv_transpose2d(x, w, None, 2, 1)).abs().max()) <= 1e-12


def test_merged_heads_equal_the_two_separate_heads(net):
    from visiondepth3d_amd.rife import conv_transpose_4phase, merge_heads
    blk = net.block1
    feat = torch.randn(2, 90, 5, 7, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        flow, mask = blk.conv1(feat), blk.conv2(feat)
        (w1, b1, s1), (w2, b2) = merge_heads(blk)
        assert tuple(w1.shape) == (90, 90, 4, 4) and tuple(w2.shape) == (90, 5, 4, 4)
        h = conv_transpose_4phase(feat, w1, b1)
        h = torch.where(h >= 0, h, s1.view(1, -1, 1, 1) * h)
        out = conv_transpose_4phase(h, w2, b2)
    assert float((out[:, :4] - flow).abs().max()) <= 1e-12 and float((out[:, 4:] - mask).abs().max()) <= 1e-12
    assert float(w2[:45, 4].abs().max()) == 0 and float(w2[45:, :4].abs().max()) == 0      # block-diagonal


def test_padded_channels_change_nothing_and_stay_zero(net):
    from visiondepth3d_amd.rife import K3S1, K3S2, T4S2, ifnet_plan, pad_conv, run_layer_reference
    g = torch.Generator().manual_seed(2)
    conv, act = net.block0.conv0[1]
    x = torch.randn(1, 45, 6, 9, generator=g, dtype=torch.float64)
    w, b, s = pad_conv(K3S2, conv.weight.detach(), conv.bias.detach(), act.weight.detach(), 48, 96)
    assert tuple(w.shape) == (96, 48, 3, 3) and tuple(b.shape) == (96,) and tuple(s.shape) == (96,)
    xp = torch.cat((x, torch.zeros(1, 19, 6, 9, dtype=torch.float64)), 1)                    # a 64-pitch buffer, 48 channels read
    y = run_layer_reference(dict(kind=K3S2, w=w, b=b, slope=s, cin=48, cout=96), xp)
    with torch.no_grad():
        want = act(conv(x))
    assert float((y[:, :90] - want).abs().max()) <= 1e-12 and float(y[:, 90:].abs().max()) == 0
    wt, bt, _ = pad_conv(T4S2, torch.ones(90, 5, 4, 4), torch.ones(5), None, 96, 32)
    assert tuple(wt.shape) == (96, 32, 4, 4) and float(wt[90:].abs().max()) == 0 and float(wt[:, 5:].abs().max()) == 0 and float(bt[5:].abs().max()) == 0
    plans = ifnet_plan(net)
    assert [len(p) for p in plans] == [12, 12, 12]
    for p in plans:
        assert [ly["kind"] for ly in p] == [K3S2] * 2 + [K3S1] * 8 + [T4S2] * 2
        assert [(ly["cin"], ly["cout"]) for ly in p] == [(16, 64), (48, 96)] + [(96, 96)] * 9 + [(96, 32)]
        assert [ly["real"] for ly in p] == [(11, 45), (45, 90)] + [(90, 90)] * 9 + [(90, 5)]
        assert [ly["residual"] for ly in p] == [False] * 2 + [False, True] * 4 + [False] * 2
        assert p[-1]["slope"] is None and all(ly["slope"] is not None for ly in p[:-1])


def test_pixel_unit_warp_and_two_tap_downscale_equal_the_modules_ops():
    from visiondepth3d_amd.rife import backwarp, downscale_2tap, warp_pixels
    g = torch.Generator().manual_seed(3)
    img = torch.rand(2, 3, 32, 64, generator=g, dtype=torch.float64)
    flow = (torch.rand(2, 2, 32, 64, generator=g, dtype=torch.float64) * 2 - 1) * 40
    assert float((warp_pixels(img, flow) - backwarp(img, flow)).abs().max()) <= 1e-12
    for s in (1, 2, 4):
        want = F.interpolate(img, scale_factor=1.0 / s, mode="bilinear", align_corners=False, recompute_scale_factor=False)
        assert float((downscale_2tap(img, s) - want).abs().max()) <= 1e-14


@pytest.mark.parametrize("h,w", [(64, 96), (70, 100)])
def test_plan_forward_reference_is_the_same_function_as_the_module(net, h, w):
    """The operation list of RifeSession(conv="bf16x3") in float64 against RifeNet.forward in float64, batch 2: <= 1e-10, the rounding noise of a float64
    re-association on values of order 1.  70 x 100 takes the pad-and-crop path.  Measured: 1.1e-14 and 1.2e-14 with the synthetic weights."""
    from visiondepth3d_amd.rife import plan_forward_reference
    x = torch.rand(2, 6, h, w, generator=torch.Generator().manual_seed(h), dtype=torch.float64)
    with torch.no_grad():
        want = net(x)
    got = plan_forward_reference(net, x)
    assert got.shape == want.shape == (2, 3, h, w)
    d = float((got - want).abs().max())
    print("PLAN_VS_MODULE", h, w, d)
    assert d <= 1e-10, d
    assert float((want - 0.5 * (x[:, :3] + x[:, 3:])).abs().max()) > 1e-3      # the network moves content: the comparison is not one of two identities


def test_header_declares_and_exports_list_the_new_entry_points():
    from visiondepth3d_amd import _abi, _lib
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    for name in NEW:
        assert re.search(r"\bint(64_t)? " + name + r"\(", hdr), name
        assert name in _lib.EXPORTS
    assert _abi.ABI_VERSION == 6 and "#define VD3D_ABI_VERSION 6" in hdr          # additive change
    assert (_abi.IFN_K3S1, _abi.IFN_K3S2, _abi.IFN_T4S2) == (0, 1, 2)
    assert re.search(r"VD3D_IFN_K3S1 = 0, VD3D_IFN_K3S2 = 1, VD3D_IFN_T4S2 = 2", hdr)
    mk = open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "Makefile")).read()
    assert "vd3d_conv_ifn.hip" in mk and "vd3d_conv_x3.hip" in mk


def test_weight_bytes_query_names_the_built_shapes():
    """Host-only: 9 (3 x 3) or 16 (four phases of 2 x 2 taps) K steps of 96 C_out bytes per 16 input channels, plus the 64-byte zero page."""
    from visiondepth3d_amd import _lib
    L = _lib.lib()
    for kind, steps in ((0, 9), (1, 9), (2, 16)):
        for cin in (16, 48, 96):
            for cout in (32, 64, 96):
                assert L.vd3d_conv_ifn_weight_bytes(kind, cin, cout) == cin // 16 * steps * cout * 96 + 64
        assert L.vd3d_conv_ifn_weight_bytes(kind, 24, 32) < 0 and L.vd3d_conv_ifn_weight_bytes(kind, 16, 128) < 0 and L.vd3d_conv_ifn_weight_bytes(kind, 0, 32) < 0
    assert L.vd3d_conv_ifn_weight_bytes(3, 16, 32) < 0 and L.vd3d_conv_ifn_weight_bytes(-1, 16, 32) < 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_conv_ifn_kernels_fit_their_register_and_lds_budget():
    """Nine instantiations (three geometries x C_out 32 / 64 / 96) of 512-thread workgroups: two waves per SIMD, so at most 256 registers, nothing spilled; no
    static LDS in front of the dynamic array (a multiple of 16 keeps ds_read_b128 aligned); the launcher's largest dynamic-LDS request is CX_LDS_MAX <= 163 840,
    tied to the plan by the file's static_assert.  No kernel of the file spills.  (The other three instantiations are the DPT convolution's, without epilogue
    options: tests/test_conv_x3_host.py.)"""
    k = _census("vd3d_conv_x3.hip")
    convs = {n: v for n, v in k.items() if re.match(r"_Z9k_conv_x3ILi[012]ELi(8ELi1|4ELi1|8ELi3)ELb1E", n)}
    assert len(convs) == 9, sorted(k)
    assert len([n for n in k if n.startswith("_Z9k_conv_x3ILi")]) == 12, sorted(k)
    for n, v in convs.items():
        assert v["spill"] == 0 and v["vgpr"] <= 256 and v["lds"] % 16 == 0 and v["lds"] + 155392 <= 163840, (n, v)
    for n, v in k.items():
        assert v["spill"] == 0, (n, v)
    src = open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "vd3d_conv_x3.hip")).read()
    m = re.search(r"#define CX_LDS_MAX (\d+)", src)
    assert m and int(m.group(1)) == 155392 and int(m.group(1)) <= 163840
    assert "static_assert(cx_lds(128) == CX_LDS_MAX && cx_lds(96) == CX_LDS_MAX && cx_lds(64) <= CX_LDS_MAX && cx_lds(32) <= CX_LDS_MAX && CX_LDS_MAX <= 163840" in src
    assert 2 * (3 * 2 * 340 * 16) + 3 * 512 * 16 + 4 * 16384 == 155392            # the plan of the header comment: two chunk images, staging, four ring stages
    # every launch requests its plan's size (128: the DPT convolution's widest workgroup, launched from the same file)
    assert set(re.findall(r"cx_lds\((\d+)\), s, a\)", src)) == {"32", "64", "96", "128"}


def test_construction_rules():
    from visiondepth3d_amd.rife import RifeNet, RifeSession
    with pytest.raises(ValueError):
        RifeSession("cpu", conv="bf16x3")
    with pytest.raises(ValueError):
        RifeSession(conv="bf16x3")                                   # no renderer
    with pytest.raises(ValueError):
        RifeSession("cpu", conv="bf16x3", renderer=object())         # a renderer does not make the CPU a GPU
    with pytest.raises(ValueError):
        RifeSession("cpu", conv="fp16x2")
    s = RifeSession("cpu")
    assert isinstance(s.net, RifeNet) and s.conv is None and s.routes == []
    y = s(torch.rand(1, 6, 32, 32))
    assert tuple(y.shape) == (1, 3, 32, 32) and y.dtype == torch.float32
