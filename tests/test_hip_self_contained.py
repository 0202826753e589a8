"""GPU tests (-m gpu) of DepthPipe(self_contained=True) and of the two kernels it adds: vd3d_conv3x3_s2_x3 (csrc/vd3d_conv_s2.hip: the tile convolution's
stride-2 geometry with 128-channel slices) and vd3d_patchify_f32 (csrc/vd3d_netops.hip).

Kernel level: the stride-2 convolution against FLOAT64 beside PyTorch's float32 CPU convolution, with the bars of test_conv3x3_x3_is_float32_faithful; exact
small-integer cases; NaN containment (the reason the geometry runs no zero-weight tap); the refusals; the weight image and the patch rows bit for bit against
the numpy statements of tests/test_self_contained_host.py.

Depth leg: depth-anything-v2-small with synthetic weights at a 9 x 17 patch grid (maps 36 x 68, 18 x 34, 9 x 17 and 5 x 9: every new route, the odd-size path
of the stride-2 kernel included).  No vendor-library operator is dispatched; the prediction is float32-faithful against the stock module in float64 on the CPU
(the stock float32 module on the CPU is the yardstick; bars of tests/test_hip_depth_f64.py); the uint8 plane meets the stock float32 GPU graph's; forwards
repeat bit for bit and a frame's prediction does not depend on its batch; the flop count equals the library mode's.  Every network is fed the pipe's own
pre-processed pixel values (vd3d_depth_preprocess is not under test here), widened exactly for float64."""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
CL = torch.channels_last

from test_self_contained_host import patchify_reference, s2_image_reference, unfold_rows   # noqa: E402


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _conv_s2(R, x, w):
    img = R.conv3x3_s2_x3_pack(w)
    assert img is not None
    return R.conv3x3_s2_x3(x.contiguous(memory_format=CL), img, w.shape[0])


S2_CASES = [(1, 1, 1, 16, 128),       # one pixel
            (1, 2, 2, 16, 128),       # one output pixel fed by all four sub-pixels
            (1, 16, 64, 32, 384),     # exactly one 8 x 32 output tile, three slices
            (2, 17, 65, 48, 256),     # odd sizes, one pixel past a tile on both axes, batch 2
            (1, 37, 66, 64, 128),     # the model's own map
            (1, 5, 9, 1024, 128)]     # 576 K steps


@pytest.mark.parametrize("B,H,W,Cin,Cout", S2_CASES)
def test_conv3x3_s2_x3_is_float32_faithful(R, B, H, W, Cin, Cout):
    """vd3d_conv3x3_s2_x3 against a float64 convolution, beside PyTorch's float32 CPU F.conv2d(stride=2, padding=1) on the same operands, with the bars of
    test_conv3x3_x3_is_float32_faithful: maximum of |y - y64| / conv(|x|, |w|) <= max(2.5 x the yardstick's, 2^-21), relative RMS <= 1.5 x the yardstick's
    + 1e-9.  Post-ReLU inputs with log-normal channel scales.  Two calls return identical bits."""
    g = torch.Generator(device="cuda").manual_seed(B * 100 + H)
    x = torch.relu(torch.randn(B, Cin, H, W, device="cuda", generator=g)) * torch.exp(torch.randn(1, Cin, 1, 1, device="cuda", generator=g))
    x = x.contiguous(memory_format=CL)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) * 0.05
    img = R.conv3x3_s2_x3_pack(w)
    assert img is not None
    y = R.conv3x3_s2_x3(x, img, Cout)
    assert y.shape == (B, Cout, (H + 1) // 2, (W + 1) // 2) and y.is_contiguous(memory_format=CL) and bool(torch.isfinite(y).all())
    ref = F.conv2d(x.double(), w.double(), None, 2, 1)
    y32 = F.conv2d(x.cpu(), w.cpu(), None, 2, 1).to(x.device)
    scale = F.conv2d(x.abs().double(), w.abs().double(), None, 2, 1) + 1e-30
    e3, e32 = float(((y.double() - ref).abs() / scale).max()), float(((y32.double() - ref).abs() / scale).max())
    r3 = float((y.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    r32 = float((y32.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"CONV_S2_X3_ERR {B}x{H}x{W}x{Cin}->{Cout} max {e3:.3e} (f32 {e32:.3e}, {e3 / max(e32, 1e-30):.2f}x) rms {r3:.3e} (f32 {r32:.3e}, {r3 / max(r32, 1e-30):.2f}x)")
    assert e3 <= max(2.5 * e32, 2.0 ** -21), (e3, e32)
    assert r3 <= 1.5 * r32 + 1e-9, (r3, r32)
    assert torch.equal(R.conv3x3_s2_x3(x, img, Cout), y)


@pytest.mark.parametrize("Cout", [128, 384])
def test_conv3x3_s2_x3_exact_small_integers_pin_the_geometry(R, Cout):
    """Small integers on both sides: one bf16 term per operand and conv(|x|, |w|) < 2^24, so every sum is exact in any order and the answer is the integer one --
    a swapped sub-pixel, a mirrored tap, a shifted halo, a permuted channel slice shows.  Odd sizes on both axes, two frames, three chunks."""
    B, Cin, H, W = 2, 48, 19, 67
    x = ((torch.arange(B * Cin * H * W, device="cuda").view(B, Cin, H, W) * 7) % 5 - 2).float()
    w = ((torch.arange(Cout * Cin * 9, device="cuda").view(Cout, Cin, 3, 3) * 11) % 7 - 3).float()
    assert float(F.conv2d(x.abs().double(), w.abs().double(), None, 2, 1).max()) < 2 ** 24
    assert torch.equal(_conv_s2(R, x, w).double(), F.conv2d(x.double(), w.double(), None, 2, 1))


@pytest.mark.parametrize("py,px", [(4, 6), (5, 6), (4, 7), (5, 7), (0, 0), (8, 32)])
def test_conv3x3_s2_x3_nan_stays_inside_its_windows(R, py, px):
    """One NaN input pixel (each of the four sub-pixel parities, a corner, the last pixel) gives NaN in exactly the outputs whose 3 x 3 window holds it: output (q, r)
    reads rows 2 q - 1 .. 2 q + 1.  A zero-weight tap on the space-to-depth view would carry it further."""
    H, W = 9, 33
    x = torch.ones(1, 16, H, W, device="cuda")
    x[0, 5, py, px] = float("nan")
    y = _conv_s2(R, x, torch.ones(128, 16, 3, 3, device="cuda"))
    q = torch.arange((H + 1) // 2, device="cuda").view(-1, 1)
    r = torch.arange((W + 1) // 2, device="cuda").view(1, -1)
    holds = ((2 * q - 1 <= py) & (py <= 2 * q + 1) & (2 * r - 1 <= px) & (px <= 2 * r + 1))
    assert 1 <= int(holds.sum()) <= 4
    assert torch.equal(torch.isnan(y[0]), holds.expand(128, -1, -1))


def test_conv3x3_s2_x3_weight_image_is_the_schedule_order(R):
    """The device packer against the numpy statement of the kernel's schedule, every byte, the zero page included."""
    w = torch.randn(256, 48, 3, 3, generator=torch.Generator().manual_seed(9)) * 0.05
    img = R.conv3x3_s2_x3_pack(w.cuda())
    assert np.array_equal(img.cpu().numpy(), s2_image_reference(w.numpy()))


def test_conv3x3_s2_x3_refuses_what_it_does_not_build(R):
    from visiondepth3d_amd import _lib
    assert R.conv3x3_s2_x3_pack(torch.zeros(96, 16, 3, 3, device="cuda")) is None       # C_out 96
    assert R.conv3x3_s2_x3_pack(torch.zeros(128, 24, 3, 3, device="cuda")) is None      # C_in 24
    assert R.conv3x3_s2_x3_pack(torch.zeros(128, 16, 1, 1, device="cuda")) is None      # not 3 x 3
    L = _lib.lib()
    img = R.conv3x3_s2_x3_pack(torch.zeros(128, 16, 3, 3, device="cuda"))
    buf = torch.zeros(2 * 16 * 4 * 4 + 4, device="cuda")
    out = torch.zeros(2 * 128 * 2 * 2, device="cuda")
    vp = ctypes.c_void_p
    call = lambda xp, B, Cin=16, Cout=128, H=4: L.vd3d_conv3x3_s2_x3(R._ctx, vp(xp), B, H, 4, Cin, vp(img.data_ptr()), Cout, vp(out.data_ptr()))   # noqa: E731
    assert call(buf.data_ptr(), 1, Cout=96) == -4 and b"C_out" in L.vd3d_last_error()
    assert call(buf.data_ptr(), 1, Cin=24) == -4 and b"C_in" in L.vd3d_last_error()
    assert call(buf.data_ptr() + 4, 1) == -4 and b"aligned" in L.vd3d_last_error()       # a misaligned image
    assert call(buf.data_ptr(), 0) == -4 and b"batch" in L.vd3d_last_error()
    assert call(buf.data_ptr(), 65536) == -4 and b"batch" in L.vd3d_last_error()
    assert call(buf.data_ptr(), 1, H=0) == -4
    assert L.vd3d_conv3x3_s2_x3_pack_weights(R._ctx, vp(buf.data_ptr()), 16, 96, vp(img.data_ptr())) == -4 and b"C_out" in L.vd3d_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0   # nothing ran


@pytest.mark.parametrize("B,th,tw", [(1, 28, 42), (2, 126, 238)])
def test_patchify_equals_unfold_bit_for_bit(R, B, th, tw):
    x = torch.randn(B, 3, th, tw, generator=torch.Generator().manual_seed(th)).cuda().contiguous(memory_format=CL)
    rows = R.patchify(x, 14)
    assert tuple(rows.shape) == (B, (th // 14) * (tw // 14), 592) and rows.is_contiguous()
    assert torch.equal(rows[:, :, :588], unfold_rows(x, 14)) and not bool(rows[:, :, 588:].any())
    assert np.array_equal(rows.cpu().numpy(), patchify_reference(x.permute(0, 2, 3, 1).cpu().numpy(), 14))
    with pytest.raises(ValueError):
        R.patchify(x.contiguous(), 14)                    # planar memory is not the layout depth_preprocess hands over
    with pytest.raises(ValueError, match="patch"):
        R.patchify(x[:, :, :10], 14)                      # not one whole patch
    from visiondepth3d_amd import _lib
    vp = ctypes.c_void_p
    assert _lib.lib().vd3d_patchify_f32(R._ctx, vp(x.data_ptr()), B, 10, tw, 14, vp(rows.data_ptr())) == -4 and b"patch" in _lib.lib().vd3d_last_error()
    assert _lib.lib().vd3d_patchify_f32(R._ctx, vp(x.data_ptr()), B, th, tw, 14, vp(rows.data_ptr() + 4)) == -4 and b"aligned" in _lib.lib().vd3d_last_error()


# ---- the depth leg
NAME, SIZE, FH, FW = "depth-anything-v2-small", (126, 238), 252, 476
BANNED = re.compile(r"^aten\.(convolution|_convolution|miopen_|cudnn_|mm\b|addmm|bmm|baddbmm|linear|matmul|_scaled_dot_product_|_flash_attention_forward|_efficient_attention_forward)")


def _frames(n):
    from visiondepth3d_amd import synth
    return torch.from_numpy(np.stack([synth.synth_frame(i, FH, FW)[0] for i in range(n)])).cuda()


def _pipe(R, seed, **kw):
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    return DepthPipe(NAME, device="cuda", dtype=torch.float32, seed=seed, renderer=R, processor=dict(PROCESSORS["da"], size=SIZE), gemm="bf16x3", conv="bf16x3", **kw)


_CACHE = {}


def _leg(R, seed):
    """Per seed, once: the self-contained pipe, its prediction for the two frames, and the stock module's on the same pixel values -- float64 on the CPU (the
    truth), float32 on the CPU (the yardstick), float32 on the GPU.  Shared by the tests below; they do not modify it."""
    if seed not in _CACHE:
        from transformers import DepthAnythingForDepthEstimation
        from visiondepth3d_amd.depth import build_config, synthetic_weights_
        import torch.cuda.tunable as tn
        flags = (torch.backends.cudnn.benchmark, tn.is_enabled())
        pipe = _pipe(R, seed, self_contained=True)
        flags = (flags, (torch.backends.cudnn.benchmark, tn.is_enabled()))
        frames = _frames(2)
        assert pipe.resize_target(FH, FW) == SIZE
        pred = pipe.infer_bgr_u8(frames, raw=True)
        x = R.depth_preprocess(frames, SIZE[0], SIZE[1], pipe.proc["mean"], pipe.proc["std"]).contiguous()   # NCHW copy of what the pipe's network saw
        stock = DepthAnythingForDepthEstimation(build_config(NAME)).eval()
        synthetic_weights_(stock, seed)
        with torch.no_grad():
            p32 = stock(pixel_values=x.cpu()).predicted_depth
            p32g = stock.cuda()(pixel_values=x).predicted_depth
            p64 = stock.cpu().double()(pixel_values=x.cpu().double()).predicted_depth
        _CACHE[seed] = dict(flags=flags, pipe=pipe, frames=frames, pred=pred, p64=p64, p32=p32, p32g=p32g)
    return _CACHE[seed]


def test_self_contained_forward_dispatches_no_vendor_library_operator(R):
    """The second forward (position embedding cached) under a TorchDispatchMode: no convolution, no matrix product, no attention operator of ATen -- every one of
    those would be a MIOpen / hipBLASLt / AOTriton call.  conv_routes names the patch embedding, the four projections, the two transposed convolutions, the
    stride-2 convolution, the four fusion projections and all 20 three-by-three convolutions, none as "library".  The library selection did not run."""
    from torch.utils._python_dispatch import TorchDispatchMode
    leg = _leg(R, 0)
    pipe = leg["pipe"]
    seen = []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with Log():
        pred = pipe.infer_bgr_u8(leg["frames"], raw=True)
    assert len(seen) > 20, seen                       # the mode saw the forward's ATen glue (cat, add, layer norm, views)
    bad = sorted({s for s in seen if BANNED.match(s)})
    assert not bad, bad
    assert torch.equal(pred, leg["pred"])
    routes = pipe.conv_routes
    assert routes and all(v[0] != "library" for v in routes.values()), routes
    mods = dict(pipe.model.named_modules())
    convs = [n for n, m in mods.items() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)) and "layers.0.residual_layer1" not in n and n != "head.conv3"]
    assert sorted(routes) == sorted(convs), sorted(set(routes) ^ set(convs))    # every convolution module that runs (head.conv3 is inside vd3d_dpt_head_tail_f32)
    k3 = [n for n in convs if isinstance(mods[n], torch.nn.Conv2d) and mods[n].kernel_size == (3, 3) and mods[n].stride == (1, 1)]
    assert len(k3) == 20 and all(routes[n] == ("bf16x3", "self-contained") for n in k3)
    for n, what in (("backbone.embeddings.patch_embeddings.projection", "vd3d_patchify_f32"), ("neck.reassemble_stage.layers.0.projection", "vd3d_gemm_x3"),
                    ("neck.reassemble_stage.layers.3.projection", "vd3d_gemm_x3"), ("neck.reassemble_stage.layers.0.resize", "vd3d_depth_to_space_bias_nhwc_f32"),
                    ("neck.reassemble_stage.layers.1.resize", "vd3d_depth_to_space_bias_nhwc_f32"), ("neck.reassemble_stage.layers.3.resize", "vd3d_conv3x3_s2_x3"),
                    ("neck.fusion_stage.layers.0.projection", "vd3d_gemm_x3"), ("neck.fusion_stage.layers.3.projection", "vd3d_gemm_x3")):
        assert routes[n][0] == "bf16x3" and what in routes[n][1], (n, routes[n])
    assert pipe.tuned_gemm is False and pipe.miopen_find is False
    assert leg["flags"][0] == leg["flags"][1]          # (cudnn.benchmark, TunableOp enabled) as the constructor found them: the process-wide switches are not touched


@pytest.mark.parametrize("seed", [0, 1])
def test_self_contained_is_float32_faithful_against_float64(R, seed):
    """E = max |pred - pred64| / range(pred64) <= 2.5 x the stock float32 CPU module's, RMS <= 1.71 x its (the bars of tests/test_hip_depth_f64.py)."""
    leg = _leg(R, seed)
    p64 = leg["p64"]
    rng = float(p64.max() - p64.min())

    def err(p):
        d = p.detach().double().cpu() - p64
        return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng
    (E, rms), (E32, rms32) = err(leg["pred"]), err(leg["p32"])
    print("SELF_CONTAINED_F64", dict(seed=seed, E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32))
    assert tuple(leg["pred"].shape) == tuple(p64.shape) == (2,) + SIZE and bool(torch.isfinite(leg["pred"]).all())
    assert E <= 2.5 * E32, (E, E32)
    assert rms <= 1.71 * rms32, (rms, rms32)


@pytest.mark.parametrize("seed", [0, 1])
def test_self_contained_u8_plane_meets_the_stock_float32_graph(R, seed):
    """depth_to_u8 of the raw prediction against that of the stock float32 graph on the GPU: no byte off by more than 1, >= 99.5 % identical (the bar of
    tests/test_hip_conv_x3.py), the raw prediction within 1e-4 of the range."""
    from visiondepth3d_amd.depth import depth_to_u8
    leg = _leg(R, seed)
    pred, exp = leg["pred"], leg["p32g"]
    d = (depth_to_u8(pred).to(torch.int16) - depth_to_u8(exp).to(torch.int16)).abs()
    st = dict(exact=float((d == 0).float().mean()), max=int(d.max()), pred_err_of_range=float((pred - exp).abs().max()) / float(exp.max() - exp.min()))
    print("SELF_CONTAINED_U8", seed, st)
    assert st["max"] <= 1 and st["exact"] >= 0.995, st
    assert st["pred_err_of_range"] < 1e-4, st


def test_self_contained_repeats_and_does_not_depend_on_the_batch(R):
    """Two forwards are bit-identical; frame 0 alone and frame 0 inside a batch of 3 give equal raw predictions: every kernel's per-element summation order is
    fixed and nothing is split along K."""
    leg = _leg(R, 0)
    pipe = leg["pipe"]
    assert torch.equal(pipe.infer_bgr_u8(leg["frames"], raw=True), leg["pred"])
    f3 = _frames(3)
    one, three = pipe.infer_bgr_u8(f3[:1], raw=True), pipe.infer_bgr_u8(f3, raw=True)
    assert torch.equal(one[0], three[0])
    assert torch.equal(three[:2], leg["pred"])


def test_self_contained_counts_the_library_modes_flops(R):
    leg = _leg(R, 0)
    lib_pipe = _pipe(R, 0)
    assert lib_pipe.self_contained is False
    a, b = leg["pipe"].flops_per_frame(FH, FW), lib_pipe.flops_per_frame(FH, FW)
    assert a == b and a > 0, (a, b)
    assert any(v[0] == "library" for v in lib_pipe.conv_routes.values())      # the library mode at this size is not the self-contained one

