"""The float32 head's first convolution as coarse GEMM + fine gather (depth.py head_upconv_compose, csrc/vd3d_head_upconv.hip vd3d_head_upconv_gather_f32): the
gather bit for bit against its NumPy restatement (tests/test_head_upconv_host.py gather_restated: exact fused multiply-adds in the stated order), the whole route
against the float64 module chain beside the library chain it replaces, the refusals, the switch and the pipe.

The kernel's fine tile is 16 x 32 (HU_TH x HU_TW; below a factor of about 2 the host shrinks it so that a tile's reach fits the staged window): 8 x 16 -> 16 x 32 is
exactly one tile, 9 x 17 -> 17 x 33 one pixel past it in each direction (four tiles, three of them one pixel wide or high)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_head_upconv_host import MAPS, TILE, chain64, gather_restated

pytestmark = pytest.mark.gpu

CL = torch.channels_last
GATHER_MAPS = MAPS + (((8, 16), TILE), ((9, 17), (TILE[0] + 1, TILE[1] + 1)))
GATHER_IDS = ["%dx%d-%dx%d" % (a + b) for a, b in GATHER_MAPS]


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("Co", (64, 32))
@pytest.mark.parametrize("hw,HW", GATHER_MAPS, ids=GATHER_IDS)
def test_gather_is_the_restatement_bit_for_bit(R, hw, HW, Co):
    """Batch 3, a frame of NaNs behind the last input frame and a sentinel frame behind the output: every index (tap, corner, border, channel chunk, tile seam, frame
    seam) and every rounding is pinned, and nothing is read or written past the batch."""
    from visiondepth3d_amd.render_3d import _ptr
    (h, w), (H, W) = hw, HW
    g = torch.Generator(device="cuda").manual_seed(100 * h + 10 * w + H + Co)
    zs = torch.full((4, h, w, 9, Co), float("nan"), device="cuda")
    zs[:3] = torch.randn(3, h, w, 9, Co, device="cuda", generator=g)
    outs = torch.full((4, H, W, Co), -7.0, device="cuda")
    torch.cuda.synchronize()
    R._enter(zs, outs)
    assert R._L.vd3d_head_upconv_gather_f32(R._ctx, _ptr(zs), 3, h, w, H, W, Co, _ptr(outs)) == 0, R._L.vd3d_last_error()
    torch.cuda.synchronize()
    want = gather_restated(zs[:3].cpu().numpy(), H, W)
    got = outs[:3].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    assert bool((outs[3] == -7.0).all())
    via = R.head_upconv_gather(zs[:3], (H, W), Co)
    assert via.shape == (3, Co, H, W) and via.is_contiguous(memory_format=CL) and torch.equal(via.permute(0, 2, 3, 1), outs[:3])


@pytest.mark.parametrize("Co", (64, 32))
def test_gather_repeats_its_bits_from_call_to_call_and_from_batch_to_batch(R, Co):
    """Every value is summed by one lane in one fixed order: two calls give equal bits, and frame 0 alone equals frame 0 of a batch of 3 (37 x 45: several tiles with
    ragged edges, so the batch puts the frame's tiles into other workgroups)."""
    g = torch.Generator(device="cuda").manual_seed(Co)
    z = torch.randn(3, 19, 23, 9 * Co, device="cuda", generator=g)
    a, b = R.head_upconv_gather(z, (37, 45), Co), R.head_upconv_gather(z, (37, 45), Co)
    one = R.head_upconv_gather(z[:1].contiguous(), (37, 45), Co)
    two = R.head_upconv_gather(z[1:].contiguous(), (37, 45), Co)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(one[0], a[0]) and torch.equal(two, a[1:])


def _route(R, x, pw, pb, cw, size):
    """The route as DepthPipe runs it: the composed matrix, the library GEMM over the channels_last storage's rows, the gather."""
    from visiondepth3d_amd.depth import head_upconv_compose
    Wc, bc = head_upconv_compose(pw, pb, cw)
    B, Cc, h, w = x.shape
    z = F.linear(x.contiguous(memory_format=CL).permute(0, 2, 3, 1).reshape(B * h * w, Cc), Wc, bc)
    return R.head_upconv_gather(z.view(B, h, w, -1), size, cw.shape[0])


@pytest.mark.parametrize("cc,hw,HW", (((128, 64), (19, 33), (38, 66)), ((64, 32), (19, 33), (38, 66)), ((128, 64), (5, 7), (9, 13)), ((64, 32), (5, 7), (9, 13))),
                         ids=("128-64-38x66", "64-32-38x66", "128-64-9x13", "64-32-9x13"))
def test_route_error_against_float64_is_the_library_chains(R, cc, hw, HW):
    """Reference: the module chain in torch float64 (projection with bias, bilinear align_corners=True, conv1 with zero padding).  The route and the library chain in
    float32 on the GPU are both measured against it: max error <= 2 x and RMS error <= 1.25 x the library chain's (the bars of tests/test_hip_dpt_head_f32.py and
    tests/test_hip_neck_poly.py; on the CPU the ratios were at most 1.01 and 0.99)."""
    C_, Co = cc
    g = torch.Generator(device="cuda").manual_seed(C_ + hw[0])
    x = torch.randn(2, C_, *hw, device="cuda", generator=g).contiguous(memory_format=CL)
    pw = torch.randn(C_, C_, 1, 1, device="cuda", generator=g) / C_ ** 0.5
    pb = torch.randn(C_, device="cuda", generator=g)
    cw = torch.randn(Co, C_, 3, 3, device="cuda", generator=g) / (3.0 * C_ ** 0.5)
    ref = chain64(x, pw, pb, cw, HW)
    lib = F.conv2d(F.interpolate(F.conv2d(x, pw, pb), size=HW, mode="bilinear", align_corners=True), cw, None, padding=1)
    got = _route(R, x, pw, pb, cw, HW)
    assert got.shape == ref.shape
    e_got, e_lib = (got.double() - ref).abs(), (lib.double() - ref).abs()
    mx, mx_lib = float(e_got.max()), float(e_lib.max())
    rms, rms_lib = float(e_got.pow(2).mean().sqrt()), float(e_lib.pow(2).mean().sqrt())
    print("HEAD_UPCONV_F64", cc, HW, dict(max=mx, max_lib=mx_lib, rms=rms, rms_lib=rms_lib, max_ratio=mx / mx_lib, rms_ratio=rms / rms_lib))
    assert mx <= 2.0 * mx_lib and rms <= 1.25 * rms_lib, (mx, mx_lib, rms, rms_lib)


def test_refusals_launch_nothing(R):
    """Channels that are not built, an output below 2 x 2, a misaligned pointer, a tensor of another layout: VD3D_E_UNSUPPORTED or ValueError, and the output buffer
    keeps its bytes."""
    from visiondepth3d_amd import _abi, _lib
    from visiondepth3d_amd.render_3d import _ptr
    L, ctx = R._L, R._ctx
    z = torch.randn(1, 6, 7, 9 * 64, device="cuda")
    out = torch.full((1, 10, 14, 64), -7.0, device="cuda")
    torch.cuda.synchronize()
    f = L.vd3d_head_upconv_gather_f32
    assert f(ctx, _ptr(z), 1, 5, 7, 10, 14, 48, _ptr(out)) == _abi.E_UNSUPPORTED and b"not built" in L.vd3d_last_error()
    assert f(ctx, _ptr(z), 1, 5, 7, 10, 14, 128, _ptr(out)) == _abi.E_UNSUPPORTED
    assert f(ctx, _ptr(z), 1, 5, 7, 1, 14, 64, _ptr(out)) == _abi.E_UNSUPPORTED
    assert f(ctx, _ptr(z), 1, 5, 7, 10, 1, 64, _ptr(out)) == _abi.E_UNSUPPORTED
    assert f(ctx, _ptr(z), 0, 5, 7, 10, 14, 64, _ptr(out)) == _abi.E_UNSUPPORTED
    assert f(ctx, C.c_void_p(z.data_ptr() + 4), 1, 5, 7, 10, 14, 64, _ptr(out)) == _abi.E_UNSUPPORTED and b"aligned" in L.vd3d_last_error()
    assert f(ctx, _ptr(z), 1, 5, 7, 10, 14, 64, C.c_void_p(out.data_ptr() + 4)) == _abi.E_UNSUPPORTED
    assert f(ctx, None, 1, 5, 7, 10, 14, 64, _ptr(out)) == _abi.E_INVALID
    with pytest.raises(_lib.Vd3dError):
        R.head_upconv_gather(torch.randn(1, 5, 7, 9 * 48, device="cuda"), (10, 14), 48)        # 48 output channels are not built
    with pytest.raises(ValueError):
        R.head_upconv_gather(z[:, :5], (10, 14), 32)                                          # 9 x 64 channels are not 9 x 32
    with pytest.raises(ValueError):
        R.head_upconv_gather(z[:, :5, :, ::2], (10, 14), 32)                                  # channels with gaps
    with pytest.raises(ValueError):
        R.head_upconv_gather(z[:, :5].double(), (10, 14), 64)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_pipe_prediction_is_the_library_routes(R, monkeypatch):
    """DepthPipe("depth-anything-v2-small"), two 270 x 480 frames: VD3D_HEAD_UPCONV=0 and =1 give the same raw prediction to 1e-4 of its range and the same uint8
    hand-off plane on >= 99.5 % of the bytes, never more than one level apart (the bars of tests/test_hip_dpt_head_f32.py and tests/test_hip_neck_poly.py); both
    routes are named in conv_routes, the gather runs once per forward with the switch on and never with it off, the neck called on its own still returns the
    up-sampled projection, and the counted FLOPs are the module graph's either way."""
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import DepthPipe
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, 270, 480)[0] for i in range(2)])).cuda()
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R)
    calls = [0]
    real = R.head_upconv_gather
    monkeypatch.setattr(R, "head_upconv_gather", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real(*a, **k))[1])
    n_last = len(pipe.model.neck.fusion_stage.layers) - 1
    names = [f"neck.fusion_stage.layers.{n_last}.projection", "head.conv1"]
    monkeypatch.setenv("VD3D_HEAD_UPCONV", "0")
    p0 = pipe.infer_bgr_u8(frames, raw=True).clone()
    assert calls[0] == 0 and all(pipe.conv_routes[n] == ("library", "VD3D_HEAD_UPCONV=0") for n in names), pipe.conv_routes
    monkeypatch.setenv("VD3D_HEAD_UPCONV", "1")
    p1 = pipe.infer_bgr_u8(frames, raw=True).clone()
    assert calls[0] == 1 and all(pipe.conv_routes[n][0] == "f32-upconv" for n in names), pipe.conv_routes
    assert "64 -> 9 x 32 channels" in pipe.conv_routes[names[0]][1] and pipe.conv_routes["head.conv2"][0] == "f32-fused"
    pipe.infer_bgr_u8(frames, raw=True)
    assert calls[0] == 2                                   # once per forward, from the matrix cached per parameter version
    monkeypatch.setenv("VD3D_HEAD_FUSED", "0")             # the three-launch head takes the gather's output and conv1's bias through the up-sampling kernel
    p2 = pipe.infer_bgr_u8(frames, raw=True).clone()
    monkeypatch.setenv("VD3D_HEAD_FUSED", "1")
    assert calls[0] == 3 and pipe.conv_routes["head.conv2"][0] == "library"
    assert p0.shape == p1.shape == p2.shape
    rng = float(p0.max() - p0.min())
    err, err2 = float((p1 - p0).abs().max()) / rng, float((p2 - p0).abs().max()) / rng
    u0, u1 = R.depth_handoff(p0, 270, 480), R.depth_handoff(p1, 270, 480)
    d = (u0.to(torch.int16) - u1.to(torch.int16)).abs()
    exact, mx = float((d == 0).float().mean()), int(d.max())
    print("HEAD_UPCONV_PIPE", dict(pred_err_of_range=err, pred_err_of_range_unfused_head=err2, u8_exact=exact, u8_max=mx))
    assert err < 1e-4 and err2 < 1e-4, (err, err2)
    assert exact >= 0.995 and mx <= 1, (exact, mx)
    # the neck on its own (no head behind it): the last fusion layer materialises the up-sampled projection as ever
    with torch.no_grad():
        hs = [torch.randn(1, 1 + 5 * 7, pipe.model.neck.reassemble_stage.layers[0].projection.in_channels, device="cuda") for _ in range(4)]
        outs = pipe.model.neck(hs, 5, 7)
    assert calls[0] == 3 and outs[-1].shape[1] == pipe.model.head.conv1.in_channels
    assert tuple(outs[-1].shape[2:]) == (2 * outs[-2].shape[2], 2 * outs[-2].shape[3])
    fl1 = pipe.flops_per_frame(270, 480)                   # the record's FLOP count stays the module graph's
    monkeypatch.setenv("VD3D_HEAD_UPCONV", "0")
    assert pipe.flops_per_frame(270, 480) == fl1
