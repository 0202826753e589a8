"""vd3d_dpt_head_conv_f32 (csrc/vd3d_conv_head.hip): conv3x3(up(x) + b_in) [+ the head's tail] in one exact-float32 MFMA kernel, against the three launches it
replaces (vd3d_upsample_bilinear_bias_nhwc_f32, the library convolution, vd3d_dpt_head_tail_f32) and against torch float64.

Shapes: partial tiles on both axes of the 8 x 32 output tile, halo rows on the map's border, a non-integer scale, the identity scale, the x2 scale, batches
across tile counts, every built channel pair.  Bars against float64 are RELATIVE to the library path's own error (max <= 2 x, RMS <= 1.25 x: the bars of
tests/test_hip_attention_f32.py for the same kind of replacement); the one-hot cases are bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
#        B, (ih, iw), (oh, ow), C_in, C_out, tail
CASES = [(2, (5, 7), (9, 13), 64, 32, True),
         (1, (21, 29), (37, 50), 64, 32, True),
         (3, (9, 5), (9, 5), 32, 32, True),        # identity scale: a plain convolution
         (1, (11, 19), (22, 38), 128, 64, False),
         (2, (37, 66), (65, 116), 128, 32, True)]
IDS = ["%dx%dx%d-%dx%d-c%d-%d-%s" % (c[0], *c[1], *c[2], c[3], c[4], "tail" if c[5] else "plain") for c in CASES]


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _inputs(case, seed):
    B, (ih, iw), _, Cin, Cout, tail = case
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, Cin, ih, iw, device="cuda", generator=g).contiguous(memory_format=CL)
    b_in = torch.randn(Cin, device="cuda", generator=g)
    W = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / (3.0 * Cin ** 0.5)
    b2, w3 = torch.randn(Cout, device="cuda", generator=g), torch.randn(Cout, device="cuda", generator=g)
    return x, b_in, W, b2, w3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_hot_weights_are_bit_exact_on_all_nine_taps(R, case):
    """W one-hot in (output channel, tap, input channel), b2 = 0, w3 one-hot, b3 = 0, scale = 1: the output is relu of ONE channel of
    upsample_bilinear_bias(x, size, b_in) shifted by the tap, zero outside the map -- every product is x * 1 or x * 0, every sum exact.  Pins the interpolation
    arithmetic, the padding (0, not bias) and the tile seams bit for bit.  Plain epilogue: the same without the ReLU, every other output channel exactly 0."""
    B, _, (oh, ow), Cin, Cout, tail = case
    x, b_in, _, _, _ = _inputs(case, 11)
    up = R.upsample_bilinear_bias(x, (oh, ow), b_in)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        oc, ci = (5 * tap + 3) % Cout, (7 * tap + Cin // 2 + 1) % Cin    # both lane halves, several accumulator registers, several chunks
        W = torch.zeros(Cout, Cin, 3, 3, device="cuda")
        W[oc, ci, ky, kx] = 1.0
        img = R.dpt_head_conv_pack(W)
        assert img is not None
        exp = F.pad(up[:, ci], (1, 1, 1, 1))[:, ky:ky + oh, kx:kx + ow]
        if tail:
            w3 = torch.zeros(Cout, device="cuda")
            w3[oc] = 1.0
            got = R.dpt_head_conv(x, b_in, (oh, ow), img, torch.zeros(Cout, device="cuda"), w3, 0.0, 1.0)
            assert got.shape == (B, oh, ow) and got.dtype == torch.float32
            assert torch.equal(got, torch.relu(exp)), (tap, float((got - torch.relu(exp)).abs().max()))
        else:
            got = R.dpt_head_conv(x, b_in, (oh, ow), img)
            assert got.shape == (B, Cout, oh, ow) and got.is_contiguous(memory_format=CL)
            assert torch.equal(got[:, oc], exp), (tap, float((got[:, oc] - exp).abs().max()))
            rest = got.clone()
            rest[:, oc] = 0.0
            assert not bool(rest.any()), tap


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_error_against_float64_is_the_library_paths(R, case):
    """Reference: torch float64 interpolate -> conv2d -> tail.  The fused kernel and today's three launches (upsample_bilinear_bias, F.conv2d float32,
    dpt_head_tail) are both measured against it: max error <= 2 x and RMS error <= 1.25 x the library path's.  b3 sits where the last ReLU clips about half
    of the pixels (asserted: 0.2 .. 0.8); only pixels whose float64 pre-ReLU value is within 1e-6 of the range of 0 are left out (asserted: <= 1 %)."""
    B, _, (oh, ow), Cin, Cout, tail = case
    x, b_in, W, b2, w3 = _inputs(case, 23)
    img = R.dpt_head_conv_pack(W)
    up64 = F.interpolate(x.double(), size=(oh, ow), mode="bilinear", align_corners=True) + b_in.double().view(1, -1, 1, 1)
    y64 = F.conv2d(up64, W.double(), None, padding=1)
    y_lib = F.conv2d(R.upsample_bilinear_bias(x, (oh, ow), b_in), W, None, padding=1).contiguous(memory_format=CL)
    if tail:
        pre = (torch.relu(y64 + b2.double().view(1, -1, 1, 1)) * w3.double().view(1, -1, 1, 1)).sum(1)
        b3, scale = -float(pre.mean()), 1.5
        ref = torch.relu(pre + b3) * scale
        lib = R.dpt_head_tail(y_lib, b2, w3, b3, scale)
        got = R.dpt_head_conv(x, b_in, (oh, ow), img, b2, w3, b3, scale)
        clipped = float((got == 0).float().mean())
        keep = (pre + b3).abs() > 1e-6 * float(pre.max() - pre.min())
        left_out = 1.0 - float(keep.float().mean())
        assert float(got.min()) >= 0.0 and 0.2 < clipped < 0.8, clipped
        assert left_out <= 0.01, left_out
    else:
        ref, lib, got = y64, y_lib, R.dpt_head_conv(x, b_in, (oh, ow), img)
        keep = torch.ones_like(ref, dtype=torch.bool)
    e_got, e_lib = (got.double() - ref).abs()[keep], (lib.double() - ref).abs()[keep]
    mx, mx_lib = float(e_got.max()), float(e_lib.max())
    rms, rms_lib = float(e_got.pow(2).mean().sqrt()), float(e_lib.pow(2).mean().sqrt())
    print("DPT_HEAD_F64", IDS[CASES.index(case)], dict(max=mx, max_lib=mx_lib, rms=rms, rms_lib=rms_lib, max_ratio=mx / mx_lib, rms_ratio=rms / rms_lib))
    assert mx <= 2.0 * mx_lib and rms <= 1.25 * rms_lib, (mx, mx_lib, rms, rms_lib)


def test_same_bits_from_run_to_run_beside_a_gemm_on_another_stream(R):
    """No split-K, no atomics: two calls on the largest case give the same bits while a second stream keeps the matrix pipe busy."""
    case = CASES[-1]
    _, _, size, _, _, _ = case
    x, b_in, W, b2, w3 = _inputs(case, 5)
    img = R.dpt_head_conv_pack(W)
    a = torch.randn(2048, 2048, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        with torch.cuda.stream(side):
            for _ in range(4):
                a @ a
        outs.append(R.dpt_head_conv(x, b_in, size, img, b2, w3, 0.25, 2.0))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


def test_packed_image_is_the_restated_layout(R):
    from test_dpt_head_host import BUILT, pack_restated
    for Cin, Cout in BUILT:
        w = torch.randn(Cout, Cin, 3, 3, device="cuda")
        assert torch.equal(R.dpt_head_conv_pack(w).view(torch.float32), pack_restated(w))


def test_refusals_launch_nothing(R):
    """C_in 48, C_out 16, a misaligned pointer and NCHW-contiguous input: VD3D_E_UNSUPPORTED or ValueError, and the output buffer keeps its bytes."""
    from visiondepth3d_amd import _abi
    from visiondepth3d_amd.render_3d import _ptr
    L, ctx = R._L, R._ctx
    assert L.vd3d_dpt_head_conv_weight_bytes(48, 32) < 0 and L.vd3d_dpt_head_conv_weight_bytes(64, 16) < 0 and L.vd3d_dpt_head_conv_weight_bytes(64, 64) < 0
    assert L.vd3d_dpt_head_conv_weight_bytes(64, 32) == 64 * 9 * 32 * 4 and L.vd3d_dpt_head_conv_weight_bytes(128, 64) == 128 * 9 * 64 * 4
    assert R.dpt_head_conv_pack(torch.zeros(32, 48, 3, 3)) is None and R.dpt_head_conv_pack(torch.zeros(16, 64, 3, 3)) is None
    assert R.dpt_head_conv_pack(torch.zeros(32, 64, 1, 1)) is None
    x = torch.randn(1, 6, 7, 64, device="cuda")                    # NHWC storage, room for the misaligned view
    vec = torch.randn(128, device="cuda")
    img = R.dpt_head_conv_pack(torch.randn(32, 64, 3, 3))
    out = torch.full((1, 9, 13), -7.0, device="cuda")
    torch.cuda.synchronize()

    def call(xp, Cin, Cout, tail=True, o=out):
        return L.vd3d_dpt_head_conv_f32(ctx, xp, _ptr(vec), 1, 5, 7, 9, 13, Cin, _ptr(img), Cout, _ptr(vec) if tail else None, _ptr(vec) if tail else None, 0.0, 1.0,
                                        _ptr(o))
    assert call(_ptr(x), 48, 32) == _abi.E_UNSUPPORTED
    assert call(_ptr(x), 64, 16) == _abi.E_UNSUPPORTED
    assert call(_ptr(x), 64, 32, tail=False) == _abi.E_UNSUPPORTED          # the plain epilogue is built for 128 -> 64 only
    assert call(_ptr(x), 128, 64, tail=True) == _abi.E_UNSUPPORTED
    assert call(C.c_void_p(x.data_ptr() + 4), 64, 32) == _abi.E_UNSUPPORTED and b"aligned" in L.vd3d_last_error()
    assert L.vd3d_dpt_head_conv_f32(ctx, _ptr(x), _ptr(vec), 1, 5, 7, 1, 13, 64, _ptr(img), 32, _ptr(vec), _ptr(vec), 0.0, 1.0, _ptr(out)) == _abi.E_UNSUPPORTED
    assert L.vd3d_dpt_head_conv_f32(ctx, _ptr(x), _ptr(vec), 1, 5, 7, 9, 13, 64, _ptr(img), 32, _ptr(vec), None, 0.0, 1.0, _ptr(out)) == _abi.E_INVALID
    nchw = torch.randn(1, 64, 5, 7, device="cuda")
    with pytest.raises(ValueError):
        R.dpt_head_conv(nchw, vec[:64], (9, 13), img, vec[:32], vec[32:64], 0.0, 1.0)
    with pytest.raises(ValueError):                                          # an image of another shape
        R.dpt_head_conv(torch.randn(1, 48, 5, 7, device="cuda").contiguous(memory_format=CL), vec[:48], (9, 13), img, vec[:32], vec[32:64], 0.0, 1.0)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def _small_pipe_frames():
    from visiondepth3d_amd import synth
    return torch.from_numpy(np.stack([synth.synth_frame(i, 270, 480)[0] for i in range(2)])).cuda()


def test_pipe_with_an_unbuilt_head_keeps_the_three_launches(R, monkeypatch):
    """A head whose conv2 has 16 output channels (dpt_head_tail builds it, the fused kernel does not): the three-launch route stays and conv_routes says why."""
    from transformers import DepthAnythingForDepthEstimation
    from visiondepth3d_amd.depth import DepthPipe, build_config, synthetic_weights_
    cfg = build_config("depth-anything-v2-small")
    cfg.head_hidden_size = 16
    model = DepthAnythingForDepthEstimation(cfg).eval()
    synthetic_weights_(model, 0)
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R, model=model)
    calls = [0]
    real = R.dpt_head_conv
    monkeypatch.setattr(R, "dpt_head_conv", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real(*a, **k))[1])
    pred = pipe.infer_bgr_u8(_small_pipe_frames()[:1], raw=True)
    assert bool(torch.isfinite(pred).all()) and calls[0] == 0
    assert pipe.conv_routes["head.conv2"] == ("library", "shape not built: 32 -> 16 channels"), pipe.conv_routes


def test_pipe_prediction_is_the_three_launch_routes(R, monkeypatch):
    """DepthPipe("depth-anything-v2-small"), two 270 x 480 frames: VD3D_HEAD_FUSED=0 and =1 give the same raw prediction to 1e-4 of its range (the bar
    tests/test_hip_depth_e2e.py applies to the neck glue) and the same uint8 hand-off plane on >= 99.5 % of the bytes, never more than one level apart; the
    fused route is really taken, once per forward."""
    from visiondepth3d_amd.depth import DepthPipe
    frames = _small_pipe_frames()
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R)
    calls = [0]
    real = R.dpt_head_conv
    monkeypatch.setattr(R, "dpt_head_conv", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real(*a, **k))[1])
    monkeypatch.setenv("VD3D_HEAD_FUSED", "0")
    p0 = pipe.infer_bgr_u8(frames, raw=True).clone()
    assert calls[0] == 0 and pipe.conv_routes["head.conv2"] == ("library", "VD3D_HEAD_FUSED=0"), pipe.conv_routes
    monkeypatch.setenv("VD3D_HEAD_FUSED", "1")
    p1 = pipe.infer_bgr_u8(frames, raw=True).clone()
    assert calls[0] == 1 and pipe.conv_routes["head.conv2"][0] == "f32-fused", pipe.conv_routes
    assert p0.shape == p1.shape
    rng = float(p0.max() - p0.min())
    err = float((p1 - p0).abs().max()) / rng
    u0, u1 = R.depth_handoff(p0, 270, 480), R.depth_handoff(p1, 270, 480)
    d = (u0.to(torch.int16) - u1.to(torch.int16)).abs()
    exact, mx = float((d == 0).float().mean()), int(d.max())
    print("DPT_HEAD_PIPE", dict(pred_err_of_range=err, u8_exact=exact, u8_max=mx))
    assert err < 1e-4, err
    assert exact >= 0.995 and mx <= 1, (exact, mx)
