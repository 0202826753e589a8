"""vd3d_head_conv_gather_f32 (csrc/vd3d_head_gather.hip): the float32 head's up-sampling + conv2 + tail as coarse MFMA GEMM + in-LDS gather in one launch.

Exact family: bit for bit against the NumPy restatement of the kernel's contract (tests/test_head_gather_host.py head_restated) -- every Z value is an exact float32
in any summation order, so gather and tail must match at any interpolation ratio.  Float64 bars: relative to the library chain's own error (max <= 2 x,
RMS <= 1.25 x: the bars of tests/test_hip_dpt_head_f32.py).  Determinism, refusals, and the pipe's route."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_head_gather_host import F64_CASES, F64_IDS, MAPS, chain64, exact_inputs, f64_inputs, head_restated, pack_restated, tail64

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _compose(R, W, b1):
    from visiondepth3d_amd.depth import head_conv2_compose
    Wt, bc = head_conv2_compose(W, b1)
    return Wt, bc, R.head_conv_gather_pack(Wt, bc)


def _exact_maps(R, Cin):
    """MAPS + a map of exactly one fitted tile + one pixel past it in both directions (coarse 9 / 16 of the fine map + 1: about the workload's ratio)."""
    T = R.head_conv_gather_tile((19, 19), (32, 32), Cin)                                     # the largest tile: 32 x 32, or 16 x 32 (C_in 128)
    assert T is not None and T[0] in (16, 32) and T[1] == 32, T
    hw = (T[0] * 9 // 16 + 1, 19)
    one, past = (hw, T), (hw, (T[0] + 1, T[1] + 1))
    assert R.head_conv_gather_tile(*one, Cin) == T                                           # exactly one tile
    Tp = R.head_conv_gather_tile(*past, Cin)
    assert Tp is not None and Tp[0] <= T[0] and Tp[1] <= T[1]                                # two ragged tiles per axis
    return MAPS + (one, past)


def _run_raw(R, y1s, B, size, packed, b2, w3, b3, scale, outs):
    from visiondepth3d_amd.render_3d import _ptr
    img, bc, Cin = packed
    _, ih, iw, _ = y1s.shape
    R._enter(y1s, img, bc, b2, w3, outs)
    rc = R._L.vd3d_head_conv_gather_f32(R._ctx, _ptr(y1s), B, ih, iw, size[0], size[1], Cin, _ptr(img), _ptr(bc), _ptr(b2), _ptr(w3), float(b3), float(scale), _ptr(outs))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("Cin", (32, 64, 128))
def test_exact_family_is_the_restatement_bit_for_bit(R, Cin):
    """Batch 3, a frame of NaNs behind the last input frame and a sentinel frame behind the output: every index (group, tap, corner, border, tile and frame seam)
    and every rounding of gather and tail is pinned, and nothing is read or written past the batch."""
    zeros = total = 0
    for hw, HW in _exact_maps(R, Cin):
        y1, b1, W, b2, w3 = exact_inputs(3, hw, Cin, 100 * hw[0] + 10 * hw[1] + HW[0] + Cin)
        Wt, bc, packed = _compose(R, W, b1)
        if R.head_conv_gather_tile(hw, HW, Cin) is None:
            pytest.fail("refused: %r -> %r" % (hw, HW))
        y1s = torch.full((4, hw[0], hw[1], Cin), float("nan"), device="cuda")
        y1s[:3] = y1.cuda()
        outs = torch.full((4, HW[0], HW[1]), -7.0, device="cuda")
        b3, scale = -3.25, 1.5
        assert _run_raw(R, y1s, 3, HW, packed, b2.cuda(), w3.cuda(), b3, scale, outs) == 0, R._L.vd3d_last_error()
        want = head_restated(y1.numpy(), Wt.numpy(), bc.numpy(), b2.numpy(), w3.numpy(), b3, scale, HW)
        got = outs[:3].cpu().numpy()
        clipped = float((want == 0).mean())
        print("HEAD_GATHER_EXACT", Cin, hw, HW, dict(clipped=clipped, max_abs=float(np.abs(got - want).max())))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (hw, HW, float(np.abs(got - want).max()), int((got != want).sum()))
        assert bool((outs[3] == -7.0).all())
        zeros, total = zeros + int((want == 0).sum()), total + want.size
        via = R.dpt_head_conv(y1s[:3].permute(0, 3, 1, 2), b1.cuda(), HW, packed, b2.cuda(), w3.cuda(), b3, scale, form="gather")
        assert via.shape == (3, HW[0], HW[1]) and torch.equal(via, outs[:3])
    assert 0.05 < zeros / total < 0.95, zeros / total                                         # over the family both sides of the last ReLU are exercised


@pytest.mark.parametrize("Cin", (32, 64, 128))
def test_one_hot_weights_pin_every_tap(R, Cin):
    """W one-hot in (output channel, tap, input channel), integer y1 and b1, b2 = 0, w3 one-hot, b3 = 0, scale 1: the output is relu of ONE channel of the up-sampled
    (y1 + b1) shifted by the tap, zero outside the map -- against the restatement bit for bit, and against the float64 module chain to float32 rounding."""
    hw, HW = (19, 33), (33, 57)
    y1, b1, _, _, _ = exact_inputs(1, hw, Cin, 7 + Cin)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        oc, ci = (5 * tap + 3) % 32, (7 * tap + Cin // 2 + 1) % Cin
        W = torch.zeros(32, Cin, 3, 3)
        W[oc, ci, ky, kx] = 1.0
        Wt, bc, packed = _compose(R, W, b1)
        w3 = torch.zeros(32)
        w3[oc] = 1.0
        b2 = torch.zeros(32)
        got = R.dpt_head_conv(y1.cuda().permute(0, 3, 1, 2), b1.cuda(), HW, packed, b2.cuda(), w3.cuda(), 0.0, 1.0, form="gather").cpu()
        want = head_restated(y1.numpy(), Wt.numpy(), bc.numpy(), b2.numpy(), w3.numpy(), 0.0, 1.0, HW)
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), tap
        ref = torch.relu(chain64(y1.permute(0, 3, 1, 2), b1, W, HW)[:, oc])
        # |y1 + b1| <= 12.  The float32 coordinate s * y (two roundings, below 33) is within 2 x 2^-24 x 33 of the float64 one per axis and a sample moves by at
        # most 24 per unit of it; the four rounded corner products and the four fmaf roundings add at most 8 x 2^-24 x 12
        assert float((got.double() - ref).abs().max()) <= (2 * 2 * 33 * 24 + 8 * 12) * 2.0 ** -24, tap
        inside = F.pad(torch.ones(1, *HW), (1, 1, 1, 1))[:, ky:ky + HW[0], kx:kx + HW[1]] > 0
        assert bool((got[~inside] == 0).all()) and (tap == 4) == bool(inside.all())              # the zero padding: exactly 0 where the tap is outside the map


@pytest.mark.parametrize("case", F64_CASES, ids=F64_IDS)
def test_error_against_float64_is_the_library_chains(R, case):
    """Reference: the float64 module chain.  The new launch and the library chain (upsample_bilinear_bias, F.conv2d float32, dpt_head_tail) are both measured against
    it: max error <= 2 x and RMS error <= 1.25 x the library chain's; b3 = -mean(pre); clipped share within (0.2, 0.8), at most 1 % of the pixels left out."""
    B, _, size, Cin = case
    x, b_in, W, b2, w3 = (t.cuda() for t in f64_inputs(case))
    x = x.contiguous(memory_format=CL)
    _, _, packed = _compose(R, W, b_in)
    pre, _ = tail64(chain64(x, b_in, W, size), b2, w3, 0.0, 1.0)
    b3, scale = -float(pre.mean()), 1.5
    ref = torch.relu(pre + b3) * scale
    y_lib = F.conv2d(R.upsample_bilinear_bias(x, size, b_in), W, None, padding=1).contiguous(memory_format=CL)
    lib = R.dpt_head_tail(y_lib, b2, w3, b3, scale)
    got = R.dpt_head_conv(x, b_in, size, packed, b2, w3, b3, scale, form="gather")
    assert got.shape == ref.shape and got.dtype == torch.float32
    clipped = float((ref == 0).float().mean())
    keep = (pre + b3).abs() > 1e-6 * float(pre.max() - pre.min())
    left_out = 1.0 - float(keep.float().mean())
    assert float(got.min()) >= 0.0 and 0.2 < clipped < 0.8, clipped
    assert left_out <= 0.01, left_out
    e_got, e_lib = (got.double() - ref).abs()[keep], (lib.double() - ref).abs()[keep]
    mx, mx_lib = float(e_got.max()), float(e_lib.max())
    rms, rms_lib = float(e_got.pow(2).mean().sqrt()), float(e_lib.pow(2).mean().sqrt())
    print("HEAD_GATHER_F64", F64_IDS[F64_CASES.index(case)], dict(max=mx, max_lib=mx_lib, rms=rms, rms_lib=rms_lib, max_ratio=mx / mx_lib, rms_ratio=rms / rms_lib))
    assert mx <= 2.0 * mx_lib and rms <= 1.25 * rms_lib, (mx, mx_lib, rms, rms_lib)


def test_same_bits_from_call_to_call_and_from_batch_to_batch(R):
    """No split-K, no atomics: two calls give the same bits while a second stream keeps the matrix pipe busy, and frame 0 alone equals frame 0 of a batch of 3."""
    case = (3, (37, 41), (65, 71), 64)
    x, b_in, W, b2, w3 = (t.cuda() for t in f64_inputs(case))
    x = x.contiguous(memory_format=CL)
    _, _, packed = _compose(R, W, b_in)
    a = torch.randn(2048, 2048, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        with torch.cuda.stream(side):
            for _ in range(4):
                a @ a
        outs.append(R.dpt_head_conv(x, b_in, case[2], packed, b2, w3, 0.25, 2.0, form="gather"))
    one = R.dpt_head_conv(x[:1].contiguous(memory_format=CL), b_in, case[2], packed, b2, w3, 0.25, 2.0, form="gather")
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(one[0], outs[0][0])


def test_packed_image_is_the_restated_layout(R):
    for Cin in (32, 64, 128):
        Wt, bc = torch.randn(288, Cin), torch.randn(288)
        img, b, c = R.head_conv_gather_pack(Wt, bc)
        assert c == Cin and torch.equal(b.cpu(), bc)
        assert np.array_equal(img.view(torch.float32).cpu().numpy().reshape(9, Cin // 8, 64, 4), pack_restated(Wt.numpy()))


def test_refusals_launch_nothing(R):
    """Unbuilt channel counts, misaligned b2 / w3 / image, oh or ow below 2, a ratio beyond the window: VD3D_E_UNSUPPORTED or ValueError, the output keeps its bytes."""
    from visiondepth3d_amd import _abi
    from visiondepth3d_amd.render_3d import _ptr
    L, ctx = R._L, R._ctx
    assert R.head_conv_gather_pack(torch.zeros(288, 48), torch.zeros(288)) is None and R.head_conv_gather_pack(torch.zeros(288, 16), torch.zeros(288)) is None
    with pytest.raises(ValueError):
        R.head_conv_gather_pack(torch.zeros(144, 64), torch.zeros(144))
    img, bc, _ = R.head_conv_gather_pack(torch.randn(288, 64), torch.randn(288))
    y1 = torch.randn(1, 40, 40, 64, device="cuda")
    vec = torch.randn(128, device="cuda")
    out = torch.full((1, 9, 13), -7.0, device="cuda")
    torch.cuda.synchronize()
    R._enter(y1, img, bc, vec, out)

    def call(ih=5, iw=7, oh=9, ow=13, Cin=64, y=None, im=None, b2=None, w3=None):
        return L.vd3d_head_conv_gather_f32(ctx, y or _ptr(y1), 1, ih, iw, oh, ow, Cin, im or _ptr(img), _ptr(bc), b2 or _ptr(vec), w3 or _ptr(vec[32:]), 0.0, 1.0, _ptr(out))
    for Cin in (48, 16, 256):
        assert call(Cin=Cin) == _abi.E_UNSUPPORTED and b"not built" in L.vd3d_last_error()
    off = lambda t: C.c_void_p(t.data_ptr() + 4)   # noqa: E731
    for kw in (dict(b2=off(vec)), dict(w3=off(vec)), dict(im=off(img)), dict(y=off(y1))):
        assert call(**kw) == _abi.E_UNSUPPORTED and b"aligned" in L.vd3d_last_error(), kw
    assert call(oh=1) == _abi.E_UNSUPPORTED and call(ow=1) == _abi.E_UNSUPPORTED
    assert call(ih=40, iw=40, oh=2, ow=2) == _abi.E_UNSUPPORTED and R.head_conv_gather_tile((40, 40), (2, 2), 64) is None      # a down-sampling factor of 39
    assert L.vd3d_head_conv_gather_f32(ctx, _ptr(y1), 1, 5, 7, 9, 13, 64, _ptr(img), _ptr(bc), None, _ptr(vec), 0.0, 1.0, _ptr(out)) == _abi.E_INVALID
    x = y1[:, :5, :7].permute(0, 3, 1, 2)
    with pytest.raises(ValueError):                                                          # 48 channels against a 64-channel image
        R.dpt_head_conv(torch.randn(1, 48, 5, 7, device="cuda").contiguous(memory_format=CL), vec[:48], (9, 13), (img, bc, 64), vec[:32], vec[32:64], 0.0, 1.0, form="gather")
    with pytest.raises(ValueError):                                                          # the gather form has no plain epilogue
        R.dpt_head_conv(x.contiguous(memory_format=CL), vec[:64], (9, 13), (img, bc, 64), form="gather")
    with pytest.raises(ValueError):
        R.dpt_head_conv(x.contiguous(memory_format=CL), vec[:64], (9, 13), (img, bc, 64), vec[:32], vec[32:64], form="other")
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def _small_pipe_frames():
    from visiondepth3d_amd import synth
    return torch.from_numpy(np.stack([synth.synth_frame(i, 270, 480)[0] for i in range(2)])).cuda()


def test_pipe_prediction_is_the_conv_forms(R, monkeypatch):
    """DepthPipe("depth-anything-v2-small"), two 270 x 480 frames: VD3D_HEAD_CONV2_GATHER=0 and =1 give the same raw prediction to 1e-4 of its range and the same
    uint8 hand-off plane on >= 99.5 % of the bytes, never more than one level apart (the bars of tests/test_hip_dpt_head_f32.py); R.dpt_head_conv is called once per
    forward in both, the route string names the form, and VD3D_HEAD_FUSED=0 still yields the library route."""
    from visiondepth3d_amd.depth import DepthPipe
    frames = _small_pipe_frames()
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R)
    calls, forms = [0], []
    real = R.dpt_head_conv

    def counted(*a, **k):
        calls[0] += 1
        forms.append(k.get("form", "conv"))
        return real(*a, **k)
    monkeypatch.setattr(R, "dpt_head_conv", counted)
    monkeypatch.setenv("VD3D_HEAD_CONV2_GATHER", "0")
    p0 = pipe.infer_bgr_u8(frames, raw=True).clone()
    r0 = pipe.conv_routes["head.conv2"]
    assert calls[0] == 1 and forms == ["conv"] and r0[0] == "f32-fused" and "form conv" in r0[1] and "gather" not in r0[1], r0
    monkeypatch.setenv("VD3D_HEAD_CONV2_GATHER", "1")
    p1 = pipe.infer_bgr_u8(frames, raw=True).clone()
    r1 = pipe.conv_routes["head.conv2"]
    assert calls[0] == 2 and forms == ["conv", "gather"] and r1[0] == "f32-fused" and "form gather" in r1[1], r1
    monkeypatch.setenv("VD3D_HEAD_FUSED", "0")
    p2 = pipe.infer_bgr_u8(frames, raw=True).clone()
    assert calls[0] == 2 and pipe.conv_routes["head.conv2"] == ("library", "VD3D_HEAD_FUSED=0"), pipe.conv_routes
    assert p0.shape == p1.shape == p2.shape
    rng = float(p0.max() - p0.min())
    err = float((p1 - p0).abs().max()) / rng
    u0, u1 = R.depth_handoff(p0, 270, 480), R.depth_handoff(p1, 270, 480)
    d = (u0.to(torch.int16) - u1.to(torch.int16)).abs()
    exact, mx = float((d == 0).float().mean()), int(d.max())
    print("HEAD_GATHER_PIPE", dict(pred_err_of_range=err, u8_exact=exact, u8_max=mx))
    assert err < 1e-4, err
    assert exact >= 0.995 and mx <= 1, (exact, mx)
