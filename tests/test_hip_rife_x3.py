"""GPU tests (-m gpu) of the interpolation network on this library's kernels: the bf16x3 convolution family vd3d_conv_ifn (csrc/vd3d_conv_x3.hip: 3 x 3 stride 1,
3 x 3 stride 2, transposed 4 x 4 stride 2; bias / PReLU / residual epilogue), the three glue kernels, and RifeSession(conv="bf16x3") end to end.

Floating-point kernels: every bar is stated against FLOAT64, beside PyTorch's float32 CPU op on the same operands -- the yardstick and the bars of
tests/test_hip_conv_x3.py test_conv3x3_x3_is_float32_faithful (maximum <= max(2.5 x the yardstick's, 2^-21), RMS <= 1.5 x the yardstick's + 1e-9).  Then exact
small-integer cases that pin the geometry, NaN / Inf, the refusals, and the session against float64 / float32 CPU runs of the module."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
K3S1, K3S2, T4S2 = 0, 1, 2
KNAME = {K3S1: "k3s1", K3S2: "k3s2", T4S2: "t4s2"}


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _osize(kind, H, W):
    return {K3S1: (H, W), K3S2: ((H + 1) // 2, (W + 1) // 2), T4S2: (2 * H, 2 * W)}[kind]


def _op(kind, x, w, b):
    if kind == T4S2:
        return F.conv_transpose2d(x, w, b, 2, 1)
    return F.conv2d(x, w, b, 2 if kind == K3S2 else 1, 1)


def _ref(kind, x, w, b, slope, res, dtype, device):
    y = _op(kind, x.to(device, dtype), w.to(device, dtype), b.to(device, dtype))
    if slope is not None:
        y = torch.where(y >= 0, y, slope.to(device, dtype).view(1, -1, 1, 1) * y)
    return y if res is None else y + res.to(device, dtype)


def _nhwc(t, pitch=None, offset=0, fill=0.0):
    """A channels_last [B, pitch, H, W] tensor that holds t in channels [offset, offset + C) and `fill` elsewhere."""
    B, Cc, H, W = t.shape
    buf = torch.full((B, H, W, pitch or Cc), fill, dtype=torch.float32, device="cuda")
    buf[..., offset:offset + Cc] = t.permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)


def _run(R, kind, x, w, b, slope, res=None, x_stride=None, y_stride=None, y_offset=0):
    """x NCHW on the GPU; the channels of the input buffer behind C_in hold 1e30 (read = seen), the output buffer holds a sentinel outside the written slice."""
    B, Cin, H, W = x.shape
    Cout = w.shape[1] if kind == T4S2 else w.shape[0]
    Ho, Wo = _osize(kind, H, W)
    img = R.conv_ifn_pack(kind, w)
    assert img is not None
    xb = _nhwc(x, x_stride, 0, 1e30)
    out = _nhwc(torch.zeros(B, 0, Ho, Wo, device="cuda"), y_stride or Cout, 0, -7.5)
    rb = None if res is None else _nhwc(res)
    R.conv_ifn(kind, xb, Cin, img, b, slope, Cout, out, y_offset, rb)
    y = out[:, y_offset:y_offset + Cout]
    rest = torch.cat((out[:, :y_offset], out[:, y_offset + Cout:]), 1)
    assert bool((rest == -7.5).all())                      # nothing outside the slice is written
    again = _nhwc(torch.zeros(B, 0, Ho, Wo, device="cuda"), y_stride or Cout, 0, -7.5)
    R.conv_ifn(kind, xb, Cin, img, b, slope, Cout, again, y_offset, rb)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))      # two calls return identical bits (NaNs included)
    return y


# (kind, B, H, W, Cin, Cout, x_stride, y_stride, y_offset)
FAITHFUL = [(K3S1, 1, 1, 1, 16, 32, None, None, 0), (K3S1, 2, 9, 33, 96, 96, None, None, 0), (K3S1, 1, 17, 31, 48, 64, None, None, 0),
            (K3S1, 1, 8, 32, 96, 96, 128, 160, 32),
            (K3S2, 1, 1, 1, 16, 32, None, None, 0), (K3S2, 1, 2, 2, 16, 64, None, None, 0), (K3S2, 1, 7, 65, 16, 64, None, None, 0), (K3S2, 2, 16, 34, 48, 96, None, None, 0),
            (T4S2, 1, 1, 1, 96, 32, None, None, 0), (T4S2, 2, 5, 35, 96, 96, None, None, 0), (T4S2, 1, 9, 33, 48, 32, None, None, 0)]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("kind,B,H,W,Cin,Cout,xs,ys,yo", FAITHFUL)
def test_conv_ifn_is_float32_faithful(R, kind, B, H, W, Cin, Cout, xs, ys, yo, with_res, record_property):
    """vd3d_conv_ifn against the float64 torch op, beside PyTorch's float32 CPU op on the same operands: maximum of |y - y64| / (op(|x|, |w|) + |bias|) <=
    max(2.5 x the yardstick's, 2^-21), relative RMS <= 1.5 x the yardstick's + 1e-9.  Post-ReLU inputs with log-normal channel scales, random bias, per-channel
    slopes from {1, 0.25, -0.5, 0}, with and without a residual; one-pixel maps, ragged tiles, odd stride-2 sizes, a strided input and an output slice.
    Measured (profiles/r11_rife_x3.md): maximum 0.44 - 2.03 x the yardstick's (the 2.03 x case: 1.07e-7, below the 2^-21 floor), RMS 0.53 - 1.17 x."""
    g = torch.Generator(device="cuda").manual_seed(kind * 1000 + B * 100 + H)
    x = torch.relu(torch.randn(B, Cin, H, W, device="cuda", generator=g)) * torch.exp(torch.randn(1, Cin, 1, 1, device="cuda", generator=g))
    w = torch.randn((Cin, Cout, 4, 4) if kind == T4S2 else (Cout, Cin, 3, 3), device="cuda", generator=g) * 0.05
    b = torch.randn(Cout, device="cuda", generator=g) * 0.5
    slope = torch.tensor([1.0, 0.25, -0.5, 0.0], device="cuda")[torch.randint(0, 4, (Cout,), device="cuda", generator=g)]
    Ho, Wo = _osize(kind, H, W)
    res = torch.randn(B, Cout, Ho, Wo, device="cuda", generator=g) if with_res else None
    y = _run(R, kind, x, w, b, slope, res, xs, ys, yo)
    assert y.shape == (B, Cout, Ho, Wo) and bool(torch.isfinite(y).all())
    ref = _ref(kind, x, w, b, slope, res, torch.float64, "cuda")
    y32 = _ref(kind, x, w, b, slope, res, torch.float32, "cpu").cuda()
    scale = _op(kind, x.abs().double(), w.abs().double(), None) + b.abs().double().view(1, -1, 1, 1) + 1e-30
    e3, e32 = float(((y.double() - ref).abs() / scale).max()), float(((y32.double() - ref).abs() / scale).max())
    den = ref.pow(2).mean().sqrt()
    r3, r32 = float((y.double() - ref).pow(2).mean().sqrt() / den), float((y32.double() - ref).pow(2).mean().sqrt() / den)
    print(f"CONV_IFN_ERR {KNAME[kind]} {B}x{H}x{W}x{Cin}->{Cout} res {int(with_res)} max {e3:.3e} (f32 {e32:.3e}, {e3 / max(e32, 1e-30):.2f}x) "
          f"rms {r3:.3e} (f32 {r32:.3e}, {r3 / max(r32, 1e-30):.2f}x)")
    record_property("conv_ifn_err", dict(e3=e3, e32=e32, r3=r3, r32=r32))
    assert e3 <= max(2.5 * e32, 2.0 ** -21), (e3, e32)
    assert r3 <= 1.5 * r32 + 1e-9, (r3, r32)


@pytest.mark.parametrize("Cout", [32, 64, 96])
@pytest.mark.parametrize("kind,H,W", [(K3S1, 21, 45), (K3S2, 21, 69), (K3S2, 18, 66), (T4S2, 11, 37)])
def test_conv_ifn_exact_small_integers_pin_the_geometry(R, kind, H, W, Cout):
    """Integer inputs and weights with one bf16 term each, integer bias and residual, slopes in {0.5, 2, 1}: every product and partial sum is exact (everything
    below 2^24), so the result equals the float64 op bit for bit -- a swapped phase, a mirrored tap, a wrong stride origin or a shifted channel slice shows.
    Two frames, ragged tiles in both directions (more than one tile each way), three input chunks; stride 2 on an odd and on an even size."""
    B, Cin = 2, 48
    xi = ((torch.arange(B * Cin * H * W, device="cuda").view(B, Cin, H, W) * 7) % 5 - 2).float()
    wshape = (Cin, Cout, 4, 4) if kind == T4S2 else (Cout, Cin, 3, 3)
    wi = ((torch.arange(int(np.prod(wshape)), device="cuda").view(wshape) * 11) % 7 - 3).float()
    bi = ((torch.arange(Cout, device="cuda") * 5) % 9 - 4).float()
    slope = torch.tensor([0.5, 2.0, 1.0], device="cuda")[torch.arange(Cout, device="cuda") % 3]
    Ho, Wo = _osize(kind, H, W)
    ri = ((torch.arange(B * Cout * Ho * Wo, device="cuda").view(B, Cout, Ho, Wo) * 3) % 11 - 5).float()
    assert float(_op(kind, xi.abs().double(), wi.abs().double(), None).max()) * 2 + 16 < 2 ** 24
    for res in (None, ri):
        y = _run(R, kind, xi, wi, bi, slope, res, 64, Cout + 32, 32)          # a strided input and an output slice as well
        assert torch.equal(y.double(), _ref(kind, xi, wi, bi, slope, res, torch.float64, "cuda"))


@pytest.mark.parametrize("kind", [K3S2, T4S2])
def test_conv_ifn_nan_and_inf_reach_exactly_the_outputs_whose_window_holds_them(R, kind):
    x = torch.ones(1, 16, 9, 33, device="cuda")
    x[0, 3, 4, 5] = float("inf")
    x[0, 7, 8, 32] = float("nan")
    x[0, 0, 0, 0] = float("-inf")
    w = torch.ones((16, 32, 4, 4) if kind == T4S2 else (32, 16, 3, 3), device="cuda")
    y = _run(R, kind, x, w, torch.zeros(32, device="cuda"), None)
    bad = (~torch.isfinite(x)).any(1, keepdim=True).double()
    want = _op(kind, bad, torch.ones((1, 1, 4, 4) if kind == T4S2 else (1, 1, 3, 3), device="cuda", dtype=torch.float64), None) > 0
    assert 0 < int(want.sum()) < want.numel()
    assert torch.equal(~torch.isfinite(y), want.expand_as(y))
    # Inf alone in a window of positive weights would stay Inf in a float32 convolution; through the split it is NaN (include/vd3d.h), like vd3d_conv3x3_x3
    assert bool(torch.isnan(y[want.expand_as(y)]).all())


def test_conv_ifn_refuses_what_it_does_not_build(R):
    from visiondepth3d_amd import _lib
    assert R.conv_ifn_pack(K3S1, torch.zeros(128, 16, 3, 3, device="cuda")) is None     # C_out 128 (32 / 64 / 96 are built)
    assert R.conv_ifn_pack(K3S2, torch.zeros(64, 20, 3, 3, device="cuda")) is None      # C_in not a multiple of 16
    assert R.conv_ifn_pack(T4S2, torch.zeros(16, 32, 3, 3, device="cuda")) is None      # the transposed kind is 4 x 4
    L = _lib.lib()
    vp = ctypes.c_void_p
    img = R.conv_ifn_pack(K3S1, torch.zeros(32, 16, 3, 3, device="cuda"))
    buf = torch.full((4 * 4 * 64 + 4,), 3.0, device="cuda")
    out = torch.full((4 * 4 * 64,), -7.5, device="cuda")
    bias = torch.zeros(32, device="cuda")

    def call(kind=K3S1, x=buf.data_ptr(), B=1, xs=16, cin=16, cout=32, y=out.data_ptr(), ys=32, yo=0, r=None, rs=0):
        return L.vd3d_conv_ifn(R._ctx, kind, vp(x), B, 4, 4, xs, cin, vp(img.data_ptr()), vp(bias.data_ptr()), None, cout, vp(r) if r else None, rs, vp(y), ys, yo)
    assert call(cout=48) == -4 and b"C_out" in L.vd3d_last_error()                      # unbuilt C_out
    assert call(cin=24, xs=24) == -4 and b"C_in" in L.vd3d_last_error()                 # C_in not a multiple of 16
    assert call(kind=3) == -4 and b"kind" in L.vd3d_last_error()
    assert call(x=buf.data_ptr() + 4) == -4 and b"aligned" in L.vd3d_last_error()       # misaligned pointer
    assert call(xs=12) == -4 and b"x_stride" in L.vd3d_last_error()                     # pitch smaller than the channel count
    assert call(ys=48, yo=32) == -4 and b"y_stride" in L.vd3d_last_error()
    assert call(r=buf.data_ptr(), rs=16) == -4 and b"r_stride" in L.vd3d_last_error()
    assert call(B=0) == -4 and b"batch" in L.vd3d_last_error()
    assert call(B=65536) == -4 and b"batch" in L.vd3d_last_error()
    # an output slice over the input channels of the same buffer: [8, 40) meets [0, 16) of a 64-pitch buffer
    assert call(x=out.data_ptr(), xs=64, y=out.data_ptr(), ys=64, yo=8) == -4 and b"meets the input channels" in L.vd3d_last_error()
    assert call(r=out.data_ptr(), rs=32) == -4 and b"residual" in L.vd3d_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.5).all()) and bool((buf == 3.0).all())                       # nothing ran: the buffers keep their bits
    assert call(x=out.data_ptr(), xs=64, y=out.data_ptr(), ys=64, yo=16) == 0           # the slice behind the input channels is the dense-buffer case
    torch.cuda.synchronize()


# ---- glue kernels: 32 x 64 frames, batch 2, flows up to +-40 px so that a share of the samples clamps at every border
def _glue_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x6 = torch.rand(2, 6, 32, 64, generator=g)
    flow = (torch.rand(2, 4, 32, 64, generator=g) * 2 - 1) * 40.0
    mask = torch.rand(2, 1, 32, 64, generator=g)
    return x6, flow, mask


def _state(flow, mask):
    s = torch.zeros(flow.shape[0], flow.shape[2], flow.shape[3], 8, device="cuda")
    s[..., :4] = flow.permute(0, 2, 3, 1)
    s[..., 4] = mask[:, 0]
    return s


def _bars(tag, got, ref, yard, record_property):
    e, e32 = float((got.double() - ref).abs().max()), float((yard.double() - ref).abs().max())
    r, r32 = float((got.double() - ref).pow(2).mean().sqrt()), float((yard.double() - ref).pow(2).mean().sqrt())
    print(f"RIFE_GLUE_ERR {tag} max {e:.3e} (f32 {e32:.3e}) rms {r:.3e} (f32 {r32:.3e})")
    record_property(tag, dict(e=e, e32=e32, r=r, r32=r32))
    assert e <= max(2.5 * e32, 2.0 ** -21), (tag, e, e32)
    assert r <= 1.5 * r32 + 1e-9, (tag, r, r32)


def _warp_pack_torch(x6, flow, mask, s, dtype):
    from visiondepth3d_amd.rife import backwarp
    x6, flow, mask = x6.to(dtype), flow.to(dtype), mask.to(dtype)
    cat = torch.cat((backwarp(x6[:, :3], flow[:, :2]), backwarp(x6[:, 3:], flow[:, 2:4]), mask), 1)
    kw = dict(scale_factor=1.0 / s, mode="bilinear", align_corners=False, recompute_scale_factor=False)
    return torch.cat((F.interpolate(cat, **kw), F.interpolate(flow, **kw) * (1.0 / s)), 1)


@pytest.mark.parametrize("s", [1, 2, 4])
def test_rife_warp_pack_vs_grid_sample_interpolate_cat(R, s, record_property):
    """vd3d_rife_warp_pack against grid_sample(border, align_corners=True) + F.interpolate(1 / s) + cat in float64, beside the same ops in float32 on the CPU.  The
    seven image channels are values in [0, 1]; the four flow channels (up to 40 / s) are compared divided by 40, i.e. on the same scale.  Channels 11 .. 15 are zero."""
    x6, flow, mask = _glue_inputs(s)
    out = torch.full((2, 32 // s, 64 // s, 16), -7.5, device="cuda")
    R.rife_warp_pack(x6.cuda(), _state(flow.cuda(), mask.cuda()), s, out)
    got = out.permute(0, 3, 1, 2).cpu()
    assert bool((got[:, 11:] == 0).all())
    ref, yard = _warp_pack_torch(x6, flow, mask, s, torch.float64), _warp_pack_torch(x6, flow, mask, s, torch.float32)
    sc = torch.cat((torch.ones(7), torch.full((4,), 1.0 / 40.0))).view(1, 11, 1, 1)
    _bars(f"warp_pack_s{s}", got[:, :11] * sc, ref * sc.double(), yard * sc, record_property)
    # the first block: no state, the warp is the identity
    R.rife_warp_pack(x6.cuda(), None, s, out)
    z4, z1 = torch.zeros_like(flow), torch.zeros_like(mask)
    _bars(f"warp_pack_first_s{s}", out.permute(0, 3, 1, 2).cpu()[:, :11], _warp_pack_torch(x6, z4, z1, s, torch.float64), _warp_pack_torch(x6, z4, z1, s, torch.float32),
          record_property)


@pytest.mark.parametrize("s", [1, 2, 4])
def test_rife_update_vs_interpolate_add(R, s, record_property):
    """flow += up(t[:4]) * s, mask += up(t[4]) against F.interpolate(scale_factor=s, bilinear, align_corners=False) in float64, beside float32 on the CPU; values in [0, 1]."""
    g = torch.Generator().manual_seed(10 + s)
    t = torch.rand(2, 32 // s, 64 // s, 32, generator=g)
    st = torch.rand(2, 5, 32, 64, generator=g)

    def want(dtype, first):
        tt = t.permute(0, 3, 1, 2)[:, :5].to(dtype)
        up = tt if s == 1 else F.interpolate(tt, scale_factor=float(s), mode="bilinear", align_corners=False, recompute_scale_factor=False)
        up = torch.cat((up[:, :4] * float(s), up[:, 4:]), 1)
        return up if first else st.to(dtype) + up
    for first in (False, True):
        state = _state(st[:, :4].cuda(), st[:, 4:].cuda())
        state[..., 5:] = 9.0
        R.rife_update(t.cuda(), state, s, first, 32, 64)
        got = state.permute(0, 3, 1, 2).cpu()
        assert bool((got[:, 5:] == 0).all())
        _bars(f"update_s{s}_first{int(first)}", got[:, :5], want(torch.float64, first), want(torch.float32, first), record_property)


def test_rife_blend_vs_grid_sample_sigmoid(R, record_property):
    from visiondepth3d_amd.rife import backwarp
    x6, flow, mask = _glue_inputs(7)
    mask = (mask - 0.5) * 8.0

    def want(dtype):
        a, f, m = x6.to(dtype), flow.to(dtype), torch.sigmoid(mask.to(dtype))
        return backwarp(a[:, :3], f[:, :2]) * m + backwarp(a[:, 3:], f[:, 2:4]) * (1.0 - m)
    out = torch.full((2, 3, 32, 64), -7.5, device="cuda")
    R.rife_blend(x6.cuda(), _state(flow.cuda(), mask.cuda()), out)
    _bars("blend", out.cpu(), want(torch.float64), want(torch.float32), record_property)


# ---- the session
@pytest.fixture(scope="module")
def sessions(R):
    from visiondepth3d_amd.rife import RifeSession
    return RifeSession("cuda", renderer=R, conv="bf16x3"), RifeSession("cpu")


@pytest.mark.parametrize("h,w", [(64, 96), (70, 100)])
def test_run_rife_on_the_bf16x3_session_vs_cpu_float64_and_float32(R, sessions, h, w, record_property):
    """run_rife(R, RifeSession("cuda", renderer=R, conv="bf16x3"), f1, f2, 3): the float32 prediction's RMS error against a float64 CPU run of RifeNet is <= 1.5 x the
    float32 CPU run's + 1e-9; the uint8 frames against the float32 CPU run with the reference's NumPy glue differ by <= 1 level on < 1 % of the samples (the bar
    test_run_rife_with_the_interpolation_network_vs_cpu_float32 holds the MIOpen path to); the two frames are equal; not the plain average; repeatable bits.
    Measured (profiles/r11_rife_x3.md): RMS 2.6e-8 against the float32 CPU run's 1.6e-7 / 2.0e-7 (0.17 x / 0.13 x), maximum 1.5e-7 against 2.1e-6 / 4.9e-6."""
    import copy
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.upscale import run_rife
    hip, cpu = sessions
    f1, _ = synth.synth_frame(1, h, w)
    f2, _ = synth.synth_frame(2, h, w)
    merged = np.concatenate((f1.astype(np.float32) / 255.0, f2.astype(np.float32) / 255.0), axis=2)
    batch = torch.from_numpy(np.repeat(np.expand_dims(np.transpose(merged, (2, 0, 1)), 0).astype(np.float32), 2, axis=0))
    with torch.no_grad():
        ref64 = copy.deepcopy(cpu.net).double()(batch.double())
    ref32 = cpu(batch)
    pred = hip(batch.cuda())
    assert pred.shape == (2, 3, h, w) and pred.dtype == torch.float32
    assert torch.equal(hip(batch.cuda()), pred)
    e, e32 = (pred.cpu().double() - ref64), (ref32.double() - ref64)
    r, r32, m, m32 = float(e.pow(2).mean().sqrt()), float(e32.pow(2).mean().sqrt()), float(e.abs().max()), float(e32.abs().max())
    print(f"RIFE_X3_E2E {h}x{w} rms {r:.3e} (f32 cpu {r32:.3e}, {r / r32:.2f}x) max {m:.3e} (f32 cpu {m32:.3e}, {m / m32:.2f}x)")
    record_property("rife_x3_e2e", dict(rms=r, rms32=r32, max=m, max32=m32, rms_ratio=r / r32, max_ratio=m / m32))
    assert r <= 1.5 * r32 + 1e-9, (r, r32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    outs = run_rife(R, hip, to(f1), to(f2), 3)
    assert len(outs) == 2 and all(tuple(o.shape) == (h, w, 3) and o.dtype == torch.uint8 for o in outs)
    want = [(fr * 255).astype(np.uint8) for fr in np.transpose(np.clip(ref32.numpy(), 0, 1), (0, 2, 3, 1))]
    for o, wnt in zip(outs, want):
        d = np.abs(o.cpu().numpy().astype(int) - wnt.astype(int))
        assert d.max() <= 1 and (d > 0).mean() < 1e-2, (int(d.max()), float((d > 0).mean()))
    assert torch.equal(outs[0], outs[1])
    mid = ((f1.astype(np.int32) + f2.astype(np.int32)) // 2).astype(np.uint8)
    assert np.abs(outs[0].cpu().numpy().astype(int) - mid.astype(int)).mean() > 0.3
    assert all(torch.equal(a, b) for a, b in zip(run_rife(R, hip, to(f1), to(f2), 3), outs))


def test_no_library_convolution_or_resampling_is_on_the_bf16x3_path(R, sessions, monkeypatch):
    """With Conv2d.forward, ConvTranspose2d.forward, F.grid_sample and F.interpolate raising, the conv="bf16x3" forward still runs; session.routes lists 36 launches
    (12 per block), all on vd3d_conv_ifn; afterwards the default session still gives the bits it gave before."""
    from visiondepth3d_amd.rife import RifeSession
    hip, _ = sessions
    x = torch.rand(1, 6, 64, 96, generator=torch.Generator().manual_seed(3)).cuda()
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    default = RifeSession("cuda")
    before = default(x).clone()
    with monkeypatch.context() as mp:
        def boom(*a, **k):
            raise AssertionError("a library op on the bf16x3 path")
        mp.setattr(torch.nn.Conv2d, "forward", boom)
        mp.setattr(torch.nn.ConvTranspose2d, "forward", boom)
        mp.setattr(F, "grid_sample", boom)
        mp.setattr(F, "interpolate", boom)
        with pytest.raises(AssertionError):
            default(x)
        y = hip(x)
    assert y.shape == (1, 3, 64, 96) and bool(torch.isfinite(y).all())
    assert len(hip.routes) == 36 and all(k.startswith("vd3d_conv_ifn/") for _, k, _ in hip.routes)
    for b in range(3):
        blk = hip.routes[12 * b:12 * b + 12]
        assert all(n.startswith(f"block{b}.") for n, _, _ in blk)
        assert [k.rsplit("/", 1)[1] for _, k, _ in blk] == ["k3s2"] * 2 + ["k3s1"] * 8 + ["t4s2"] * 2
        assert [s[3:] for _, _, s in blk] == [(16, 64), (48, 96)] + [(96, 96)] * 9 + [(96, 32)]
    assert [k for _, k, _ in hip.glue_routes] == ["vd3d_rife_warp_pack", "vd3d_rife_update"] * 3 + ["vd3d_rife_blend"]
    assert torch.equal(default(x), before)
