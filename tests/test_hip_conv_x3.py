"""GPU tests (-m gpu) of the bf16x3 3 x 3 convolution (vd3d_conv3x3_x3, csrc/vd3d_conv_x3.hip) and of the depth leg that runs on it
(DepthPipe(gemm="bf16x3", conv="bf16x3")).

A floating-point kernel: the bar is stated against FLOAT64, beside PyTorch's float32 CPU convolution on the same operands (the yardstick of
test_conv3x3_x2_is_float32_faithful, for the reason its docstring gives: MIOpen's float32 result depends on the solver a box picks).  Then exact cases that pin
the term set and the geometry, the refusals, and the depth leg against the STOCK float32 Hugging Face graph with the bar the existing split modes meet."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
CL = torch.channels_last


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _conv_x3(R, x, w):
    img = R.conv3x3_x3_pack(w)
    assert img is not None
    return R.conv3x3_x3(x.contiguous(memory_format=CL), img, w.shape[0])


FAITHFUL_CASES = [(1, 16, 32, 16, 64), (2, 37, 66, 128, 128), (1, 50, 45, 96, 128), (3, 19, 33, 64, 64), (1, 74, 132, 128, 64),      # the nine x2 cases
                  (1, 1, 1, 32, 64), (2, 17, 31, 48, 128), (2, 45, 70, 64, 32), (1, 16, 32, 16, 32),
                  (1, 37, 66, 256, 256), (2, 74, 132, 256, 256), (1, 19, 33, 1024, 256), (1, 148, 264, 256, 128),                        # DA-V2-Large / DPT-Large shapes
                  (1, 1, 1, 16, 256), (1, 13, 47, 48, 256), (2, 9, 33, 96, 64), (1, 7, 65, 48, 32)]                                      # one pixel; ragged tiles; C_in 48 / 96


@pytest.mark.parametrize("B,H,W,Cin,Cout", FAITHFUL_CASES)
def test_conv3x3_x3_is_float32_faithful(R, B, H, W, Cin, Cout, record_property):
    """vd3d_conv3x3_x3 against a float64 convolution, beside PyTorch's float32 CPU convolution on the same operands.  The bar is the one the coarser fp16x2
    kernel is held to (tests/test_hip_gemm.py test_conv3x3_x2_is_float32_faithful): maximum of |y - y64| / conv(|x|, |w|) <= max(2.5 x the yardstick's, 2^-21),
    relative RMS <= 1.5 x the yardstick's + 1e-9.  Post-ReLU inputs with log-normal channel scales, like the maps the fusion stage sees; sizes that are not
    multiples of the 8 x 32 tile in either direction, one-pixel images, 48- and 96-channel inputs, the 256-channel shapes of DA-V2-Large.  The measured ratios
    per case are in profiles/r08_conv_x3.md: 0.35 - 0.95 x the yardstick's on both figures, except the one-pixel 32 -> 64 case (maximum 1.30 x = 6.8e-8, RMS
    1.21 x), which is why the bf16x3 GEMM's tighter bar (1.25 x, floor 2^-24) is not the one asserted here.  Two calls return identical bits."""
    g = torch.Generator(device="cuda").manual_seed(B * 100 + H)
    x = torch.relu(torch.randn(B, Cin, H, W, device="cuda", generator=g)) * torch.exp(torch.randn(1, Cin, 1, 1, device="cuda", generator=g))
    x = x.contiguous(memory_format=CL)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) * 0.05
    img = R.conv3x3_x3_pack(w)
    assert img is not None
    y = R.conv3x3_x3(x, img, Cout)
    assert y.shape == (B, Cout, H, W) and y.is_contiguous(memory_format=CL) and bool(torch.isfinite(y).all())
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    y32 = F.conv2d(x.cpu(), w.cpu(), None, 1, 1).to(x.device)
    scale = F.conv2d(x.abs().double(), w.abs().double(), None, 1, 1) + 1e-30
    e3, e32 = float(((y.double() - ref).abs() / scale).max()), float(((y32.double() - ref).abs() / scale).max())
    r3 = float((y.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    r32 = float((y32.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"CONV_X3_ERR {B}x{H}x{W}x{Cin}->{Cout} max {e3:.3e} (f32 {e32:.3e}, {e3 / max(e32, 1e-30):.2f}x) rms {r3:.3e} (f32 {r32:.3e}, {r3 / max(r32, 1e-30):.2f}x)")
    record_property("conv_x3_err", dict(e3=e3, e32=e32, r3=r3, r32=r32))
    assert e3 <= max(2.5 * e32, 2.0 ** -21), (e3, e32)
    assert r3 <= 1.5 * r32 + 1e-9, (r3, r32)
    assert torch.equal(R.conv3x3_x3(x, img, Cout), y)


def _exact(R, x, w):
    """Every kept product and every partial sum exactly representable: conv(|x|, |w|) < 2^24, so float32 accumulation is exact in any order."""
    assert float(F.conv2d(x.abs().double(), w.abs().double(), None, 1, 1).max()) < 2 ** 24
    y = _conv_x3(R, x, w)
    return torch.equal(y.double(), F.conv2d(x.double(), w.double(), None, 1, 1))


@pytest.mark.parametrize("Cout", [32, 64, 128, 256])
def test_conv3x3_x3_exact_small_integers_pin_the_geometry(R, Cout):
    """(a) the x2 test's small-integer pattern: one bf16 term per operand, so only x1 w1 is non-zero -- a transposed tap, a shifted halo, a swapped channel half or
    a permuted output channel shows.  W not a multiple of 32, H not a multiple of 8, two frames, C_in with three chunks."""
    B, Cin, H, W = 2, 48, 21, 45
    xi = ((torch.arange(B * Cin * H * W, device="cuda").view(B, Cin, H, W) * 7) % 5 - 2).float()
    wi = ((torch.arange(Cout * Cin * 9, device="cuda").view(Cout, Cin, 3, 3) * 11) % 7 - 3).float()
    assert _exact(R, xi, wi)


def _odd_ints(shape, lo, hi, g):
    v = torch.randint(lo, hi, shape, device="cuda", generator=g) | 1
    s = torch.randint(0, 2, shape, device="cuda", generator=g) * 2 - 1
    return (v * s).float()


@pytest.mark.parametrize("Cout", [32, 64, 128, 256])
def test_conv3x3_x3_exact_two_term_by_two_term(R, Cout):
    """(b) odd 9-bit integers on both sides (two bf16 terms each): x1 w1 + x1 w2 + x2 w1 + x2 w2 is the exact product, and dropping x2 w2 (odd x odd low bits)
    changes it.  A four-tap mask (asymmetric, so a mirrored tap shows too) and C_in 16 keep sum |x||w| <= 4 x 16 x 511^2 = 16 711 744 < 2^24."""
    g = torch.Generator(device="cuda").manual_seed(Cout)
    B, Cin, H, W = 1, 16, 11, 37
    x = _odd_ints((B, Cin, H, W), 256, 512, g)
    w = _odd_ints((Cout, Cin, 3, 3), 256, 512, g)
    mask = torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 0.0, 1.0]], device="cuda")
    assert _exact(R, x, w * mask)


@pytest.mark.parametrize("Cout", [32, 64, 128, 256])
def test_conv3x3_x3_exact_three_term_by_one_term(R, Cout):
    """(c) odd 17-bit integers (three bf16 terms, the third one the lowest bit) against weights in {-1, 0, 1} with few non-zeros, then the roles swapped: fails when
    x3 w1 or x1 w3 is dropped, or when the split rounds instead of truncating exactly."""
    g = torch.Generator(device="cuda").manual_seed(100 + Cout)
    B, Cin, H, W = 1, 32, 10, 35
    big = _odd_ints((B, Cin, H, W), 2 ** 16, 2 ** 17, g)
    sparse_w = torch.zeros(Cout, Cin, 3, 3, device="cuda")
    oc = torch.arange(Cout, device="cuda")
    for j in range(6):   # six non-zeros per output channel, over taps and channels: sum |x||w| < 6 x 2^17 < 2^24
        sparse_w[oc, (oc * 5 + j * 7) % Cin, (oc + j) % 3, (oc // 3 + 2 * j) % 3] = 1.0 if j % 2 == 0 else -1.0
    assert _exact(R, big, sparse_w)
    big_w = _odd_ints((Cout, Cin, 3, 3), 2 ** 16, 2 ** 17, g)
    sparse_x = torch.zeros(B, Cin, H, W, device="cuda")
    sel = torch.rand(B, 1, H, W, device="cuda", generator=g) < 0.08     # few non-zero pixels, ONE channel each: at most 9 products per output
    ch = torch.randint(0, Cin, (B, 1, H, W), device="cuda", generator=g)
    sparse_x.scatter_(1, ch, torch.where(sel, torch.randint(0, 2, (B, 1, H, W), device="cuda", generator=g).float() * 2 - 1, torch.zeros(B, 1, H, W, device="cuda")))
    assert float(sparse_x.abs().sum()) > 0
    assert _exact(R, sparse_x, big_w)


def test_conv3x3_x3_nan_and_inf_inputs_give_nan(R):
    x = torch.ones(1, 16, 9, 33, device="cuda")
    x[0, 3, 4, 5] = float("inf")
    x[0, 7, 8, 32] = float("nan")
    y = _conv_x3(R, x, torch.ones(32, 16, 3, 3, device="cuda"))
    assert bool(torch.isnan(y[0, :, 3:6, 4:7]).all()) and bool(torch.isnan(y[0, :, 7:, 31:]).all())
    assert bool(torch.isfinite(y[0, :, 0, 20:]).all())


def test_conv3x3_x3_refuses_shapes_it_does_not_build(R):
    from visiondepth3d_amd import _lib
    assert R.conv3x3_x3_pack(torch.zeros(16, 64, 3, 3, device="cuda")) is None      # C_out 16 (32 / 64 / 128 / 256 are built)
    assert R.conv3x3_x3_pack(torch.zeros(64, 20, 3, 3, device="cuda")) is None      # C_in not a multiple of 16
    assert R.conv3x3_x3_pack(torch.zeros(64, 64, 1, 1, device="cuda")) is None      # not 3 x 3
    # the C entry point checks its arguments before it launches anything: -4 (VD3D_E_UNSUPPORTED) and a message that names the rule
    L = _lib.lib()
    img = R.conv3x3_x3_pack(torch.zeros(32, 16, 3, 3, device="cuda"))
    buf = torch.zeros(2 * 16 * 4 * 4 + 4, device="cuda")
    out = torch.zeros(2 * 32 * 4 * 4, device="cuda")
    vp = ctypes.c_void_p
    args = lambda xp, B: (R._ctx, vp(xp), B, 4, 4, 16, vp(img.data_ptr()), 32, vp(out.data_ptr()))   # noqa: E731
    assert L.vd3d_conv3x3_x3(*args(buf.data_ptr() + 4, 1)) == -4 and b"aligned" in L.vd3d_last_error()
    assert L.vd3d_conv3x3_x3(*args(buf.data_ptr(), 0)) == -4 and b"batch" in L.vd3d_last_error()
    assert L.vd3d_conv3x3_x3(*args(buf.data_ptr(), 65536)) == -4 and b"batch" in L.vd3d_last_error()
    assert L.vd3d_conv3x3_x3(R._ctx, vp(buf.data_ptr()), 1, 0, 4, 16, vp(img.data_ptr()), 32, vp(out.data_ptr())) == -4
    assert L.vd3d_conv3x3_x3(R._ctx, vp(buf.data_ptr()), 1, 4, 4, 16, vp(img.data_ptr()), 48, vp(out.data_ptr())) == -4 and b"C_out" in L.vd3d_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0   # nothing ran


def _depth_leg(R, name, n_frames, H, W, tag, stock=None, **kw):
    from test_hip_depth_e2e import _plane_stats, _record, _stock_u8_planes
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import DepthPipe
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, H, W)[0] for i in range(n_frames)])).cuda()
    exp_u8, exp_pred = (stock or (lambda f: _stock_u8_planes(name, f)))(frames)
    pipe = DepthPipe(name, device="cuda", dtype=torch.float32, renderer=R, gemm="bf16x3", conv="bf16x3", **kw)
    pred = pipe.infer_bgr_u8(frames, raw=True)
    st = _plane_stats(R.depth_handoff(pred, H, W), exp_u8)
    st["pred_max_err_of_range"] = float((pred - exp_pred).abs().max()) / float(exp_pred.max() - exp_pred.min())
    st["routes"] = {k: v[0] for k, v in pipe.conv_routes.items()}
    _record(tag, st)
    print("CONV_X3_LEG", tag, {k: v for k, v in st.items() if k != "routes"}, sorted(pipe.conv_routes.items()))
    assert any(v[0] == "bf16x3" for v in pipe.conv_routes.values()), pipe.conv_routes
    assert st["pred_max_err_of_range"] < 1e-4, st
    assert st["exact"] >= 0.995 and st["max"] <= 1, st


@pytest.mark.parametrize("name,n,H,W", [("depth-anything-v2-small", 2, 1080, 1920), ("depth-anything-v2-base", 1, 2160, 3840), ("depth-anything-v2-large", 1, 1080, 1920)])
def test_depth_leg_conv_x3_meets_the_float32_legs_bar(R, name, n, H, W):
    """DepthPipe(gemm="bf16x3", conv="bf16x3") against the STOCK float32 graph, the bar of the existing split modes (tests/test_hip_gemm.py, tests/test_hip_dpt.py):
    raw prediction within 1e-4 of its range, >= 99.5 % of the uint8 hand-off bytes identical, no byte off by more than one level.  DA-V2-Large exercises the
    256-channel kernel."""
    _depth_leg(R, name, n, H, W, f"conv_x3_{name.rsplit('-', 1)[1]}_{H}p")


def test_dpt_large_conv_x3_meets_the_float32_legs_bar_1080p(R):
    from test_hip_dpt import SEED, _stock_dpt_u8_planes
    _depth_leg(R, "dpt-large", 2, 1080, 1920, "dpt_conv_x3_1080p", stock=_stock_dpt_u8_planes, seed=SEED)


def _count_conv_x3(R, monkeypatch):
    calls = [0]
    orig = R.conv3x3_x3

    def counted(*a, **kw):
        calls[0] += 1
        return orig(*a, **kw)
    monkeypatch.setattr(R, "conv3x3_x3", counted)
    return calls


def test_conv_x3_routes_are_recorded_and_nothing_falls_back_silently(R, monkeypatch):
    """DA-V2-Base at 4K, one forward of two frames: conv_routes names all 20 three-by-three stride-1 convolutions (4 neck, 14 fusion, 2 head); whatever stayed on the library
    names the size rule; each of neck, fusion and head has at least one convolution on the new kernel; the kernel ran exactly once per "bf16x3" entry."""
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import DepthPipe
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, 2160, 3840)[0] for i in range(2)])).cuda()
    pipe = DepthPipe("depth-anything-v2-base", device="cuda", dtype=torch.float32, renderer=R, gemm="bf16x3", conv="bf16x3")
    calls = _count_conv_x3(R, monkeypatch)
    pipe.infer_bgr_u8(frames, raw=True)
    routes = pipe.conv_routes
    want = [n for n, m in pipe.model.named_modules()   # the first fusion layer has no residual input: its residual_layer1 (two more convolutions) never runs
            if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and "layers.0.residual_layer1" not in n]
    assert len(want) == 20 and sorted(routes) == sorted(want), (sorted(routes), sorted(want))
    assert sum(n.startswith("neck.convs.") for n in want) == 4 and sum(n.startswith("neck.fusion_stage.") for n in want) == 14 and sum(n.startswith("head.") for n in want) == 2
    for n, (where, why) in routes.items():
        assert where in ("bf16x3", "library"), (n, where)
        if where == "library":
            assert why.startswith("size rule"), (n, why)
    for part in ("neck.convs.", "neck.fusion_stage.", "head."):
        assert any(n.startswith(part) and v[0] == "bf16x3" for n, v in routes.items()), (part, routes)
    assert calls[0] == sum(v[0] == "bf16x3" for v in routes.values()), (calls, routes)


def test_conv_none_is_todays_behaviour(R, monkeypatch):
    """conv=None never calls the new kernel, records no route, and computes bit for bit what a pipe built without the keyword computes.
    The comparison runs with PyTorch's deterministic-kernels flag on: without it MIOpen's kernels for the reassemble stage's transposed and stride-2
    convolutions do not repeat their own bits (measured: the SAME pipe called twice differed by 4.6e-6 in the prediction, the backbone outputs identical,
    reassemble layers 0, 1 and 3 not), so no two forwards of today's code compare equal either; with the flag two pipes agree bit for bit."""
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import DepthPipe
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    frames = torch.from_numpy(np.stack([synth.synth_frame(0, 1080, 1920)[0]])).cuda()
    calls = _count_conv_x3(R, monkeypatch)
    a = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R, gemm="bf16x3", conv=None)
    b = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R, gemm="bf16x3")
    pa, pb = a.infer_bgr_u8(frames, raw=True), b.infer_bgr_u8(frames, raw=True)
    assert calls[0] == 0 and a.conv_routes == {} and a.conv is None
    assert all("forward" not in m.__dict__ for m in a.model.neck.convs)
    assert torch.equal(pa, pb)


def test_conv3x3_x3_on_a_second_device():
    """The > 64 KB dynamic-LDS opt-in is a per-device function attribute: a call on device 1 after one on device 0 must succeed."""
    if torch.cuda.device_count() < 2:
        pytest.skip("only one GPU visible")
    from visiondepth3d_amd.render_3d import Renderer
    w = torch.randn(128, 32, 3, 3) * 0.1
    x = torch.randn(1, 32, 20, 40)
    outs = []
    for d in (0, 1):
        r = Renderer(d)
        try:
            with torch.cuda.device(d):
                outs.append(_conv_x3(r, x.to(f"cuda:{d}"), w.to(f"cuda:{d}")).cpu())
        finally:
            r.close()
    assert torch.equal(outs[0], outs[1])
