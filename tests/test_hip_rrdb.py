"""GPU tests of the RRDB (RealESRGAN_x4plus) path: k_conv3x3_dense_f16 against ATen's float32 convolution of the same fp16-rounded operands, the
epilogue and the up2 load on known answers, one residual-in-residual block and the whole network against the float32 module graph, determinism of the
in-place slices, the refusals of the entry point, and ``run_esrgan`` around it."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
CL = torch.channels_last
SIZES = [(1, 1), (5, 7), (8, 32), (9, 33), (17, 65), (135, 240)]   # one pixel, sub-tile, exactly one 32 x 8 tile, one past it both ways, several workgroups per CU
# (C_in, C_out, up2): the five convolutions of a dense block, and the 64 -> 64 layers behind the body without and with the folded nearest x2
SHAPES = [(64, 32, False), (96, 32, False), (128, 32, False), (160, 32, False), (192, 64, False), (64, 64, False), (64, 64, True)]


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    r = Renderer(0)
    yield r
    r.close()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.int16)


def _buf(c, h, w, gen, scale=0.7):
    return (torch.randn(1, c, h, w, generator=gen) * scale).half().cuda().contiguous(memory_format=CL)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("cin,cout,up2", SHAPES)
def test_dense_kernel_vs_float32_reference(R, cin, cout, up2, H, W):
    """fp16 operands, float32 accumulate on the MFMA units vs ATen's float32 convolution of the SAME fp16-rounded operands (the bar of
    test_conv3x3_c64_f16_vs_float32_reference).  The input is the first C_in channels of a 192-stride buffer, the output the next slice of that buffer
    (192 -> 64 and up2 have no room / another size: the slice [64, 128) of a second 192-stride buffer); everything outside the slice is a canary.
    With up2, (H, W) is the size of the INPUT and the output is (2H, 2W)."""
    import torch.nn.functional as F
    from visiondepth3d_amd.upscale import dense_weight_fragments
    gen = torch.Generator().manual_seed(H * 1000 + W + cin * 7 + cout)
    xb = _buf(192, H, W, gen)
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * 0.06 * (64.0 / cin) ** 0.5).half()   # asymmetric in every index
    b = torch.randn(cout, generator=gen) * 0.1
    slope = 0.2 if cout == 32 else 1.0
    OH, OW = (2 * H, 2 * W) if up2 else (H, W)
    in_place = cin + cout <= 192 and not up2
    yb = xb if in_place else _buf(192, OH, OW, gen)
    off = cin if in_place else 64
    before = yb.clone()
    src = xb[:, :cin].float()
    if up2:
        src = F.interpolate(src, scale_factor=2, mode="nearest")
    ref = F.conv2d(src, w.float().cuda(), b.cuda(), padding=1)
    ref = torch.where(ref >= 0, ref, ref * slope)
    R.conv3x3_dense(xb, cin, dense_weight_fragments(w).cuda(), b.cuda(), cout, yb, off, slope=slope, up2=up2)
    torch.cuda.synchronize()
    got = yb[:, off:off + cout].float()
    err = (got - ref).abs()
    tol = 2e-3 * ref.abs() + 2e-3
    assert bool((err <= tol).all()), (float(err.max()), float(ref.abs().max()))
    assert float(err.mean()) < 2e-4 * max(1.0, float(ref.abs().mean()))
    keep = torch.ones(192, dtype=torch.bool, device="cuda")
    keep[off:off + cout] = False
    assert torch.equal(yb[:, keep].view(torch.int16), before[:, keep].view(torch.int16))      # the canary: nothing outside the slice was touched


@pytest.mark.parametrize("cout", [32, 64])
def test_epilogue_known_answers(R, cout):
    """Zero weights: the result is exactly fp16((leaky(bias, slope) * alpha + r1) * beta + r2), every operation one float32 rounding."""
    from visiondepth3d_amd.upscale import dense_weight_fragments
    H, W = 9, 33
    gen = torch.Generator().manual_seed(cout)
    x = _buf(192, H, W, gen)
    r1, r2 = _buf(64, H, W, gen), _buf(192, H, W, gen)               # two different pixel strides
    wf = dense_weight_fragments(torch.zeros(cout, 96, 3, 3)).cuda()
    b = torch.randn(cout, generator=gen)                             # both signs
    alpha, beta, slope = np.float32(0.2), np.float32(0.7), np.float32(0.3)
    out = torch.full((1, cout, H, W), 7.0, dtype=torch.float16, device="cuda").contiguous(memory_format=CL)
    R.conv3x3_dense(x, 96, wf, b.cuda(), cout, out, 0, slope=float(slope), r1=r1, alpha=float(alpha), r2=r2, beta=float(beta))
    bn = b.numpy().astype(np.float32)[None, :, None, None]
    v = np.where(bn >= 0, bn, bn * slope).astype(np.float32)         # slope BEFORE the residuals
    v = (v * alpha).astype(np.float32) + r1[:, :cout].float().cpu().numpy()
    v = (v * beta).astype(np.float32) + r2[:, :cout].float().cpu().numpy()
    assert np.array_equal(_bits(out), v.astype(np.float16).view(np.int16))
    # r1 alone, and no residual: the bare activation
    R.conv3x3_dense(x, 96, wf, b.cuda(), cout, out, 0, slope=float(slope), r1=r1, alpha=float(alpha))
    v1 = (np.where(bn >= 0, bn, bn * slope).astype(np.float32) * alpha).astype(np.float32) + r1[:, :cout].float().cpu().numpy()
    assert np.array_equal(_bits(out), v1.astype(np.float16).view(np.int16))
    R.conv3x3_dense(x, 96, wf, b.cuda(), cout, out, 0, slope=float(slope))
    v0 = np.broadcast_to(np.where(bn >= 0, bn, bn * slope).astype(np.float32), (1, cout, H, W))
    assert np.array_equal(_bits(out), v0.astype(np.float16).view(np.int16))


def test_up2_centre_tap_is_the_nearest_upsampled_input(R):
    """Weights that pick the centre tap of ONE input channel per output channel (a permutation, so a swapped index shows): bit for bit F.interpolate(nearest)."""
    import torch.nn.functional as F
    from visiondepth3d_amd.upscale import dense_weight_fragments
    H, W = 9, 35
    gen = torch.Generator().manual_seed(11)
    x = _buf(64, H, W, gen)
    perm = [(5 * o + 3) % 64 for o in range(64)]
    w = torch.zeros(64, 64, 3, 3)
    for o, i in enumerate(perm):
        w[o, i, 1, 1] = 1.0
    out = torch.empty((1, 64, 2 * H, 2 * W), dtype=torch.float16, device="cuda").contiguous(memory_format=CL)
    R.conv3x3_dense(x, 64, dense_weight_fragments(w).cuda(), torch.zeros(64, device="cuda"), 64, out, 0, up2=True)
    exp = F.interpolate(x[:, perm], scale_factor=2, mode="nearest")
    assert torch.equal(out.view(torch.int16), exp.contiguous(memory_format=CL).view(torch.int16))


def _one_block(R):
    from visiondepth3d_amd.upscale import RRDBNet, Upscaler
    torch.manual_seed(5)
    up = Upscaler(R, "RealESRGAN_x4_fp16", net=RRDBNet(num_block=1), rrdb_hip=True)
    assert up._rrdb is not None and len(up._rrdb) == 3
    return up


def _run_block(up, x):
    """The three RDBs of body[0] on the kernels (15 launches), like Upscaler._forward_rrdb runs them."""
    H, W = int(x.shape[2]), int(x.shape[3])
    P, Q, S = (torch.zeros((1, 192, H, W), dtype=torch.float16, device="cuda").contiguous(memory_format=CL) for _ in range(3))
    P[:, :64].copy_(x)
    up._rdb(up._rrdb[0], P, Q)
    up._rdb(up._rrdb[1], Q, S)
    up._rdb(up._rrdb[2], S, Q, r2=P)
    torch.cuda.synchronize()
    return Q[:, :64].clone()


def test_one_rrdb_block_vs_float32_module(R):
    up = _one_block(R)
    x = _buf(64, 17, 33, torch.Generator().manual_seed(17), 0.5)
    with torch.no_grad():
        block16 = up.net.body[0]
        ref = copy.deepcopy(block16).float()(x.float())              # the float32 module on the fp16-rounded weights
        lib = block16(x).float()                                     # the fp16 module graph
    got = _run_block(up, x).float()
    ea, eb = float((got - ref).abs().mean()), float((lib - ref).abs().mean())
    print(f"one RRDB block 17 x 33: mean error HIP {ea:.3e}, fp16 module graph {eb:.3e}, mean |ref| {float(ref.abs().mean()):.3e}")
    assert ea <= 2.0 * eb + 1e-4, (ea, eb)


def test_block_is_bit_for_bit_repeatable(R):
    """135 x 240 (several workgroups per CU) five times: the in-place slices and the LDS ring leave no room for a race."""
    up = _one_block(R)
    x = _buf(64, 135, 240, torch.Generator().manual_seed(23), 0.5)
    first = _run_block(up, x)
    assert bool(torch.isfinite(first.float()).all()) and float(first.float().abs().mean()) > 0.05
    for _ in range(4):
        assert torch.equal(_run_block(up, x).view(torch.int16), first.view(torch.int16))


@pytest.fixture(scope="module")
def nets(R):
    """One seeded RealESRGAN_x4plus three ways: the kernels, the fp16 module graph, the float32 module graph (on the same fp16-rounded weights)."""
    from visiondepth3d_amd.upscale import Upscaler
    torch.manual_seed(3)
    a = Upscaler(R, "RealESRGAN_x4_fp16", rrdb_hip=True)
    b = Upscaler(R, "RealESRGAN_x4_fp16", net=a.net, rrdb_hip=False)
    ref = Upscaler(R, "RealESRGAN_x4_fp16", net=torch.nn.Module.float(copy.deepcopy(a.net)), dtype=torch.float32)
    return a, b, ref


def test_whole_network_routing_and_prediction(R, nets, monkeypatch):
    import torch.nn.functional as F
    from visiondepth3d_amd import synth
    a, b, ref = nets
    assert a._rrdb is not None and len(a._rrdb) == 69 and b._rrdb is None and ref._rrdb is None
    frame, _ = synth.synth_frame(5, 24, 40)
    calls = {"conv2d": 0, "cat": 0, "interpolate": 0}

    def counted(name, fn):
        def f(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)
        return f
    with monkeypatch.context() as m:
        m.setattr(F, "conv2d", counted("conv2d", F.conv2d))
        m.setattr(torch, "cat", counted("cat", torch.cat))
        m.setattr(F, "interpolate", counted("interpolate", F.interpolate))
        pa = a._infer(T(frame))
        assert calls == {"conv2d": 0, "cat": 0, "interpolate": 0}, calls
        pb = b._infer(T(frame))
        assert calls["conv2d"] == 351 and calls["cat"] == 69 * 4 and calls["interpolate"] == 2, calls    # the counters do see the module graph
    pr = ref._infer(T(frame))
    assert tuple(pa.shape) == (1, 3, 96, 160) and pa.dtype == torch.float32
    ea, eb = float((pa - pr).abs().mean()), float((pb - pr).abs().mean())
    print(f"RealESRGAN_x4plus 24 x 40: mean error HIP {ea:.3e}, fp16 module graph {eb:.3e}; float32 prediction {float(pr.min()):.3f} .. {float(pr.max()):.3f}")
    assert float(pr.max() - pr.min()) > 0.5                           # not a flat plane that compares equal whatever was computed
    assert ea <= 2.0 * eb + 1e-4, (ea, eb)
    oa, ob = a.upscale(T(frame)), b.upscale(T(frame))
    d = (oa.int() - ob.int()).abs()
    assert int(d.max()) <= 3 and float((d > 1).float().mean()) < 0.01, (int(d.max()), float((d > 1).float().mean()))
    assert len(torch.unique(oa)) > 50


def test_whole_network_is_bit_for_bit_repeatable(R, nets):
    from visiondepth3d_amd import synth
    a = nets[0]
    frame, _ = synth.synth_frame(5, 24, 40)
    p1, p2 = a._infer(T(frame)), a._infer(T(frame))
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32))


def test_entry_point_refuses_what_it_does_not_build(R):
    """Each broken rule: VD3D_E_UNSUPPORTED with a message, and the output buffer keeps its bits (nothing was launched)."""
    from visiondepth3d_amd import _abi
    from visiondepth3d_amd.upscale import dense_weight_fragments
    H, W = 8, 32
    gen = torch.Generator().manual_seed(2)
    x = _buf(192, H, W, gen)
    y = _buf(192, H, W, gen)
    wf = dense_weight_fragments(torch.randn(64, 192, 3, 3, generator=gen)).cuda()
    bias = torch.zeros(64, device="cuda")
    x0, y0 = x.clone(), y.clone()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(xp=None, x_stride=192, cin=64, cout=32, yp=None, y_stride=192, y_off=64):
        return R._L.vd3d_conv3x3_dense_f16(R._ctx, xp or p(x), H, W, x_stride, cin, p(wf), p(bias), cout, 1.0, 1.0, None, 0, 1.0, None, 0, 0,
                                           yp or p(y), y_stride, y_off)
    cases = {
        "C_in 80": dict(cin=80),
        "C_out 48": dict(cout=48),
        "stride < C_in": dict(x_stride=64, cin=96),
        "misaligned x": dict(xp=p(x, 8)),
        "misaligned y": dict(yp=p(y, 2)),
        "slice meets the input": dict(xp=p(x), yp=p(x), cin=96, y_off=64),
        "slice partly meets the input": dict(xp=p(x), yp=p(x), cin=128, cout=64, y_off=96),
    }
    for name, kw in cases.items():
        rc = call(**kw)
        assert rc == _abi.E_UNSUPPORTED, (name, rc)
        assert len(R._L.vd3d_last_error()) > 20, name
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int16), x0.view(torch.int16)) and torch.equal(y.view(torch.int16), y0.view(torch.int16))
    assert call(xp=p(x), yp=p(x), cin=96, y_off=96) == 0              # the neighbouring slice of the same buffer is the supported case
    torch.cuda.synchronize()
    assert torch.equal(x[:, :96].view(torch.int16), x0[:, :96].view(torch.int16)) and not torch.equal(x[:, 96:128], x0[:, 96:128])


def test_run_esrgan_glue_with_the_rrdb_kernels(R, nets):
    from visiondepth3d_amd import synth
    a, b, _ = nets
    frame, _ = synth.synth_frame(7, 48, 64)
    kw = dict(input_res_pct=50, model_name="RealESRGAN_x4_fp16", tile=16, tile_pad=4)
    oa, ob = a.run_esrgan(T(frame), **kw), b.run_esrgan(T(frame), **kw)
    assert oa.dtype == torch.uint8 and tuple(oa.shape) == (48, 64, 3) and tuple(ob.shape) == (48, 64, 3)
    d = (oa.int() - ob.int()).abs()
    assert int(d.max()) <= 3 and float((d > 1).float().mean()) < 0.01, (int(d.max()), float((d > 1).float().mean()))
    assert len(torch.unique(oa)) > 20
