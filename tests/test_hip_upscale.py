"""GPU parity of the up-scale stage glue (core/merged_pipeline.py:219-284) and of the uint8 INTER_CUBIC / INTER_AREA
resizes: every HIP kernel against the oracle bit for bit, then ``run_esrgan`` end to end -- the network's own prediction is taken from
the device, everything around it is recomputed with the oracle and must agree exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    r = Renderer(0)
    yield r
    r.close()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("shape,dsize", [((37, 53), (74, 106)), ((37, 53), (91, 140)), ((64, 48), (48, 36)), ((30, 40, 3), (120, 160)),
                                         ((50, 70, 3), (20, 33)), ((5, 4), (17, 9)), ((1, 9), (3, 27)), ((270, 480), (1080, 1920)),
                                         ((540, 960, 3), (2160, 3840)), ((432, 768, 3), (108, 192)), ((33, 21, 3), (33, 21))])
def test_resize_cubic_u8_bit_exact(R, oracle, shape, dsize):
    rng = np.random.default_rng(shape[0] * 131 + dsize[1])
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    got = R.resize_cubic_u8(T(a), *dsize).cpu().numpy()
    assert np.array_equal(got, oracle.resize_cubic_u8(a, *dsize))


@pytest.mark.parametrize("shape,dsize", [((64, 96, 3), (32, 48)), ((64, 96, 3), (16, 24)), ((60, 90, 3), (45, 67)), ((1080, 1920, 3), (810, 1440)),
                                         ((1080, 1920, 3), (270, 480)), ((40, 60, 3), (50, 30)), ((21, 33, 3), (21, 33))])
def test_resize_area_u8_bit_exact(R, oracle, shape, dsize):
    rng = np.random.default_rng(shape[0] + dsize[0])
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    got = R.resize_area_u8(T(a), *dsize).cpu().numpy()
    assert np.array_equal(got, oracle.resize_area(a, dsize[1], dsize[0]))


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("channels_last", [True, False])
def test_esr_preprocess_crop(R, oracle, dtype, channels_last):
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (41, 57, 3), dtype=np.uint8)
    td = getattr(torch, dtype)
    for (y0, x0, h, w) in [(0, 0, 41, 57), (5, 9, 20, 31), (40, 56, 1, 1)]:
        x = R.esr_preprocess(T(f), y0, x0, h, w, dtype=td, channels_last=channels_last)
        assert tuple(x.shape) == (1, 3, h, w)
        assert x.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        want = torch.from_numpy(oracle.esr_pre(f[y0:y0 + h, x0:x0 + w])).to(td)      # one rounding from float32, like the kernel
        assert torch.equal(x[0].cpu(), want)


def test_esr_postprocess_window_and_layouts(R, oracle):
    rng = np.random.default_rng(4)
    p = (rng.standard_normal((1, 3, 36, 52)) * 0.6 + 0.5).astype(np.float32)
    p[0, 1, 3, 4] = np.nan
    want = oracle.esr_post(p[0])
    for cl in (False, True):
        t = T(p)
        if cl:
            t = t.contiguous(memory_format=torch.channels_last)
        assert np.array_equal(R.esr_postprocess(t).cpu().numpy(), want)
        canvas = torch.full((30, 40, 3), 7, dtype=torch.uint8, device="cuda")
        R.esr_postprocess(t, out=canvas, window=(8, 12, 10, 20), dst_yx=(15, 5))
        c = canvas.cpu().numpy()
        assert np.array_equal(c[15:25, 5:25], want[8:18, 12:32])
        c[15:25, 5:25] = 7
        assert np.all(c == 7)
    with pytest.raises(AssertionError):
        R.esr_postprocess(T(p), out=torch.empty((10, 10, 3), dtype=torch.uint8, device="cuda"))


def test_add_weighted_u8_bit_exact(R, oracle):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (90, 121, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (90, 121, 3), dtype=np.uint8)
    for alpha in (0.85, 0.5, 0.25, 1.0):
        got = R.add_weighted_u8(T(a), alpha, T(b), 1 - alpha).cpu().numpy()
        assert np.array_equal(got, oracle.add_weighted_u8(a, alpha, b, 1 - alpha))


def _run_esrgan_with_oracle_glue(up, oracle, frame, preds, blend_mode, input_res_pct, target_size, tile, tile_pad):
    """run_esrgan (core/merged_pipeline.py:237-284) with numpy / oracle glue.  ``preds``: the network outputs the device run produced, in
    call order (the library convolutions are not run-to-run deterministic, so the session is replayed, not re-run); the INPUT each call
    saw is re-derived here with the oracle and must have the recorded shape."""
    it = iter(preds)

    def session(crop, y0=0, x0=0):
        p, (fy, fx, fh, fw) = next(it)
        assert (fy, fx, fh, fw) == (y0, x0, crop.shape[0], crop.shape[1])      # the device run cut the same crop
        assert p.shape == (3, crop.shape[0] * up.scale, crop.shape[1] * up.scale)
        return p

    original = frame
    if input_res_pct != 100:
        h, w = frame.shape[:2]
        nh, nw = int(h * input_res_pct / 100), int(w * input_res_pct / 100)
        frame = oracle.resize_area(frame, nw, nh) if input_res_pct < 100 else oracle.resize_cubic_u8(frame, nh, nw)
    if tile:
        h, w = frame.shape[:2]
        out = np.zeros_like(frame)
        for y in range(0, h, tile):
            for x in range(0, w, tile):
                y0, x0 = max(0, y - tile_pad), max(0, x - tile_pad)
                y1, x1 = min(h, y + tile + tile_pad), min(w, x + tile + tile_pad)
                upc = oracle.esr_post(session(frame[y0:y1, x0:x1], y0, x0))
                yc0, xc0 = y - y0, x - x0
                yc1, xc1 = yc0 + min(tile, h - y), xc0 + min(tile, w - x)
                out[y:y + min(tile, h - y), x:x + min(tile, w - x)] = upc[yc0:yc1, xc0:xc1]
        upscaled = out
    else:
        upscaled = oracle.esr_post(session(frame))
    s = up.scale
    upscaled = oracle.resize_cubic_u8(upscaled, frame.shape[0] * s, frame.shape[1] * s)
    upscaled = oracle.resize_cubic_u8(upscaled, original.shape[0], original.shape[1])
    if target_size:
        upscaled = oracle.resize_cubic_u8(upscaled, target_size[1], target_size[0])
    if blend_mode == "OFF":
        return upscaled
    alpha = {"LOW": 0.85, "MEDIUM": 0.5, "HIGH": 0.25}[blend_mode]
    return oracle.add_weighted_u8(upscaled, alpha, original, 1 - alpha)


@pytest.mark.parametrize("model,kw", [
    ("RealESR_Animex4_fp16", dict(blend_mode="OFF", input_res_pct=100, target_size=None, tile=None, tile_pad=8)),
    ("RealESR_Animex4_fp16", dict(blend_mode="LOW", input_res_pct=50, target_size=None, tile=None, tile_pad=8)),
    ("RealESR_Animex4_fp16", dict(blend_mode="OFF", input_res_pct=75, target_size=(200, 120), tile=None, tile_pad=8)),
    ("RealESR_Gx4_fp16", dict(blend_mode="HIGH", input_res_pct=100, target_size=None, tile=32, tile_pad=8)),
    ("RealESRGAN_x4_fp16", dict(blend_mode="MEDIUM", input_res_pct=25, target_size=None, tile=None, tile_pad=8)),
])
def test_run_esrgan_end_to_end(R, oracle, model, kw):
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.upscale import Upscaler
    torch.manual_seed(9)
    # float32 network: the device prediction is deterministic for one input, so device glue and oracle glue see the same numbers
    up = Upscaler(R, model, dtype=torch.float32)
    frame, _ = synth.synth_frame(3, 72, 104)
    preds, infer = [], up._infer

    def recording(f, y0=0, x0=0, h=None, w=None):
        p = infer(f, y0, x0, h, w)
        preds.append((p.cpu().numpy()[0], (y0, x0, f.shape[0] - y0 if h is None else h, f.shape[1] - x0 if w is None else w)))
        return p
    up._infer = recording
    got = up.run_esrgan(T(frame), **kw).cpu().numpy()
    want = _run_esrgan_with_oracle_glue(up, oracle, frame, preds, **kw)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.abs(got.astype(int) - want.astype(int)).max()


def test_upscale_4x_output_and_fp16_default(R):
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.upscale import Upscaler
    up = Upscaler(R, "RealESR_Gx4_fp16")
    assert up.dtype == torch.float16                 # the reference's ONNX exports are fp16
    frame, _ = synth.synth_frame(1, 54, 96)
    out = up.upscale(T(frame))
    assert tuple(out.shape) == (216, 384, 3) and out.dtype == torch.uint8


def test_depth_frames_u8_with_inference_size(R, oracle):
    """a24 with an explicit inference size (core/render_depth.py:1113-1116,1907-1917): prediction at the inference size -> uint8 ->
    INTER_CUBIC back to the frame size."""
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import DepthPipe, depth_to_u8
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", renderer=R)
    frame, _ = synth.synth_frame(2, 180, 320)
    fr = T(frame)[None]
    pred = pipe.infer_bgr_u8(fr, (224, 126), at_inference_size=True)
    assert tuple(pred.shape) == (1, 126, 224)
    pipe.infer_bgr_u8 = lambda *a, **k: pred        # the network is not run-to-run deterministic (atomics in the GEMMs): pin its output
    got = pipe.depth_frames_u8(fr, inference_size=(224, 126), invert=True)
    assert tuple(got.shape) == (1, 180, 320) and got.dtype == torch.uint8
    small = depth_to_u8(pred, True)[0].cpu().numpy()
    assert np.array_equal(got[0].cpu().numpy(), oracle.resize_cubic_u8(small, 180, 320))
    # without an inference size nothing is resized
    del pipe.infer_bgr_u8
    full = pipe.depth_frames_u8(fr)
    assert tuple(full.shape) == (1, 180, 320)


# ---- optional NV12 wire format --------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(2, 2), (54, 96), (270, 482), (1080, 1920), (2160, 3840)])
def test_nv12_both_ways_bit_exact_and_round_trip(R, oracle, h, w):
    from visiondepth3d_amd import synth
    frame = synth.synth_frame(4, h, w)[0] if h >= 16 else np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    nv = R.bgr_to_nv12(T(frame)).cpu().numpy()
    assert nv.shape == (h * 3 // 2, w)
    assert np.array_equal(nv, oracle.bgr_to_nv12(frame))
    rng = np.random.default_rng(h + w)
    noise = rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)           # every code value, in and out of the legal range
    for src in (nv, noise):
        assert np.array_equal(R.nv12_to_bgr(T(src)).cpu().numpy(), oracle.nv12_to_bgr(src))
    # luma survives a round trip within the 8-bit quantisation of two 20-bit fixed-point maps
    back = R.nv12_to_bgr(T(nv)).cpu().numpy().astype(int)
    y0 = (0.114 * frame[..., 0] + 0.587 * frame[..., 1] + 0.299 * frame[..., 2])
    y1 = (0.114 * back[..., 0] + 0.587 * back[..., 1] + 0.299 * back[..., 2])
    dy = np.abs(y0 - y1)            # saturated chroma at hard edges may clip: bound the bulk, not the worst pixel
    assert dy.mean() <= 1.0 and np.percentile(dy, 99) <= 3.0
    with pytest.raises(AssertionError):
        R.bgr_to_nv12(T(np.zeros((5, 4, 3), np.uint8)))


# ---- body layers on the matrix cores (vd3d_conv3x3_c64_f16) ----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 32), (17, 33), (5, 7), (1, 1), (64, 96), (135, 240), (300, 500), (540, 960), (1080, 1920)])   # up to 4 080 workgroups: several per CU
@pytest.mark.parametrize("act", [True, False])
def test_conv3x3_c64_f16_vs_float32_reference(R, H, W, act):
    """fp16 operands, float32 accumulate on the MFMA units vs ATen's float32 convolution of the SAME fp16-rounded operands: the only
    differences are the summation order (float32) and the final fp16 rounding of the output (2^-11 relative)."""
    import torch.nn.functional as F
    from visiondepth3d_amd.upscale import conv_weight_fragments
    gen = torch.Generator().manual_seed(H * 1000 + W)
    x = (torch.randn(1, 64, H, W, generator=gen) * 0.7).half()
    w = (torch.randn(64, 64, 3, 3, generator=gen) * 0.06).half()          # asymmetric in every index
    b = torch.randn(64, generator=gen) * 0.1
    sl = torch.rand(64, generator=gen) * 0.5 if act else None
    ref = F.conv2d(x.float().cuda(), w.float().cuda(), b.cuda(), padding=1)
    if act:
        ref = torch.where(ref >= 0, ref, ref * sl.cuda()[None, :, None, None])
    xd = x.cuda().contiguous(memory_format=torch.channels_last)
    got = R.conv3x3_c64(xd, conv_weight_fragments(w).cuda(), b.cuda(), sl.cuda() if act else None)
    assert got.dtype == torch.float16 and got.is_contiguous(memory_format=torch.channels_last)
    err = (got.float() - ref).abs()
    tol = 2e-3 * ref.abs() + 2e-3
    assert bool((err <= tol).all()), (float(err.max()), float(ref.abs().max()))
    # and much tighter on average than an fp16-accumulating kernel could be
    assert float(err.mean()) < 2e-4 * max(1.0, float(ref.abs().mean()))


@pytest.mark.parametrize("H,W", [(5, 7), (1, 1), (64, 66), (135, 240), (540, 960)])
@pytest.mark.parametrize("act", [True, False])
def test_conv3x3_head_vs_float32_reference(R, H, W, act):
    """3 -> 64 head layer (vd3d_conv3x3_head_f16): fp16 operands, float32 accumulate vs ATen's float32 convolution of the same fp16-rounded
    operands: summation order and the final fp16 rounding only."""
    import torch.nn.functional as F
    from visiondepth3d_amd.upscale import head_weight_matrix
    gen = torch.Generator().manual_seed(7 * H + W)
    x = torch.rand(1, 3, H, W, generator=gen).half()
    w = (torch.randn(64, 3, 3, 3, generator=gen) * 0.2).half()
    b = torch.randn(64, generator=gen) * 0.1
    sl = torch.rand(64, generator=gen) * 0.5 if act else None
    ref = F.conv2d(x.float().cuda(), w.float().cuda(), b.cuda(), padding=1)
    if act:
        ref = torch.where(ref >= 0, ref, ref * sl.cuda()[None, :, None, None])
    got = R.conv3x3_head(x.cuda().contiguous(memory_format=torch.channels_last), head_weight_matrix(w).cuda(), b.cuda(), sl.cuda() if act else None)
    assert got.dtype == torch.float16 and tuple(got.shape) == (1, 64, H, W) and got.is_contiguous(memory_format=torch.channels_last)
    err = (got.float() - ref).abs()
    assert bool((err <= 1e-3 * ref.abs() + 1e-3).all()), float(err.max())


@pytest.mark.parametrize("r", [4, 2])
@pytest.mark.parametrize("H,W", [(3, 5), (64, 64), (70, 100), (135, 241), (1, 1), (2, 63), (1, 64), (1, 65)])
def test_esr_tail_equals_pixel_shuffle_plus_nearest_add(R, H, W, r):
    """vd3d_esr_tail_f32 == float(pixel_shuffle(t[:, :3 r^2], r) + interpolate(x, nearest)) bit for bit (fp16 addition like the network's)."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(H * 31 + W + r)
    t = (torch.randn(1, 64, H, W, generator=gen) * 0.3).half().cuda().contiguous(memory_format=torch.channels_last)
    x = torch.rand(1, 3, H, W, generator=gen).half().cuda().contiguous(memory_format=torch.channels_last)
    exp = (F.pixel_shuffle(t[:, :3 * r * r], r) + F.interpolate(x, scale_factor=r, mode="nearest")).float()
    got = R.esr_tail(t, x, r)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, H * r, W * r)
    assert torch.equal(got, exp.contiguous())


def test_upscaler_hip_body_matches_the_library_convolutions(R):
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.upscale import Upscaler
    torch.manual_seed(3)
    a = Upscaler(R, "RealESR_Gx4_fp16", hip_body=True)
    assert a._body is not None and len(a._body) == 32
    b = Upscaler(R, "RealESR_Gx4_fp16", net=a.net, hip_body=False)
    ref = Upscaler(R, "RealESR_Gx4_fp16", net=torch.nn.Module.float(__import__("copy").deepcopy(a.net)), dtype=torch.float32)
    frame, _ = synth.synth_frame(5, 70, 100)
    pa, pb, pr = a._infer(T(frame)), b._infer(T(frame)), ref._infer(T(frame))
    # both fp16 paths sit within fp16 noise of the float32 network, and the hand-written body is not the worse of the two by much
    ea, eb = float((pa - pr).abs().mean()), float((pb - pr).abs().mean())
    assert ea < 5e-3 and ea <= 2.0 * eb + 1e-4, (ea, eb)
    oa, ob = a.upscale(T(frame)), b.upscale(T(frame))
    d = (oa.int() - ob.int()).abs()
    assert int(d.max()) <= 3 and float((d > 1).float().mean()) < 0.01


def test_run_rife_glue(R):
    """run_rife (core/merged_pipeline.py:195-218) around a stand-in session: the device glue must equal the reference's numpy lines."""
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.upscale import run_rife
    f1, _ = synth.synth_frame(1, 46, 62)
    f2, _ = synth.synth_frame(2, 46, 62)
    seen = {}

    def session(x):                                   # a "network" that mixes the two frames and overshoots [0, 1] in places
        seen["x"] = x.clone()
        return x[:, :3] * 0.75 + x[:, 3:] * 0.5 - 0.1
    outs = run_rife(R, session, T(f1), T(f2), 3)
    assert len(outs) == 2 and all(tuple(o.shape) == (46, 62, 3) and o.dtype == torch.uint8 for o in outs)
    merged = np.concatenate((f1.astype(np.float32) / 255.0, f2.astype(np.float32) / 255.0), axis=2)          # concatenate_images :195-196
    tensor = np.expand_dims(np.transpose(merged, (2, 0, 1)), 0).astype(np.float32)                             # preprocess_rife :198-201
    batch = np.repeat(tensor, 2, axis=0)
    assert np.array_equal(seen["x"].cpu().numpy(), batch)
    out = session(torch.from_numpy(batch)).numpy()
    out = np.transpose(np.clip(out, 0, 1), (0, 2, 3, 1))
    want = [(fr * 255).astype(np.uint8) for fr in out]                                                        # :214-216
    # the stand-in session runs in float32 on both sides; ATen's elementwise kernels agree bit for bit between CPU and GPU here
    for o, wnt in zip(outs, want):
        d = np.abs(o.cpu().numpy().astype(int) - wnt.astype(int))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
    assert run_rife(R, None, T(f1), T(f2), 2) == []


def test_run_rife_with_the_interpolation_network_vs_cpu_float32(R):
    """run_rife end to end with a real interpolation network (VERDICT r2 missing 1): HIP pre-process -> IFNet HDv3 on PyTorch-ROCm ->
    HIP post-process, against the same module run in float32 on the CPU with the reference's NumPy glue (core/merged_pipeline.py:195-216).
    The convolutions differ by float32 association noise (MIOpen vs oneDNN): <= 1 level, on < 1 % of the samples."""
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.rife import RifeSession
    from visiondepth3d_amd.upscale import run_rife
    f1, _ = synth.synth_frame(1, 270, 480)
    f2, _ = synth.synth_frame(2, 270, 480)
    gpu, cpu = RifeSession("cuda"), RifeSession("cpu")
    outs = run_rife(R, gpu, T(f1), T(f2), 3)
    assert len(outs) == 2 and all(tuple(o.shape) == (270, 480, 3) and o.dtype == torch.uint8 for o in outs)
    merged = np.concatenate((f1.astype(np.float32) / 255.0, f2.astype(np.float32) / 255.0), axis=2)
    batch = np.repeat(np.expand_dims(np.transpose(merged, (2, 0, 1)), 0).astype(np.float32), 2, axis=0)
    ref = cpu(torch.from_numpy(batch)).numpy()
    want = [(fr * 255).astype(np.uint8) for fr in np.transpose(np.clip(ref, 0, 1), (0, 2, 3, 1))]
    for o, wnt in zip(outs, want):
        d = np.abs(o.cpu().numpy().astype(int) - wnt.astype(int))
        assert d.max() <= 1 and (d > 0).mean() < 1e-2, (int(d.max()), float((d > 0).mean()))
    assert int((outs[0].int() - outs[1].int()).abs().max()) <= 1   # the reference repeats one mid-point input (:212)
    mid = ((f1.astype(np.int32) + f2.astype(np.int32)) // 2).astype(np.uint8)
    assert np.abs(outs[0].cpu().numpy().astype(int) - mid.astype(int)).mean() > 0.3      # not a plain average of the frames
