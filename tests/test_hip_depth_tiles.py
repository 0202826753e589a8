"""GPU tests (-m gpu) of the tiled high-resolution depth path (csrc/vd3d_tiles.hip, DepthPipe.infer_tiled_bgr_u8 / depth_frames_u8(tiled=True)):
the gather, the blend (same-size and fused-bicubic predictions) and the percentile normalisation bit for bit against numpy statements of the
reference (core/render_depth.py:102-194), then the whole chain with a deterministic model and with a real network."""
import numpy as np
import pytest

from visiondepth3d_amd import depth_tiles as DT
from visiondepth3d_amd import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL_GEOMETRIES = [(120, 160, 64, 8), (61, 200, 64, 8), (40, 50, 64, 8), (100, 150, 48, 0), (90, 130, 64, 20)]


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def pipe(R):
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    return DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R, processor=dict(PROCESSORS["da"], size=(112, 112), multiple=14))


def _bits_equal(got, exp):
    """bit-identical float32 planes, NaNs compared as equal"""
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    nan = np.isnan(exp)
    return got.shape == exp.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], exp.view(np.uint32)[~nan])


# ---- gather ------------------------------------------------------------------------------------------------------------------------
def test_gather_bit_exact_vs_oracle_odd_pitch(R, oracle):
    H, W, tile, pad = 97, 131, 48, 4
    plan = DT.tile_plan(H, W, tile, pad)
    assert plan.n_tiles == 12 and len(plan.groups) > 3
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, size=(2, H + 3, W + 9, 3), dtype=np.uint8)
    frames = torch.from_numpy(buf).cuda()[:, :H, :W]            # row pitch 3 * 140 = 420 bytes, frame stride 100 rows
    assert not frames.is_contiguous() and frames.stride(1) == 420
    for g in plan.groups:
        org = torch.from_numpy(plan.gather_origins(g, 2)).cuda()
        got = R.tile_gather_cubic_u8(frames, org, g.ch, g.cw, g.chs, g.cws).cpu().numpy()
        assert got.shape == (2 * len(g.tiles), g.chs, g.cws, 3)
        k = 0
        for b in range(2):
            for t in g.tiles:
                tl = plan.tiles[t]
                crop = np.ascontiguousarray(buf[b, tl.yp0:tl.yp1, tl.xp0:tl.xp1])
                assert np.array_equal(got[k], oracle.resize_cubic_u8(crop, g.chs, g.cws)), (g, b, t)
                k += 1


# ---- blend -------------------------------------------------------------------------------------------------------------------------
def _pool(plan, B, preds):
    """preds[b][t]: float32 plane of tile t, frame b -> (pool, tile_tab, pred_off) on the device, in TilePlan.blend_tables' order"""
    shapes = [preds[0][g.tiles[0]].shape for g in plan.groups]
    tab, off, total = plan.blend_tables(B, shapes)
    pool = np.zeros(total, np.float32)
    for b in range(B):
        for t in range(plan.n_tiles):
            p = preds[b][t]
            pool[off[b * plan.n_tiles + t]: off[b * plan.n_tiles + t] + p.size] = p.reshape(-1)
    return torch.from_numpy(pool).cuda(), torch.from_numpy(tab).cuda(), torch.from_numpy(off).cuda()


@pytest.mark.parametrize("geom", SMALL_GEOMETRIES)
def test_blend_same_size_bit_exact_vs_numpy_loop(R, geom):
    H, W, tile, pad = geom
    B = 2
    plan = DT.tile_plan(H, W, tile, pad)
    rng = np.random.default_rng(H * 7 + W)
    preds = [[(rng.standard_normal((t.chs, t.cws)) * 3.0).astype(np.float32) for t in plan.tiles] for _ in range(B)]
    t0, t1 = plan.tiles[0], plan.tiles[-1]
    preds[0][0][t0.yc0 + t0.th // 2, t0.xc0 + t0.tw // 2] = np.nan
    preds[1][plan.n_tiles - 1][t1.yc0 + t1.th // 3, t1.xc0 + t1.tw // 3] = np.inf
    pool, tab, off = _pool(plan, B, preds)
    wp = torch.from_numpy(plan.weight_pool()).cuda()
    got = R.tile_blend(pool, off, tab, wp, B, H, W, tile, pad).cpu().numpy()
    again = R.tile_blend(pool, off, tab, wp, B, H, W, tile, pad).cpu().numpy()
    with np.errstate(all="ignore"):
        for b in range(B):
            exp = DT.blend_tiles_numpy(plan, [preds[b][i][t.yc0:t.yc0 + t.th, t.xc0:t.xc0 + t.tw] for i, t in enumerate(plan.tiles)])
            assert np.isnan(exp).any() or np.isinf(exp).any()
            assert _bits_equal(got[b], exp), (geom, b)
    assert _bits_equal(again, got)


def _bicubic_up_f32(p, H, W):
    """vd3d_cubic.h:bicubic_at operation by operation in float32 (source index = the single-rounded s * (i + 0.5) - 0.5)."""
    f = np.float32
    ph, pw = p.shape

    def axis(n_in, n_out):
        s = f(n_in) / f(n_out)
        r = (np.float64(s) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(f)   # exact in double, rounded once: the fused form
        fl = np.floor(r)
        t = r - fl
        A = f(-0.75)
        c1 = lambda x: ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
        c2 = lambda x: ((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A
        c = np.stack([c2(t + f(1)), c1(t), c1(f(1) - t), c2((f(1) - t) + f(1))], 1).astype(f)
        idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None], 0, n_in - 1)
        return idx, c
    iy, cy = axis(ph, H)
    ix, cx = axis(pw, W)
    acc = np.zeros((H, W), f)
    for i in range(4):
        rows = p[iy[:, i]]                                         # [H, pw]
        r = np.zeros((H, W), f)
        for j in range(4):
            r = r + rows[:, ix[:, j]] * cx[None, :, j]
        acc = acc + r * cy[:, i, None]
    return acc


@pytest.mark.parametrize("geom,shrink", [((80, 210, 80, 0), {(84, 84): (28, 28), (84, 56): (42, 28)}), ((120, 160, 64, 8), None)])
def test_blend_fused_bicubic_equals_upsampled_same_size(R, geom, shrink):
    H, W, tile, pad = geom
    B = 2
    plan = DT.tile_plan(H, W, tile, pad)
    if shrink is not None:
        assert {(g.chs, g.cws) for g in plan.groups} == set(shrink)
    small_of = (lambda g: shrink[(g.chs, g.cws)]) if shrink is not None else (lambda g: (max(2, g.chs // 2 - 1), max(2, g.cws // 3 + 1)))
    rng = np.random.default_rng(3)
    gshape = {t: small_of(g) for g in plan.groups for t in g.tiles}
    small = [[(rng.standard_normal(gshape[i]) * 2.0 + 1.0).astype(np.float32) for i in range(plan.n_tiles)] for _ in range(B)]
    big = [[_bicubic_up_f32(small[b][i], t.chs, t.cws) for i, t in enumerate(plan.tiles)] for b in range(B)]
    wp = torch.from_numpy(plan.weight_pool()).cuda()
    pool, tab, off = _pool(plan, B, small)
    fused = R.tile_blend(pool, off, tab, wp, B, H, W, tile, pad).cpu().numpy()
    pool, tab, off = _pool(plan, B, big)
    same = R.tile_blend(pool, off, tab, wp, B, H, W, tile, pad).cpu().numpy()
    assert np.isfinite(same).all() and _bits_equal(fused, same)


# ---- normalise ---------------------------------------------------------------------------------------------------------------------
def _norm_cases(h, w, rng):
    n = h * w
    base = rng.standard_normal(n).astype(np.float32)
    c = {"random": base.copy(), "flat": np.full(n, -3.25, np.float32), "zeros": np.zeros(n, np.float32)}
    v = base.copy()
    v[rng.choice(n, 5, replace=False)] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    c["nonfinite"] = v
    v = (base * np.float32(0.1)).astype(np.float32)
    k = max(2, n // 100)
    idx = rng.choice(n, 2 * k, replace=False)
    v[idx[:k]] = 1e5
    v[idx[k:]] = -1e5                                                   # 2 % outliers: the percentiles differ from min and max
    c["outliers"] = v
    half = (np.arange(n) % 2).astype(np.float32)
    c["range_under_1e-6"] = half * np.float32(9e-7)                     # percentile range and min-max range below 1e-6: all 128
    c["range_over_1e-6"] = half * np.float32(1.1e-6)
    v = np.full(n, 2.0, np.float32)
    v[:max(1, n // 300)] = 3.0                                         # percentiles collapse, min-max does not
    c["minmax_fallback"] = v
    c["signed_zero"] = np.where(base > 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32) + (np.abs(base) > 2) * base
    return c


@pytest.mark.parametrize("h,w", [(1, 1001), (50, 37), (256, 320)])
def test_normalize_pclip_byte_identical_to_numpy(R, h, w):
    cases = _norm_cases(h, w, np.random.default_rng(h + w))
    names = sorted(cases)
    planes = np.stack([cases[k].reshape(h, w) for k in names])
    dev = torch.from_numpy(planes).cuda()
    lohi = torch.zeros((len(names), 2), dtype=torch.float32, device="cuda")
    got = R.depth_normalize_pclip(dev, lo_hi=lohi).cpu().numpy()
    inv = R.depth_normalize_pclip(dev, invert=True).cpu().numpy()
    lohi = lohi.cpu().numpy()
    for i, k in enumerate(names):
        exp = DT.normalize_to_u8_numpy(planes[i])
        d = np.abs(got[i].astype(int) - exp.astype(int))
        assert np.array_equal(got[i], exp), (k, int(d.max()), int(np.count_nonzero(d)))
        assert np.array_equal(inv[i], DT.normalize_to_u8_numpy(planes[i], invert=True)), k
        clean = np.nan_to_num(planes[i], nan=0.0, posinf=0.0, neginf=0.0)
        assert lohi[i, 0] == np.percentile(clean, 1.0) and lohi[i, 1] == np.percentile(clean, 99.0), k
    assert len(np.unique(got[names.index("outliers")])) > 100 and np.all(got[names.index("range_under_1e-6")] == 128)


# ---- whole chain, deterministic model ----------------------------------------------------------------------------------------------
def _model_torch(tiles):
    """pointwise float32 function of the pixel and of its position inside the tile (separate, correctly rounded operations)"""
    t = tiles.float()
    n, h, w, _ = t.shape
    v = t[..., 0] * 0.5 + t[..., 1] * 0.25
    v = v + t[..., 2] * 0.125
    yy = torch.arange(h, device=t.device, dtype=torch.float32)[None, :, None] * 0.375
    xx = torch.arange(w, device=t.device, dtype=torch.float32)[None, None, :] * 0.625
    return (v + yy) + xx


def _model_numpy(tile):
    t = tile.astype(np.float32)
    v = t[..., 0] * np.float32(0.5) + t[..., 1] * np.float32(0.25)
    v = v + t[..., 2] * np.float32(0.125)
    yy = np.arange(t.shape[0], dtype=np.float32)[:, None] * np.float32(0.375)
    xx = np.arange(t.shape[1], dtype=np.float32)[None, :] * np.float32(0.625)
    return (v + yy) + xx


def _chain_numpy(oracle, frame, tgt_h, tgt_w, tile, pad, model, invert=False):
    H, W = frame.shape[:2]
    if (tgt_h, tgt_w) == (H, W):
        img = frame
    elif tgt_w < W or tgt_h < H:
        img = oracle.resize_area(frame, tgt_w, tgt_h)
    else:
        img = oracle.resize_cubic_u8(frame, tgt_h, tgt_w)
    plan = DT.tile_plan(tgt_h, tgt_w, tile, pad)
    centres = []
    for t in plan.tiles:
        crop = np.ascontiguousarray(img[t.yp0:t.yp1, t.xp0:t.xp1])
        pred = model(oracle.resize_cubic_u8(crop, t.chs, t.cws), t)
        centres.append(pred[t.yc0:t.yc0 + t.th, t.xc0:t.xc0 + t.tw])
    d = DT.blend_tiles_numpy(plan, centres)
    u8 = DT.normalize_to_u8_numpy(d, invert)
    return d, (u8 if (tgt_h, tgt_w) == (H, W) else oracle.resize_cubic_u8(u8, H, W))


@pytest.mark.parametrize("frame_hw,inference_size", [((256, 320), None), ((512, 640), (320, 256)), ((128, 160), (320, 256))])
def test_whole_chain_deterministic_model_byte_identical(R, pipe, oracle, frame_hw, inference_size):
    H, W = frame_hw
    tile, pad = 128, 16
    plan = DT.tile_plan(256, 320, tile, pad)
    assert plan.n_tiles == 12 and len(plan.groups) == 9
    wacc = np.zeros((256, 320), np.float32)
    for t in plan.tiles:
        wacc[t.y0:t.y1, t.x0:t.x1] += DT.hann_tile_weight(plan.core, t.th, t.tw)
    share = float((wacc <= 1e-8).mean())
    assert share <= 0.009, share                                       # the 1 % clip must be able to absorb the degenerate weights
    frames_np = np.stack([synth.synth_frame(i, H, W)[0] for i in range(2)])
    frames = torch.from_numpy(frames_np).cuda()
    d = pipe.infer_tiled_bgr_u8(frames, inference_size, tile=tile, pad=pad, tile_batch=5, model_call=_model_torch)
    assert d.dtype == torch.float32 and tuple(d.shape) == (2, 256, 320)
    u8 = R.depth_normalize_pclip(d)
    if (H, W) != (256, 320):
        u8 = torch.stack([R.resize_cubic_u8(u8[b], H, W) for b in range(2)])
    with np.errstate(all="ignore"):
        for b in range(2):
            exp_d, exp_u8 = _chain_numpy(oracle, frames_np[b], 256, 320, tile, pad, lambda tl, t: _model_numpy(tl))
            assert _bits_equal(d[b].cpu().numpy(), exp_d), (frame_hw, b)
            assert np.array_equal(u8[b].cpu().numpy(), exp_u8), (frame_hw, b)
            assert len(np.unique(exp_u8)) > 64


# ---- whole chain, real network -----------------------------------------------------------------------------------------------------
def test_whole_chain_real_network_vs_one_tile_at_a_time(R, pipe, oracle):
    """depth_frames_u8(tiled=True) against the reference's structure on the same network: one tile per forward through the protocol call
    pipe([tile], inference_size=(cws, chs)), host blend, numpy hand-off.  The sides differ by batched vs single forwards, the device input
    preparation and the bicubic's association; bar = tests/test_hip_depth_e2e.py's on the uint8 plane: exact >= 0.995, max <= 1."""
    H, W, tile, pad = 256, 320, 128, 16
    frames_np = np.stack([synth.synth_frame(i, H, W)[0] for i in range(2)])
    got = pipe.depth_frames_u8(torch.from_numpy(frames_np).cuda(), tiled=True, tile=tile, pad=pad).cpu().numpy()
    assert got.shape == (2, H, W) and got.dtype == np.uint8

    def one_tile(tile_bgr, t):
        out = pipe([np.ascontiguousarray(tile_bgr[..., ::-1])], inference_size=(t.cws, t.chs))
        p = out[0]["predicted_depth"].cpu().numpy()
        assert p.shape == (t.chs, t.cws)
        return p
    for b in range(2):
        with np.errstate(all="ignore"):
            _, exp = _chain_numpy(oracle, frames_np[b], H, W, tile, pad, one_tile)
        d = np.abs(got[b].astype(int) - exp.astype(int))
        exact, mx = float((d == 0).mean()), int(d.max())
        print(f"tiled real network frame {b}: exact {exact:.5f} max {mx}")
        assert exact >= 0.995 and mx <= 1, (b, exact, mx)


# ---- rules -------------------------------------------------------------------------------------------------------------------------
def test_blend_refuses_more_than_four_covering_tiles(R):
    from visiondepth3d_amd._lib import Vd3dError
    f = torch.zeros(64, dtype=torch.float32, device="cuda")
    tab = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    for tile, pad in ((64, 25), (100, 38)):   # just above 3/8 tile (24 and 37 are built: the 90 x 130, tile 64, pad 20 geometry runs three)
        with pytest.raises(Vd3dError) as e:
            R.tile_blend(f, off, tab, f, 1, 8, 8, tile, pad)
        assert e.value.code == -4 and "pad" in str(e.value)


def test_mixed_shrink_grow_inference_size_is_refused(pipe):
    frames = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError, match="shrinks one side"):
        pipe.infer_tiled_bgr_u8(frames, inference_size=(32, 128), tile=48, pad=4, model_call=_model_torch)


def _memo_network(pipe, monkeypatch):
    """The library convolutions / GEMMs behind the network are not bit-reproducible from call to call; equal inputs get the first call's prediction
    so that the code AROUND the network can be compared exactly."""
    real, memo = pipe.infer_bgr_u8, {}

    def cached(frames, inference_size=None, raw=False, at_inference_size=False):
        key = (tuple(frames.shape), int(frames.to(torch.int64).sum()), inference_size, raw, at_inference_size)
        if key not in memo:
            memo[key] = real(frames, inference_size, raw=raw, at_inference_size=at_inference_size)
        return memo[key]
    monkeypatch.setattr(pipe, "infer_bgr_u8", cached)


def test_untiled_default_is_unchanged(pipe, monkeypatch):
    """tiled=False is the method as it was: depth_to_u8 of the prediction at the size the pipeline saw, INTER_CUBIC back to the frame size"""
    from visiondepth3d_amd.depth import depth_to_u8
    _memo_network(pipe, monkeypatch)
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, 120, 160)[0] for i in range(2)])).cuda()
    exp = depth_to_u8(pipe.infer_bgr_u8(frames, None, at_inference_size=True), False)
    assert torch.equal(pipe.depth_frames_u8(frames), exp)
    assert torch.equal(pipe.depth_frames_u8(frames, tiled=False, invert=True, tile=64, pad=8), 255 - exp)
    small = depth_to_u8(pipe.infer_bgr_u8(frames, (112, 84), at_inference_size=True), False)
    exp2 = torch.stack([pipe.renderer.resize_cubic_u8(small[b], 120, 160) for b in range(2)])
    assert torch.equal(pipe.depth_frames_u8(frames, inference_size=(112, 84)), exp2)


def test_call_tiled_protocol(pipe, monkeypatch):
    _memo_network(pipe, monkeypatch)
    rgb = np.ascontiguousarray(synth.synth_frame(0, 96, 128)[0][..., ::-1])
    out = pipe.call_tiled([rgb, rgb], tile=64, pad=8)
    assert len(out) == 2 and tuple(out[0]["predicted_depth"].shape) == (96, 128) and out[0]["predicted_depth"].dtype == torch.float32
    assert torch.equal(out[0]["predicted_depth"].nan_to_num(), out[1]["predicted_depth"].nan_to_num())
    direct = pipe.infer_tiled_bgr_u8(torch.from_numpy(np.ascontiguousarray(rgb[..., ::-1]))[None].cuda(), tile=64, pad=8)[0]
    assert torch.equal(out[0]["predicted_depth"].nan_to_num(), direct.nan_to_num())
    single = pipe.call_tiled(rgb, inference_size=(64, 48), tile=64, pad=8)
    assert len(single) == 1 and tuple(single[0]["predicted_depth"].shape) == (48, 64)
