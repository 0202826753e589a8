"""Host-side checks (no GPU) of the tiled-depth geometry, blend window and percentile hand-off (visiondepth3d_amd/depth_tiles.py):
tile_plan against a brute-force statement of the reference's loops (core/render_depth.py:118-133,149-153), hann_tile_weight against a
float64 evaluation of the same cubic convolution, normalize_to_u8_numpy on its three branches."""
import numpy as np
import pytest

from visiondepth3d_amd import depth_tiles as DT

# (tgt_h, tgt_w, tile, pad)
GEOMETRIES = [(120, 160, 64, 8), (61, 200, 64, 8), (40, 50, 64, 8), (100, 150, 48, 0), (90, 130, 64, 20), (1080, 1920, 512, 32)]


def _brute_tiles(H, W, tile, pad, mult=14):
    core = max(1, tile - 2 * pad)
    out = []
    y0 = 0
    while y0 < H:
        x0 = 0
        while x0 < W:
            y1, x1 = min(y0 + tile, H), min(x0 + tile, W)
            ya, xa = max(0, y0 - pad), max(0, x0 - pad)
            yb, xb = min(H, y1 + pad), min(W, x1 + pad)
            up = lambda v: -(-v // mult) * mult
            out.append((y0, x0, y1, x1, ya, xa, yb, xb, up(yb - ya), up(xb - xa)))
            x0 += core
        y0 += core
    return out


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_tile_plan_matches_brute_force(geom):
    H, W, tile, pad = geom
    plan = DT.tile_plan(H, W, tile, pad)
    brute = _brute_tiles(H, W, tile, pad)
    got = [(t.y0, t.x0, t.y1, t.x1, t.yp0, t.xp0, t.yp1, t.xp1, t.chs, t.cws) for t in plan.tiles]
    assert got == brute
    assert plan.n_tiles == plan.nty * plan.ntx and plan.core == max(1, tile - 2 * pad)
    for i, t in enumerate(plan.tiles):
        assert t.chs % 14 == 0 and t.cws % 14 == 0
        # the centre slice fits the prediction without the reference's "resize the centre" branch
        assert t.chs >= t.ch >= t.yc0 + t.th and t.cws >= t.cw >= t.xc0 + t.tw
        assert plan.weight_shapes[plan.weight_index[i]] == (t.th, t.tw)
    # a tile is clipped by the frame's edge only while its origin is closer than `tile` to it: <= MAX_COVER distinct sizes per axis
    assert len({s[0] for s in plan.weight_shapes}) <= DT.MAX_COVER and len({s[1] for s in plan.weight_shapes}) <= DT.MAX_COVER
    # groups partition the tiles by crop shape, ascending inside a group
    seen = sorted(i for g in plan.groups for i in g.tiles)
    assert seen == list(range(plan.n_tiles))
    for g in plan.groups:
        assert list(g.tiles) == sorted(g.tiles)
        assert all((plan.tiles[i].ch, plan.tiles[i].cw, plan.tiles[i].chs, plan.tiles[i].cws) == (g.ch, g.cw, g.chs, g.cws) for i in g.tiles)
    # analytic cover range == brute-force cover, both axes, row-major order
    for axis, n, nt in ((0, H, plan.nty), (1, W, plan.ntx)):
        for p in range(n):
            if axis == 0:
                cov = [ty for ty in range(nt) if plan.tiles[ty * plan.ntx].y0 <= p < plan.tiles[ty * plan.ntx].y1]
            else:
                cov = [tx for tx in range(nt) if plan.tiles[tx].x0 <= p < plan.tiles[tx].x1]
            lo, hi = plan.cover(p, axis)
            assert cov == list(range(lo, hi + 1)), (axis, p)
            assert len(cov) <= DT.MAX_COVER


def test_tile_plan_known_counts():
    p = DT.tile_plan(1080, 1920, 512, 32)
    assert p.n_tiles == 15 and len(p.groups) == 9
    p = DT.tile_plan(256, 320, 128, 16)
    assert p.n_tiles == 12 and len(p.groups) == 9
    p = DT.tile_plan(90, 130, 64, 20)
    assert max(p.cover(y, 0)[1] - p.cover(y, 0)[0] + 1 for y in range(90)) == 3
    assert DT.tile_plan(40, 50, 64, 8).nty == 1


@pytest.mark.parametrize("geom", GEOMETRIES[:5] + [(256, 320, 128, 16)])
def test_blend_tables_address_disjoint_planes(geom):
    H, W, tile, pad = geom
    plan = DT.tile_plan(H, W, tile, pad)
    shapes = [(g.chs, g.cws) if k % 2 else (g.chs // 2, g.cws // 2) for k, g in enumerate(plan.groups)]
    tab, off, total = plan.blend_tables(2, shapes)
    assert tab.shape == (plan.n_tiles, 8) and tab.dtype == np.int32 and off.dtype == np.int64 and off.shape == (2 * plan.n_tiles,)
    used = np.zeros(total, np.int32)
    for b in range(2):
        for t in range(plan.n_tiles):
            ph, pw = tab[t, 4], tab[t, 5]
            used[off[b * plan.n_tiles + t]: off[b * plan.n_tiles + t] + ph * pw] += 1
    assert np.all(used == 1)
    wp = plan.weight_pool()
    for t, tl in enumerate(plan.tiles):
        assert tab[t, 6] + tl.th * tl.tw <= wp.size
        assert np.array_equal(wp[tab[t, 6]: tab[t, 6] + tl.th * tl.tw].reshape(tl.th, tl.tw), DT.hann_tile_weight(plan.core, tl.th, tl.tw))
    for g in plan.groups:
        o = plan.gather_origins(g, 2)
        assert o.shape == (2 * len(g.tiles), 3) and o.dtype == np.int32
        assert np.all(o[:, 1] + g.ch <= H) and np.all(o[:, 2] + g.cw <= W) and np.all(o >= 0)


def _cubic_f64(src, dh, dw):
    """The same convolution (same float32 coordinate map, same clamped taps) with coefficients and sums in float64."""
    def axis(d, s):
        scale = 1.0 / (float(d) / float(s))
        f = ((np.arange(d, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
        i = np.floor(f).astype(np.int64)
        f = (f - i.astype(np.float32)).astype(np.float64)
        A = -0.75
        c = np.stack([((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A, ((A + 2) * f - (A + 3)) * f * f + 1,
                      ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1], 1)
        c = np.concatenate([c, 1 - c.sum(1, keepdims=True)], 1)
        return np.clip(i[:, None] + np.arange(-1, 3)[None], 0, s - 1), c
    ox, cx = axis(dw, src.shape[1])
    oy, cy = axis(dh, src.shape[0])
    s = src.astype(np.float64)
    rows = sum(s[:, ox[:, k]] * cx[None, :, k] for k in range(4))
    return sum(rows[oy[:, k], :] * cy[:, k, None] for k in range(4))


# Worst-case float32 error of the restatement against exact arithmetic, in u = 2^-24 = one ulp of the plane's maximum (which lies in [0.5, 1)):
# Horner evaluation of the coefficients with intermediates up to |8A| = 6 costs <= 36 u (outer taps), 8 - 9 u (inner taps) and 55 u for the
# fourth (1 - w0 - w1 - w2 inherits the other three), 108 u for the four together; a pass of |src| <= 1 adds that plus 7 roundings of
# magnitude <= 1.25 (7 u): 115 u after the horizontal pass; the vertical pass sees rows up to 1.25 and an input error of 115 u under a
# kernel of absolute sum <= 1.25: 108 * 1.25 + 1.25 * 115 + 7 = 286 u.  Measured on the shapes below: 3.0 u at most (printed per case).
HANN_BAR_ULPS = 286.0


@pytest.mark.parametrize("core,h,w", [(48, 64, 64), (48, 64, 32), (48, 56, 64), (48, 8, 40), (96, 128, 128), (24, 64, 2), (448, 512, 512), (448, 184, 128)])
def test_hann_tile_weight_vs_float64_convolution(core, h, w):
    got = DT.hann_tile_weight(core, h, w)
    assert got.dtype == np.float32 and got.shape == (h, w) and not got.flags.writeable
    assert DT.hann_tile_weight(core, h, w) is got                       # cached
    src = np.outer(np.hanning(core), np.hanning(core)).astype(np.float32)
    src = src / np.float32(float(src.max()) + 1e-8)
    exp = _cubic_f64(src, h, w)
    ulp = float(np.spacing(np.float32(np.abs(got).max())))
    err = float(np.abs(got.astype(np.float64) - exp).max()) / ulp
    print(f"hann_tile_weight({core},{h},{w}): max |f32 - f64| = {err:.2f} ulp(max)")
    assert err <= HANN_BAR_ULPS
    # up-scaled window (every full tile with pad > 0): the source is zero at its rim and the cubic resize leaves the edges at or below zero
    # (the four corner samples are products of two such values: tiny and positive)
    if h > core and w > core:
        for rim in (got[0], got[-1], got[:, 0], got[:, -1]):
            assert rim[1:-1].max() <= 0 and rim[len(rim) // 2] < 0
    if min(h, w) >= 8:
        assert 0.9 < got.max() < 1.01          # cubic overshoot of a maximum of 1 stays below a percent


def test_hann_tile_weight_same_shape_is_the_window():
    w = DT.hann_tile_weight(48, 48, 48)
    m = np.outer(np.hanning(48), np.hanning(48)).astype(np.float32)
    assert np.array_equal(w, m / np.float32(float(m.max()) + 1e-8))


def test_degenerate_weight_share_small_geometry():
    """Pixels whose accumulated weight is <= 1e-8 (one covering tile, window rim): 0.70 % at 256 x 320, tile 128, pad 16 -- under the
    1 % the percentile clip absorbs."""
    plan = DT.tile_plan(256, 320, 128, 16)
    wacc = np.zeros((256, 320), np.float32)
    for t in plan.tiles:
        wacc[t.y0:t.y1, t.x0:t.x1] += DT.hann_tile_weight(plan.core, t.th, t.tw)
    share = float((wacc <= 1e-8).mean())
    print("degenerate share", share)
    assert 0.004 < share < 0.009


def test_normalize_to_u8_numpy_three_branches():
    rng = np.random.default_rng(5)
    # 1. percentile clip: outliers beyond the 1 % / 99 % ranks saturate, the bulk spreads over the range
    d = rng.normal(size=(50, 37)).astype(np.float32)
    d.flat[:10] = 1e5
    d.flat[10:20] = -1e5
    d[3, 3], d[4, 4], d[5, 5] = np.nan, np.inf, -np.inf
    u = DT.normalize_to_u8_numpy(d)
    assert u.dtype == np.uint8 and u.shape == d.shape
    assert np.all(u.flat[:10] == 255) and np.all(u.flat[10:20] == 0)
    clean = np.nan_to_num(d, nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = np.percentile(clean, 1.0), np.percentile(clean, 99.0)
    assert lo.dtype == np.float32                                          # float32 arithmetic throughout (numpy 2 promotion)
    exp = (np.clip((clean - lo) / (hi - lo), 0.0, 1.0) * 255.0).astype(np.uint8)
    assert np.array_equal(u, exp)
    assert u[3, 3] == u[4, 4] == u[5, 5] == exp[3, 3]                       # non-finite samples count as 0
    assert np.array_equal(DT.normalize_to_u8_numpy(d, invert=True), 255 - u)
    assert 100 < len(np.unique(u)) <= 256
    # 2. percentiles collapse, min-max does not: a flat plane with a few outliers
    d = np.full((40, 40), 2.0, np.float32)
    d[0, :5] = 3.0
    u = DT.normalize_to_u8_numpy(d)
    assert set(np.unique(u)) == {0, 254}                                   # (1 / (1 + 1e-6)) * 255 truncates to 254
    den = np.float32(1.0 + 1e-6)
    assert u[0, 0] == np.uint8(np.float32(1.0) / den * np.float32(255.0))
    # 3. flat plane: all 128 (127 inverted)
    d = np.full((9, 11), -7.25, np.float32)
    assert np.all(DT.normalize_to_u8_numpy(d) == 128) and np.all(DT.normalize_to_u8_numpy(d, invert=True) == 127)
    assert np.all(DT.normalize_to_u8_numpy(np.full((4, 4), np.nan, np.float32)) == 128)


def test_blend_tiles_numpy_constant_prediction():
    """A constant prediction blends to the constant wherever the weight sum is sound, and to the reference's huge quotient where it is not."""
    plan = DT.tile_plan(61, 200, 64, 8)
    out = DT.blend_tiles_numpy(plan, [np.full((t.th, t.tw), 3.5, np.float32) for t in plan.tiles])
    wacc = np.zeros((61, 200), np.float32)
    for t in plan.tiles:
        wacc[t.y0:t.y1, t.x0:t.x1] += DT.hann_tile_weight(plan.core, t.th, t.tw)
    ok = wacc > 1e-3
    assert ok.mean() > 0.9 and np.allclose(out[ok], 3.5, rtol=1e-4)
