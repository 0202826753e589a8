"""Host side of the tiled high-resolution depth path (core/render_depth.py:46-48,62-66,102-194): tile geometry, the Hann blend
window and the numpy statement of the percentile hand-off.  Pure numpy, no GPU: the device kernels (csrc/vd3d_tiles.hip) take the
tables built here.

The reference cuts the inference-size frame into ``tile``-pixel tiles on a grid of ``core = max(1, tile - 2*pad)``, crops each
with a ``pad`` apron, resizes the crop so that both sides are multiples of 14, runs the model, cuts the tile's centre out of the
prediction at the UNSCALED crop coordinates (a quirk that is kept) and blends the centres under a Hann window resized to the
tile.  The window is zero at its rim and its cubic resize dips below zero there, so pixels that only one tile covers (first row /
column) get a weight sum <= 1e-8 and a huge quotient; the 1 % - 99 % percentile clip of the hand-off is what absorbs them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

MAX_COVER = 4   # covering tiles per axis the blend kernel is built for (pad <= 3/8 tile)


@dataclass(frozen=True)
class Tile:
    """One tile: target rectangle [y0:y1, x0:x1], apron crop [yp0:yp1, xp0:xp1] (ch x cw), model size chs x cws."""
    y0: int
    x0: int
    y1: int
    x1: int
    yp0: int
    xp0: int
    yp1: int
    xp1: int
    chs: int
    cws: int

    @property
    def ch(self):
        return self.yp1 - self.yp0

    @property
    def cw(self):
        return self.xp1 - self.xp0

    @property
    def yc0(self):
        return self.y0 - self.yp0

    @property
    def xc0(self):
        return self.x0 - self.xp0

    @property
    def th(self):
        return self.y1 - self.y0

    @property
    def tw(self):
        return self.x1 - self.x0


@dataclass(frozen=True)
class TileGroup:
    """Tiles whose crops share one size: one gather launch and one network batch shape."""
    ch: int
    cw: int
    chs: int
    cws: int
    tiles: tuple   # indices into TilePlan.tiles, ascending


@dataclass(frozen=True)
class TilePlan:
    tgt_h: int
    tgt_w: int
    tile: int
    pad: int
    core: int
    nty: int
    ntx: int
    tiles: tuple            # row-major over the (nty, ntx) grid
    groups: tuple           # TileGroup, in order of first appearance
    weight_shapes: tuple    # distinct (y1-y0, x1-x0), in order of first appearance (<= MAX_COVER sizes per axis)
    weight_index: tuple     # per tile: index into weight_shapes
    weight_offsets: tuple = field(default=())   # element offset of each weight plane in the pool

    @property
    def n_tiles(self):
        return len(self.tiles)

    def cover(self, p: int, axis: int):
        """Analytic range (lo, hi), inclusive, of the grid indices along ``axis`` (0 = y, 1 = x) whose tile covers coordinate ``p``:
        t * core <= p < t * core + tile -- what the blend kernel evaluates per pixel."""
        lo = max(0, -((-(p - self.tile + 1)) // self.core))
        return lo, p // self.core

    def gather_origins(self, group: TileGroup, n_frames: int) -> np.ndarray:
        """int32 [n_frames * len(group.tiles), 3] = (frame, yp0, xp0), frame-major: the table of vd3d_tile_gather_cubic_u8."""
        o = [(b, self.tiles[t].yp0, self.tiles[t].xp0) for b in range(n_frames) for t in group.tiles]
        return np.asarray(o, np.int32).reshape(-1, 3)

    def blend_tables(self, n_frames: int, pred_shapes):
        """Tables of vd3d_tile_blend_f32 for predictions stored group after group, frame-major inside a group (the order
        ``gather_origins`` produces), ``pred_shapes[g] = (ph, pw)`` of group g.  Returns (tile_tab int32 [n_tiles, 8], pred_off int64
        [n_frames * n_tiles], pool size in elements)."""
        tab = np.zeros((self.n_tiles, 8), np.int32)
        off = np.zeros((n_frames, self.n_tiles), np.int64)
        base = 0
        for g, (ph, pw) in zip(self.groups, pred_shapes):
            ph, pw = int(ph), int(pw)
            k = len(g.tiles)
            for j, t in enumerate(g.tiles):
                tl = self.tiles[t]
                tab[t] = (tl.yc0, tl.xc0, tl.chs, tl.cws, ph, pw, self.weight_offsets[self.weight_index[t]], 0)
                for b in range(n_frames):
                    off[b, t] = base + (b * k + j) * ph * pw
            base += n_frames * k * ph * pw
        return tab, off.reshape(-1), base

    def weight_pool(self) -> np.ndarray:
        """The distinct weight planes, flattened one after the other (float32)."""
        return np.concatenate([hann_tile_weight(self.core, h, w).reshape(-1) for h, w in self.weight_shapes])


def _round_up(v: int, m: int) -> int:
    return ((int(v) + m - 1) // m) * m


@lru_cache(maxsize=64)
def tile_plan(tgt_h: int, tgt_w: int, tile: int = 512, pad: int = 32, multiple: int = 14) -> TilePlan:
    """Tiles of a ``tgt_h x tgt_w`` inference-size frame in the reference's loop order, their apron crops, the groups of equal crop
    shape and the distinct blend-window shapes."""
    tgt_h, tgt_w, tile, pad, multiple = int(tgt_h), int(tgt_w), int(tile), int(pad), int(multiple)
    if tgt_h < 1 or tgt_w < 1 or tile < 1 or pad < 0 or multiple < 1:
        raise ValueError("tile_plan: sizes must be positive (pad >= 0)")
    core = max(1, tile - 2 * pad)
    tiles, gmap, wshapes, windex = [], {}, [], []
    for y0 in range(0, tgt_h, core):
        for x0 in range(0, tgt_w, core):
            y1, x1 = min(y0 + tile, tgt_h), min(x0 + tile, tgt_w)
            yp0, xp0 = max(0, y0 - pad), max(0, x0 - pad)
            yp1, xp1 = min(tgt_h, y1 + pad), min(tgt_w, x1 + pad)
            t = Tile(y0, x0, y1, x1, yp0, xp0, yp1, xp1, _round_up(yp1 - yp0, multiple), _round_up(xp1 - xp0, multiple))
            gmap.setdefault((t.ch, t.cw, t.chs, t.cws), []).append(len(tiles))
            if (t.th, t.tw) not in wshapes:
                wshapes.append((t.th, t.tw))
            windex.append(wshapes.index((t.th, t.tw)))
            tiles.append(t)
    groups = tuple(TileGroup(*k, tuple(v)) for k, v in gmap.items())
    woff, o = [], 0
    for h, w in wshapes:
        woff.append(o)
        o += h * w
    return TilePlan(tgt_h, tgt_w, tile, pad, core, -(-tgt_h // core), -(-tgt_w // core), tuple(tiles), groups, tuple(wshapes), tuple(windex),
                    tuple(woff))


# ---- Hann window + OpenCV float32 INTER_CUBIC ------------------------------------------------------------------------------------
def _hann2d(n: int) -> np.ndarray:
    """n x n Hann window (at least 2 x 2), float32, scaled by 1 / (max + 1e-8)"""
    h = np.hanning(max(2, n))
    m = np.outer(h, h).astype(np.float32)
    return m / (float(m.max()) + 1e-8)


def _cubic_axis_f32(dsize: int, ssize: int):
    """OpenCV's coordinate map and float32 cubic coefficients (A = -0.75) for every destination index of one axis: source offsets
    [dsize, 4] (clamped into the source: replicate border) and coefficients [dsize, 4] float32."""
    scale = 1.0 / (float(dsize) / float(ssize))                       # cv::resize: inv_scale in double, scale = 1 / inv_scale
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    A, one = np.float32(-0.75), np.float32(1)
    c = np.empty((dsize, 4), np.float32)
    c[:, 0] = ((A * (f + one) - np.float32(5) * A) * (f + one) + np.float32(8) * A) * (f + one) - np.float32(4) * A
    c[:, 1] = ((A + np.float32(2)) * f - (A + np.float32(3))) * f * f + one
    c[:, 2] = ((A + np.float32(2)) * (one - f) - (A + np.float32(3))) * (one - f) * (one - f) + one
    c[:, 3] = one - c[:, 0] - c[:, 1] - c[:, 2]
    o = np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, ssize - 1)
    return o, c


def resize_cubic_f32(src: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """cv2.resize(src, (dw, dh), interpolation=cv2.INTER_CUBIC) on a float32 plane, restated from OpenCV's published algorithm
    (float32 coefficients, horizontal pass then vertical pass, each a left-to-right float32 sum of four products, index clamping at
    the borders).  UNPINNED: cv2 is not available to the build; real builds may contract the sums differently."""
    src = np.ascontiguousarray(src, np.float32)
    sh, sw = src.shape
    if (sh, sw) == (dh, dw):
        return src.copy()
    ox, cx = _cubic_axis_f32(dw, sw)
    oy, cy = _cubic_axis_f32(dh, sh)
    rows = src[:, ox[:, 0]] * cx[None, :, 0]
    for k in range(1, 4):
        rows = rows + src[:, ox[:, k]] * cx[None, :, k]                # [sh, dw] float32
    out = rows[oy[:, 0], :] * cy[:, 0, None]
    for k in range(1, 4):
        out = out + rows[oy[:, k], :] * cy[:, k, None]
    return out.astype(np.float32, copy=False)


@lru_cache(maxsize=64)
def _hann_tile_weight(core: int, h: int, w: int) -> np.ndarray:
    m = _hann2d(core)
    out = m if m.shape == (h, w) else resize_cubic_f32(m, h, w)
    out = np.ascontiguousarray(out, np.float32)
    out.setflags(write=False)
    return out


def hann_tile_weight(core: int, h: int, w: int) -> np.ndarray:
    """Blend weight of an ``h x w`` tile centre: the ``core x core`` Hann window (outer product of np.hanning, float32, divided by
    max + 1e-8), resized with float32 INTER_CUBIC whenever the shapes differ.  Cached per (core, h, w); read-only."""
    return _hann_tile_weight(int(core), int(h), int(w))


# ---- hand-off ----------------------------------------------------------------------------------------------------------------------
def normalize_to_u8_numpy(d, invert: bool = False, pclip=(1.0, 99.0)) -> np.ndarray:
    """The percentile hand-off (core/render_depth.py:173-193) without its final cv2.resize: float32 plane -> uint8 plane.  Non-finite samples
    count as 0; the plane is stretched between its ``pclip`` percentiles (numpy's "linear" method, float32) and clipped; when the percentiles
    are closer than 1e-6 it falls back to min-max (denominator formed from Python floats, i.e. in double), and to 128 everywhere when the
    whole range is below 1e-6 too.  ``* 255`` truncates to uint8."""
    d = np.asarray(d, dtype=np.float32)
    if not np.isfinite(d).all():
        d = np.nan_to_num(d, nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = np.percentile(d, pclip[0]), np.percentile(d, pclip[1])
    if hi - lo >= 1e-6:
        unit = np.clip((d - lo) / (hi - lo), 0.0, 1.0)
    else:
        dmin, dmax = float(d.min()), float(d.max())
        unit = None if dmax - dmin < 1e-6 else (d - dmin) / (dmax - dmin + 1e-6)
    u8 = np.full(d.shape, 128, np.uint8) if unit is None else (unit * 255.0).astype(np.uint8)
    return 255 - u8 if invert else u8


def blend_tiles_numpy(plan: TilePlan, centres) -> np.ndarray:
    """The reference's accumulation for one frame: ``centres[t]`` is the float32 [y1-y0, x1-x0] centre of tile t (row-major)."""
    out = np.zeros((plan.tgt_h, plan.tgt_w), np.float32)
    wacc = np.zeros((plan.tgt_h, plan.tgt_w), np.float32)
    for t, c in zip(plan.tiles, centres):
        w = hann_tile_weight(plan.core, t.th, t.tw)
        out[t.y0:t.y1, t.x0:t.x1] += np.asarray(c, np.float32) * w
        wacc[t.y0:t.y1, t.x0:t.x1] += w
    return (out / np.maximum(wacc, 1e-8)).astype(np.float32, copy=False)
