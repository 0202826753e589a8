"""Letterbox handling of the depth pass (core/render_depth.py:280-573,1919-1933): the per-frame bar tracker and the bar fill behind the
hand-off.  Same role as depth_tiles.py: plain-numpy statements of the reference functions, written from their semantics, that the device
kernels (csrc/vd3d_letterbox.hip) reproduce bit for bit, plus the device tracker ``LetterboxTracker``.

What is pinned and what is not.  The numpy parts of the reference are reproduced exactly, in numpy's own order: the float32 luma
``0.2126*r + 0.7152*g + 0.0722*b`` (three products, two adds, left to right), ``mean`` / ``var`` in numpy's PAIRWISE float32 summation
(``pairwise_sum``, restated below as scalar code so that the kernel has an order to follow), the exact integer sums.  The cv2 parts
(BGR2GRAY, BGR2HSV's S, Canny, calcHist / normalize / compareHist, INTER_CUBIC) are restated from OpenCV's documented 8-bit behaviour and
marked UNPINNED: cv2 is not available to the build.

Every decision takes a ``stats`` dict (``frame_stats_numpy`` on the host, ``Renderer.letterbox_stats`` + ``Renderer.canny_u8`` on the
device), so the host statement and the device bootstrap share one copy of the rules.
"""
from __future__ import annotations

import numpy as np

# detect_letterbox_strict_robust's defaults (core/render_depth.py:336-344) and the gates around it (:295-297, :387)
Y_THRESH, VAR_THRESH, SAT_THRESH, MAX_SCAN_FRAC, MIN_BAND_FRAC, EDGE_MAX = 16, 3.0, 6.0, 0.25, 0.06, 0.04
BLACK_MEAN, BLACK_EDGE = 18, 0.02
MAD_THRESH, CORR_THRESH = 28.0, 0.60
CANNY_LOW, CANNY_HIGH = 30, 90
_DBL_EPS = float(np.finfo(np.float64).eps)


# ---- numpy's pairwise summation ------------------------------------------------------------------------------------------------------
def pairwise_sum(a, dtype=np.float32):
    """numpy's ``pairwise_sum`` (the inner loop of ``np.add.reduce`` over a contiguous axis) as scalar code: fewer than 8 elements are a
    plain loop; up to 128 use eight strided accumulators combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and a scalar tail; above that
    the range splits at ``n // 2`` rounded down to a multiple of 8.  Every add rounds to ``dtype``."""
    a = np.asarray(a, dtype).reshape(-1)
    t = dtype

    def rec(lo, n):
        if n < 8:
            res = t(0)
            for i in range(n):
                res = t(res + a[lo + i])
            return res
        if n <= 128:
            r = [a[lo + j] for j in range(8)]
            i = 8
            while i < n - (n % 8):
                for j in range(8):
                    r[j] = t(r[j] + a[lo + i + j])
                i += 8
            res = t(t(t(r[0] + r[1]) + t(r[2] + r[3])) + t(t(r[4] + r[5]) + t(r[6] + r[7])))
            while i < n:
                res = t(res + a[lo + i])
                i += 1
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return t(rec(lo, n2) + rec(lo + n2, n - n2))

    return rec(0, a.size)


def pairwise_plan(n: int):
    """The tree ``pairwise_sum`` walks for ``n`` elements, flattened: leaves [(offset, length)] in order and the combine steps
    [(dst, left, right)] over value slots (leaf i is slot i), children before parents.  The device builds the same plan.  A row, a column and
    a reduction buffer are at most 8192 elements here: one pairwise sum each."""
    leaves, comb = [], []

    def rec(lo, m):
        if m <= 128:
            leaves.append((lo, m))
            return -len(leaves)          # leaf k as -(k + 1) until the leaf count is known
        m2 = m // 2
        m2 -= m2 % 8
        left, right = rec(lo, m2), rec(lo + m2, m - m2)
        comb.append([len(comb), left, right])
        return len(comb) - 1

    rec(0, int(n))
    nl = len(leaves)
    fix = lambda v: -v - 1 if v < 0 else nl + v
    return leaves, [(nl + d, fix(a), fix(b)) for d, a, b in comb]


def _rows_pairwise_f32(y):
    """pairwise float32 sum of every row of ``y`` [H,W], vectorised over the rows (same order as ``pairwise_sum`` per row)"""
    y = np.ascontiguousarray(y, np.float32)
    leaves, comb = pairwise_plan(y.shape[1])
    slots = np.zeros((y.shape[0], len(leaves) + len(comb)), np.float32)
    for k, (lo, n) in enumerate(leaves):
        slots[:, k] = _leaf_rows(y[:, lo:lo + n])
    for d, a, b in comb:
        slots[:, d] = slots[:, a] + slots[:, b]
    return slots[:, -1].copy()


# ---- colour statistics ---------------------------------------------------------------------------------------------------------------
def bgr2gray_numpy(bgr):
    """cv2.cvtColor(bgr, COLOR_BGR2GRAY) on uint8: (1868 b + 9617 g + 4899 r + 8192) >> 14 -- the statement the DIBR chain already uses
    (csrc/vd3d_kernels.h).  UNPINNED."""
    p = np.asarray(bgr, np.uint8).astype(np.int32)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def hsv_saturation_numpy(bgr):
    """The S channel of cv2.cvtColor(bgr, COLOR_BGR2HSV) on uint8: (diff * sdiv[v] + 2048) >> 12 with v = max, diff = max - min,
    sdiv[0] = 0 and sdiv[v] = round((255 << 12) / v).  UNPINNED."""
    p = np.asarray(bgr, np.uint8).astype(np.int64)
    v = p.max(axis=-1)
    diff = v - p.min(axis=-1)
    sdiv = np.zeros(256, np.int64)
    sdiv[1:] = np.rint((255 << 12) / np.arange(1, 256, dtype=np.float64)).astype(np.int64)
    return ((diff * sdiv[v] + 2048) >> 12).astype(np.uint8)


def luma_saturation_numpy(bgr):
    """_luma_saturation (:280-292): float32 Rec.709 luma (numpy's own arithmetic: pinned) and the HSV saturation as float32 (UNPINNED
    through ``hsv_saturation_numpy``)."""
    f = np.asarray(bgr, np.uint8)
    b, g, r = (f[..., c].astype(np.float32) for c in range(3))
    y = np.float32(0.2126) * r + np.float32(0.7152) * g + np.float32(0.0722) * b
    return y, hsv_saturation_numpy(f).astype(np.float32)


def row_uniformity_numpy(bgr):
    """_row_uniformity_metrics (:322-328): per-row luma mean and variance and saturation mean, float32, in numpy's pairwise order
    (restated, not called: tests/test_letterbox_host.py holds the restatement against numpy itself)."""
    y, s = luma_saturation_numpy(bgr)
    w = np.float32(y.shape[1])
    mean = _rows_pairwise_f32(y) / w
    d = y - mean[:, None]
    var = _rows_pairwise_f32(d * d) / w
    s_sum = s.astype(np.int64).sum(axis=1)              # integers below 2^24: any order is exact
    return mean, var, s_sum.astype(np.float32) / w


NUMPY_BUFSIZE = 8192   # np.getbufsize(): elements per inner-loop call of a reduction over more than that


def luma_mean_numpy(y):
    """``y.mean()`` of the float32 luma plane: numpy reduces the contiguous plane as ONE run of H*W elements, handed to the inner loop in
    buffers of 8192 -- every buffer is a pairwise sum of its own and the buffers' sums are added up in order (held against numpy itself in
    tests/test_letterbox_host.py: a single pairwise sum over H*W is NOT what numpy computes above 8192 elements)."""
    flat = np.ascontiguousarray(y, np.float32).reshape(-1)
    nfull = flat.size // NUMPY_BUFSIZE
    sums = list(_rows_pairwise_f32(flat[:nfull * NUMPY_BUFSIZE].reshape(nfull, NUMPY_BUFSIZE))) if nfull else []
    if flat.size > nfull * NUMPY_BUFSIZE:
        sums.append(_rows_pairwise_f32(flat[None, nfull * NUMPY_BUFSIZE:])[0])
    acc = np.float32(0)
    for v in sums:
        acc = np.float32(acc + v)
    return np.float32(acc / np.float32(flat.size))


def _leaf_rows(blk):
    """one leaf (at most 128 elements) of the pairwise sum, for every row of ``blk`` at once"""
    n = blk.shape[1]
    if n < 8:
        res = np.zeros(blk.shape[0], np.float32)
        for i in range(n):
            res = res + blk[:, i]
        return res
    r = [blk[:, j].copy() for j in range(8)]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] = r[j] + blk[:, i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + blk[:, i]
        i += 1
    return res


# ---- Canny ---------------------------------------------------------------------------------------------------------------------------
def canny_classes_numpy(gray, low=CANNY_LOW, high=CANNY_HIGH):
    """First half of ``canny_numpy``: the class map (0 none, 1 weak candidate, 2 strong candidate) after Sobel, squared L2 magnitude
    and the directional non-maximum test.  UNPINNED."""
    g = np.asarray(gray, np.uint8).astype(np.int32)
    h, w = g.shape
    p = np.pad(g, 1, mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    mag = dx * dx + dy * dy
    m = np.pad(mag, 1)                                                  # magnitude counts as 0 outside the image
    c, up, dn = m[1:-1, 1:-1], m[:-2], m[2:]
    left, right = m[1:-1, :-2], m[1:-1, 2:]
    lo2, hi2 = int(low) * int(low), int(high) * int(high)
    x, y = np.abs(dx).astype(np.int64), np.abs(dy).astype(np.int64) << 15
    t = 13573 * x
    horiz = y < t
    vert = ~horiz & (y > t + (x << 16))
    neg = (dx ^ dy) < 0                                                 # s = -1: up-right and down-left
    d_up = np.where(neg, up[:, 2:], up[:, :-2])
    d_dn = np.where(neg, dn[:, :-2], dn[:, 2:])
    keep = np.where(horiz, (c > left) & (c >= right), np.where(vert, (c > up[:, 1:-1]) & (c >= dn[:, 1:-1]), (c > d_up) & (c > d_dn)))
    cand = keep & (c > lo2)
    return (cand.astype(np.uint8) + (cand & (c > hi2)).astype(np.uint8))


def hysteresis_numpy(classes):
    """Second half: 255 on every candidate that is 8-connected, through candidates, to a strong one (scipy's labelling; the edge set is
    unique, whatever the schedule)."""
    from scipy import ndimage
    cls = np.asarray(classes, np.uint8)
    lab, n = ndimage.label(cls > 0, structure=np.ones((3, 3), int))
    good = np.zeros(n + 1, bool)
    good[np.unique(lab[cls == 2])] = True
    good[0] = False
    return np.where(good[lab], 255, 0).astype(np.uint8)


def canny_numpy(gray, low=CANNY_LOW, high=CANNY_HIGH):
    """cv2.Canny(gray, low, high, apertureSize=3, L2gradient=True) on uint8: 3 x 3 Sobel with a replicated border, squared magnitude
    against squared thresholds, OpenCV's integer direction test (tan 22.5 = 13573 / 2^15), hysteresis.  UNPINNED."""
    return hysteresis_numpy(canny_classes_numpy(gray, low, high))


def edge_density_numpy(gray, low=CANNY_LOW, high=CANNY_HIGH):
    """_horizontal_edge_density (:330-334): edges.mean(axis=1) / 255.0 in float64 = ((255 * count) / W) / 255.0"""
    return edge_density_from_counts(np.count_nonzero(canny_numpy(gray, low, high), axis=1), np.asarray(gray).shape[1])


def edge_density_from_counts(counts, w):
    return ((255.0 * np.asarray(counts, np.float64)) / float(w)) / 255.0


# ---- histogram comparison -----------------------------------------------------------------------------------------------------------
def hist64_numpy(gray):
    """cv2.calcHist([gray], [0], None, [64], [0, 256]): bin = v >> 2.  UNPINNED."""
    return np.bincount(np.asarray(gray, np.uint8).reshape(-1) >> 2, minlength=64).astype(np.int64)


def hist_normalize_numpy(h):
    """cv2.normalize(h, h) of a histogram (NORM_L2, alpha 1): the norm and 1 / norm in float64 (the sum under the root is an exact integer
    below 2^53), every bin scaled in float64 and stored as float32.  UNPINNED."""
    h = np.asarray(h, np.float64).reshape(-1)
    n = float(np.sqrt(float((h * h).sum())))
    scale = 1.0 / n if n > _DBL_EPS else 0.0
    return (h * scale).astype(np.float32)


def hist_correl_numpy(a, b):
    """cv2.compareHist(a, b, HISTCMP_CORREL) on float32 histograms: float64 running sums over the bins in order, 1 when the squared
    denominator is at most DBL_EPSILON.  UNPINNED."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    s1 = s2 = s11 = s22 = s12 = 0.0
    for i in range(a.size):
        x, y = float(a[i]), float(b[i])
        s1 += x; s2 += y; s11 += x * x; s22 += y * y; s12 += x * y
    scale = 1.0 / a.size
    num = s12 - s1 * s2 * scale
    den2 = (s11 - s1 * s1 * scale) * (s22 - s2 * s2 * scale)
    return num / float(np.sqrt(den2)) if abs(den2) > _DBL_EPS else 1.0


def hist_correlation(h1, h2):
    """is_scene_cut's secondary check (:314-318) on two 64-bin count histograms"""
    return hist_correl_numpy(hist_normalize_numpy(h1), hist_normalize_numpy(h2))


# ---- per-frame statistics and the decisions on them -------------------------------------------------------------------------------
def frame_stats_numpy(bgr, prev_gray=None):
    """Everything the tracker reads from one frame: what ``Renderer.letterbox_stats`` + ``canny_u8`` give per frame on the device."""
    f = np.asarray(bgr, np.uint8)
    y, _ = luma_saturation_numpy(f)
    mean, var, sat = row_uniformity_numpy(f)
    gray = bgr2gray_numpy(f)
    counts = np.count_nonzero(canny_numpy(gray), axis=1)
    st = dict(h=f.shape[0], w=f.shape[1], row_mean=mean, row_var=var, row_sat=sat, gray=gray, hist=hist64_numpy(gray), edge_counts=counts,
              frame_mean=luma_mean_numpy(y), mad_sum=None)
    if prev_gray is not None and prev_gray.shape == gray.shape:
        st["mad_sum"] = int(np.abs(prev_gray.astype(np.int64) - gray.astype(np.int64)).sum())
    return st


def _edge_mean(st):
    e = edge_density_from_counts(st["edge_counts"], st["w"])
    return float(pairwise_sum(e, np.float64) / np.float64(e.size))


def near_black_from_stats(st) -> bool:
    return bool(float(st["frame_mean"]) < BLACK_MEAN and _edge_mean(st) < BLACK_EDGE)


def scene_cut_metrics(st, prev):
    """(mad, corr) of a frame against the previous one; mad is None when the shapes differ (a cut), corr is computed only when the
    reference would compute it (mad <= threshold)"""
    if (prev["h"], prev["w"]) != (st["h"], st["w"]):
        return None, None
    mad = st["mad_sum"] / float(st["h"] * st["w"])
    return mad, (None if mad > MAD_THRESH else hist_correlation(prev["hist"], st["hist"]))


def scene_cut_from_stats(st, prev) -> bool:
    if prev is None:
        return False
    mad, corr = scene_cut_metrics(st, prev)
    return True if mad is None or mad > MAD_THRESH else bool(corr < CORR_THRESH)


def detect_from_stats(st):
    """detect_letterbox_strict_robust's row scan (:357-385) on the statistics of one frame"""
    h, w = st["h"], st["w"]
    if h < 64 or w < 64:
        return 0, 0
    edge = edge_density_from_counts(st["edge_counts"], w)
    ok = (st["row_mean"] < Y_THRESH) & (st["row_var"] < np.float32(VAR_THRESH)) & (st["row_sat"] < np.float32(SAT_THRESH)) & (edge <= EDGE_MAX)
    scan_h, min_band = int(h * MAX_SCAN_FRAC), int(h * MIN_BAND_FRAC)

    def scan(rows):
        run = 0
        for i in rows:
            if not ok[i]:
                break
            run += 1
        if run < min_band:
            run = 0
        return run - (run % 2)

    top, bot = scan(range(0, scan_h)), scan(range(h - 1, h - 1 - scan_h, -1))
    return (0, 0) if top + bot >= h * 0.6 else (int(top), int(bot))


def is_near_black_numpy(bgr) -> bool:
    """is_near_black_frame (:387-392)"""
    return near_black_from_stats(frame_stats_numpy(bgr))


def is_scene_cut_numpy(prev_gray, gray) -> bool:
    """is_scene_cut (:295-319) on two gray planes"""
    if prev_gray is None or gray is None:
        return False
    if prev_gray.shape != gray.shape:
        return True
    mad = float(np.abs(prev_gray.astype(np.int64) - gray.astype(np.int64)).sum()) / float(gray.size)
    return True if mad > MAD_THRESH else bool(hist_correlation(hist64_numpy(prev_gray), hist64_numpy(gray)) < CORR_THRESH)


def detect_letterbox_strict_robust_numpy(bgr):
    """detect_letterbox_strict_robust (:336-385) with its default thresholds"""
    return detect_from_stats(frame_stats_numpy(bgr))


def confidence_from_stats(stats, h, prev_of=None):
    """detect_letterbox_multiframe_confidence (:394-455) on the statistics of the sampled frames, in order: black frames and cuts are
    skipped, the medians are made even, the confidence is the share of samples within 4 px of both medians."""
    tops, bots, prev = [], [], None
    for st in stats:
        skip = near_black_from_stats(st) or scene_cut_from_stats(st, prev)
        prev = st
        if skip:
            continue
        t, b = detect_from_stats(st)
        if 0 <= t < h and 0 <= b < h and t + b < h:
            tops.append(t)
            bots.append(b)
    if not tops:
        return (0, 0), 0.0
    tm, bm = int(np.median(tops)), int(np.median(bots))
    tm, bm = max(tm - tm % 2, 0), max(bm - bm % 2, 0)
    if tm + bm >= h * 0.6:
        return (0, 0), 0.0
    agree = sum(1 for t, b in zip(tops, bots) if abs(t - tm) <= 4 and abs(b - bm) <= 4)
    return (tm, bm), float(agree / max(1, len(tops)))


def sample_indices(total: int, fps, max_seconds=3, samples=9):
    """The frame numbers the reference's bootstrap probes (:407-414)"""
    window = max(min(int(total), int((fps if fps and fps > 0 else 30) * max_seconds)), 1)
    return np.linspace(0, max(0, window - 1), num=min(samples, window), dtype=int)


def multiframe_confidence_numpy(frames, h):
    """((top, bottom), confidence) from the sampled frames (already picked with ``sample_indices``)"""
    stats, prev_gray = [], None
    for f in frames:
        st = frame_stats_numpy(f, prev_gray)
        prev_gray = st["gray"]
        stats.append(st)
    return confidence_from_stats(stats, int(h))


# ---- tracker ---------------------------------------------------------------------------------------------------------------------------
class _TrackerRules:
    """Constructor arguments, defaults and lock state of the reference's LetterboxTracker (:458-494)"""

    def __init__(self, h, fps, min_change=8, confirm_needed=3, max_total_frac=0.35, conf_enable=0.7, conf_disable=0.6, cooldown_sec=3.0):
        self.h = int(h)
        self.fps = float(fps) if fps and fps > 0 else 30.0
        self.min_change, self.confirm_needed = int(min_change), int(confirm_needed)
        self.max_total_frac, self.conf_enable, self.conf_disable = float(max_total_frac), float(conf_enable), float(conf_disable)
        self.cooldown_frames = int(self.fps * cooldown_sec)
        self.max_total = int(self.h * self.max_total_frac)
        self.top = self.bot = 0
        self.locked_zero, self.locked_bars = True, False
        self._cand, self._streak, self._cooldown = (0, 0), 0, 0

    def _apply_bootstrap(self, tb, conf):
        t, b = tb
        if conf >= self.conf_enable and t + b > 0:
            self.top, self.bot, self.locked_bars, self.locked_zero = int(t), int(b), True, False
        else:
            self.top, self.bot, self.locked_bars, self.locked_zero = 0, 0, False, True
        self._cooldown = self.cooldown_frames
        return self.top, self.bot, (self.locked_bars, self.locked_zero)

    def _scalars(self):
        return dict(top=self.top, bottom=self.bot, locked_zero=int(self.locked_zero), locked_bars=int(self.locked_bars), cand_top=int(self._cand[0]),
                    cand_bottom=int(self._cand[1]), streak=self._streak, cooldown=self._cooldown)


class LetterboxTrackerNumpy(_TrackerRules):
    """The reference's LetterboxTracker (:458-573) on the numpy statements: ``bootstrap(frames)`` takes the sampled frames,
    ``update(frame)`` one frame and returns (top, bottom).  ``last`` keeps the gate values of the latest update (near_black, mad, corr)."""

    def __init__(self, h, fps, **kw):
        super().__init__(h, fps, **kw)
        self.prev = None
        self.last = {}

    def bootstrap(self, frames):
        return self._apply_bootstrap(*multiframe_confidence_numpy(frames, self.h))

    def update(self, frame):
        if self._cooldown > 0:
            self._cooldown -= 1
        st = frame_stats_numpy(frame, None if self.prev is None else self.prev["gray"])
        prev, self.prev = self.prev, st
        self.last = dict(near_black=near_black_from_stats(st), mad=None, corr=None)
        if self.last["near_black"]:
            return self.top, self.bot
        if prev is not None:
            self.last["mad"], self.last["corr"] = scene_cut_metrics(st, prev)
        if not scene_cut_from_stats(st, prev) or self._cooldown > 0:
            return self.top, self.bot
        mt, mb = detect_from_stats(st)
        if mt + mb > self.max_total:
            mt, mb = 0, 0
        mt, mb = max(mt - mt % 2, 0), max(mb - mb % 2, 0)
        if abs(mt - self.top) + abs(mb - self.bot) < self.min_change:
            self._streak, self._cand = 0, (self.top, self.bot)
            return self.top, self.bot
        if (mt, mb) == self._cand:
            self._streak += 1
        else:
            self._cand, self._streak = (mt, mb), 1
        if self._streak >= self.confirm_needed:
            if self.locked_zero and mt + mb > 0:
                self.top, self.bot, self.locked_zero, self.locked_bars = mt, mb, False, True
                self._cooldown = self.cooldown_frames
            elif self.locked_bars:
                self.top, self.bot = mt, mb
                self.locked_zero, self.locked_bars = mt + mb == 0, mt + mb > 0
                self._cooldown = self.cooldown_frames
        return self.top, self.bot

    def state(self):
        return self._scalars()


# ---- bar fill ------------------------------------------------------------------------------------------------------------------------
def resize_cubic_u8_numpy(src, dh: int, dw: int):
    """cv2.resize(src, (dw, dh), interpolation=cv2.INTER_CUBIC) on a uint8 plane in OpenCV's fixed point (A = -0.75, coefficients rounded to
    11 bits, horizontal then vertical in int32, (sum + 2^21) >> 22, saturate): the project's INTER_CUBIC statement (oracle vo_resize_cubic_u8,
    csrc/vd3d_cubic.h), in numpy.  UNPINNED."""
    from .depth_tiles import _cubic_axis_f32
    s = np.ascontiguousarray(src, np.uint8).astype(np.int32)
    sh, sw = s.shape
    if (sh, sw) == (dh, dw):
        return np.asarray(src, np.uint8).copy()

    def axis(d, n):
        o, c = _cubic_axis_f32(d, n)
        return o, np.clip(np.rint(c * np.float32(2048)), -32768, 32767).astype(np.int32)

    ox, cx = axis(dw, sw)
    oy, cy = axis(dh, sh)
    rows = sum(s[:, ox[:, k]] * cx[None, :, k] for k in range(4))
    out = sum(rows[oy[:, k], :] * cy[:, k, None] for k in range(4))
    return np.clip((out + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def letterbox_fill_numpy(depth_u8, top, bottom):
    """The letterbox handling behind the hand-off (:1919-1933) for one uint8 [H,W] depth plane: the plane squeezed into the picture rows
    with INTER_CUBIC, the bars filled with int(np.median(squeezed)).  No bars: the plane as it is; bars that leave no picture row: the
    reference drops them (the resize to the same size is a copy)."""
    d = np.asarray(depth_u8, np.uint8)
    top, bottom = int(top), int(bottom)
    if not (top or bottom):
        return d.copy()
    h, w = d.shape
    core_h = h - top - bottom
    if core_h <= 0:
        top = bottom = 0
        core_h = h
    core = resize_cubic_u8_numpy(d, core_h, w)
    out = np.full((h, w), int(np.median(core)) if core.size else 0, np.uint8)
    out[top:top + core_h] = core
    return out


# ---- device tracker ------------------------------------------------------------------------------------------------------------------
class LetterboxTracker(_TrackerRules):
    """The tracker on the device: ``update(frames)`` enqueues the statistics pass, Canny and one tracker step for the whole batch on the
    renderer's stream and returns the int32 [B,2] (top, bottom) tensor without a host synchronisation; the lock state lives in the
    renderer's context and constructing a tracker resets it: one tracker per renderer.  ``bootstrap(frames)`` runs once per clip: statistics on the device, medians and confidence on the host."""

    def __init__(self, renderer, h, fps, **kw):
        super().__init__(h, fps, **kw)
        self.renderer = renderer
        renderer.letterbox_state_reset()

    def bootstrap(self, frames_u8):
        import torch
        R = self.renderer
        f = torch.as_tensor(frames_u8).to(R.device)
        st = R.letterbox_stats(f, chain=False)
        counts = R.canny_u8(st["gray"], CANNY_LOW, CANNY_HIGH, want_counts=True)[1].cpu().numpy()
        host = {k: v.cpu().numpy() for k, v in st.items() if k != "gray"}
        S, H, W = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
        stats = [dict(h=H, w=W, row_mean=host["row_mean"][i], row_var=host["row_var"][i], row_sat=host["row_sat"][i].astype(np.float32) / np.float32(W),
                      hist=host["hist"][i].astype(np.int64), edge_counts=counts[i], frame_mean=host["frame_mean"][i],
                      mad_sum=int(host["mad_sum"][i]) if i else None) for i in range(S)]
        res = self._apply_bootstrap(*confidence_from_stats(stats, self.h))
        R.letterbox_state_import(dict(self._scalars(), have_prev=0))
        return res

    def update(self, frames_u8):
        return self.renderer.letterbox_track(frames_u8, self.h, self.min_change, self.confirm_needed, self.max_total, self.cooldown_frames)

    def state(self):
        """The lock state as a dict (synchronises: for inspection and tests)"""
        s = self.renderer.letterbox_state_export()
        self.top, self.bot, self.locked_zero, self.locked_bars = s["top"], s["bottom"], bool(s["locked_zero"]), bool(s["locked_bars"])
        self._cand, self._streak, self._cooldown = (s["cand_top"], s["cand_bottom"]), s["streak"], s["cooldown"]
        return {k: s[k] for k in self._scalars()}
