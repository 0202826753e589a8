"""Clips of the letterbox tests (tests/test_letterbox_host.py, tests/test_hip_letterbox.py): synth content spliced into segments, dark bars of
values 0..3 painted over it (row variance <= 1.25 < the strict detector's 3.0; synth.letterbox_clip's 0..9 bars do not pass it).  Every clip
has a geometry of its own (``geometry(name)``: the height the tracker is built for, the width of its first frames, the frame rate).  Built
once per process; the statement's results on them are cached so that both test files pay for them once."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from visiondepth3d_amd import synth

H, W, FPS = 96, 128, 2          # fps 2: the 3 s cooldown is 6 frames
BARS_P, BARS_Q = (12, 10), (18, 14)   # painted (top, bottom); Q differs from P by 10 >= min_change and stays under int(0.35 * 96) = 33
TALL = (150, 200)               # H = 150: the column plan of the edge densities is two leaves, (0, 72) and (72, 78): a tree and a tail
TALL_P, TALL_Q = (20, 16), (30, 24)   # under int(0.35 * 150) = 52 and inside the scan of int(0.25 * 150) = 37 rows a side
SMALL = (48, 128)               # H < 64: the detector refuses the frame
BARS_CAP = (22, 16)             # detected (20, 14): 34 > max_total = 33, each inside the scan of 24 rows a side
BARS_THIN = (4, 4)              # below min_band = int(0.06 * 96) = 5
BARS_SMALL = (8, 6)             # at 48 rows min_band is 2 and the scan 12 rows: only the size refusal keeps these from being found

_GEOMETRY = {"tall_frame": TALL + (FPS,), "small_frame": SMALL + (FPS,), "size_switch_back": TALL + (FPS,)}


def geometry(name):
    """(H, W, fps) of a clip: the height its tracker is constructed with and the size of the frames its bootstrap sees"""
    return _GEOMETRY.get(name, (H, W, FPS))


def paint_bars(frame, t, top, bottom):
    f = frame.copy()
    h, w = f.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    bar = ((3 * x + y + 5 * t) % 4).astype(np.uint8)
    m = (y < top) | (y >= h - bottom)
    f[m] = bar[m][:, None]
    return f


def segment(start, n, bars, t0=0, mirror=False, hw=(H, W)):
    """n synth frames from index ``start`` (mirrored left-right on request: another scene of the same generator) with ``bars`` painted"""
    frames, _ = synth.synth_clip(n, hw[0], hw[1], start=start)
    if mirror:
        frames = [np.ascontiguousarray(f[:, ::-1]) for f in frames]
    return [paint_bars(f, t0 + i, *bars) if bars != (0, 0) else f for i, f in enumerate(frames)]


def dim(frame, num, den):
    return ((frame.astype(np.int32) * num) // den).astype(np.uint8)


# scene starts far apart in the generator's time, alternately mirrored: every splice is a hard cut
_SCENES = ((0, False), (400, True), (910, False), (1370, True), (1800, False), (2300, True), (2750, False))


def _scene(k, n, bars, t0, hw=(H, W)):
    s, m = _SCENES[k]
    return segment(s, n, bars, t0, m, hw)


def clip(name):
    """(the frames the bootstrap samples, update frames).  Every update clip starts with 6 frames of the bootstrap scene (the cooldown
    runs out)."""
    from visiondepth3d_amd.letterbox import sample_indices
    head, upd = source(name)
    return [head[i] for i in sample_indices(len(head), geometry(name)[2])], upd


def batches(frames, n=None):
    """``frames`` in runs of at most ``n`` (None: as many as there are) that never span a change of frame size: a device batch has one size"""
    out, i = [], 0
    while i < len(frames):
        j = i + 1
        while j < len(frames) and frames[j].shape == frames[i].shape and (n is None or j - i < n):
            j += 1
        out.append(frames[i:j])
        i = j
    return out


def _fade(s):
    """a fade to black and back inside one scene (``s``: 7 consecutive frames of it)"""
    return [s[0], dim(s[1], 1, 2), dim(s[2], 1, 16), dim(s[3], 0, 1), dim(s[4], 1, 16), s[5], s[6]]


def dark_title(hw=TALL, rows=12):
    """A black frame with a band of bright stripes over its last ``rows`` rows, 49 edge pixels in each of them.  At 150 x 200 and 12 rows the
    mean edge density is 639 / 30000 = 0.0213, just above the near-black gate's 0.02, and any single one of those rows less puts it below
    (590 / 30000 = 0.0197): the frame is a scene cut only if the sum over the rows misses none of them -- the last six are the scalar tail
    of the column plan's second leaf."""
    f = np.zeros(hw + (3,), np.uint8)
    f[hw[0] - rows:, np.arange(hw[1]) % 8 < 4] = 60
    return f


def _three_cuts(bars, hw=(H, W), scenes=(1, 2, 3), t0=20):
    """three scenes after one another, each a hard cut from the one before, all with ``bars``: 2, 2 and 3 frames"""
    return _scene(scenes[0], 2, bars, t0, hw) + _scene(scenes[1], 2, bars, t0 + 10, hw) + _scene(scenes[2], 3, bars, t0 + 20, hw)


@lru_cache(maxsize=None)
def source(name):
    """(the first 9 frames of the clip, which the bootstrap probes at 2 fps: 6 samples; the frames that go through update)"""
    boot = _scene(0, 9, BARS_P, 0)
    lead = _scene(0, 15, BARS_P, 0)[9:]
    if name == "fade":        # a fade to black and back inside one scene, then a cut to another scene with the same bars
        upd = lead + _fade(_scene(0, 24, BARS_P, 0)[15:]) + _scene(1, 2, BARS_P, 30)
    elif name == "three_cuts":
        upd = lead + _three_cuts(BARS_Q)
    elif name == "two_cuts":
        upd = lead + _scene(1, 2, BARS_Q, 20) + _scene(2, 4, BARS_Q, 30)
    elif name == "streak_reset":   # Q, Q, then a cut that shows the locked bars again (change < 8), then Q, Q: no switch; a third Q switches
        upd = (lead + _scene(1, 2, BARS_Q, 20) + _scene(2, 2, BARS_Q, 30) + _scene(3, 2, BARS_P, 40) + _scene(4, 2, BARS_Q, 50) +
               _scene(5, 2, BARS_Q, 60) + _scene(6, 2, BARS_Q, 70))
    elif name == "no_bars":       # a clip without bars: bootstrap stays at zero, cuts do not invent bars; the dimmed frame is a cut by the
        boot = _scene(0, 9, (0, 0), 0)   # histogram alone (MAD about 19, correlation about 0.5), and so is the frame after it
        s = _scene(2, 4, (0, 0), 0)
        upd = _scene(0, 15, (0, 0), 0)[9:] + _scene(1, 2, (0, 0), 0) + [s[0], s[1], dim(s[2], 7, 8), s[3]]
    elif name == "tall_frame":    # 150 x 200: the fade; two cuts to Q; a dark frame that is NOT near-black by its last rows' edges, so it is a cut,
        boot = _scene(0, 9, TALL_P, 0, TALL)   # shows other bars and takes the streak back to 1; three more cuts to Q switch (frame 22, not 18)
        upd = (_scene(0, 15, TALL_P, 0, TALL)[9:] + _fade(_scene(0, 24, TALL_P, 0, TALL)[15:]) + _scene(3, 2, TALL_Q, 30, TALL) +
               _scene(1, 2, TALL_Q, 40, TALL) + [dark_title()] + _three_cuts(TALL_Q, TALL, scenes=(2, 4, 6), t0=50))   # splices that stay cuts under Q
    elif name == "bars_appear":   # locked_zero, then three agreeing cuts with bars: locked_bars
        boot = _scene(0, 9, (0, 0), 0)
        upd = _scene(0, 15, (0, 0), 0)[9:] + _three_cuts(BARS_P)
    elif name == "bars_vanish":   # locked_bars, then three agreeing cuts without: locked_zero
        upd = lead + _three_cuts((0, 0))
    elif name == "over_cap":      # three agreeing cuts whose bars sum above max_total: each counts as (0, 0), and that is what gets locked
        upd = lead + _three_cuts(BARS_CAP)
    elif name == "thin_bars":     # bars thinner than min_band, from the first frame on: nothing ever locks
        boot = _scene(0, 9, BARS_THIN, 0)
        upd = _scene(0, 15, BARS_THIN, 0)[9:] + _three_cuts(BARS_THIN)
    elif name == "cooldown":      # a switch to Q at frame 10, cuts back to P at frames 13 and 15 (swallowed by the cooldown), one at 17 (counted)
        upd = lead + _three_cuts(BARS_Q) + _scene(4, 2, BARS_P, 50) + _scene(5, 2, BARS_P, 60) + _scene(6, 2, BARS_P, 70)
    elif name == "size_switch":   # 96 x 128, then 150 x 200: a cut by the frame size alone; two more cuts at the new size switch the bars
        upd = lead + _three_cuts(TALL_P, TALL)
    elif name == "size_switch_back":   # the other way round: the tracker is built for 150 rows, the state's gray plane shrinks
        boot = _scene(0, 9, TALL_P, 0, TALL)
        upd = _scene(0, 15, TALL_P, 0, TALL)[9:] + _three_cuts(BARS_P)
    elif name == "small_frame":   # 48 x 128: H < 64, the detector refuses the frame, so three cuts with plain bars change nothing (bars
        boot = _scene(0, 9, BARS_SMALL, 0, SMALL)   # this large lower the MAD of a splice: the scenes are the ones that stay above 28)
        upd = _scene(0, 15, BARS_SMALL, 0, SMALL)[9:] + _three_cuts(BARS_SMALL, SMALL, scenes=(6, 4, 2))
    else:
        raise KeyError(name)
    return boot, upd


CLIPS = ("fade", "three_cuts", "two_cuts", "streak_reset", "no_bars", "tall_frame", "bars_appear", "bars_vanish", "over_cap", "thin_bars",
         "cooldown", "size_switch", "size_switch_back", "small_frame")


@lru_cache(maxsize=None)
def statement_run(name):
    """The numpy tracker on a clip: dict(boot=(top, bottom, (locked_bars, locked_zero)), bars=[(top, bottom)] per frame, gates=[per frame
    dict(near_black, mad, corr)], detect=[per frame what detect_from_stats finds on it], row_ok=[per frame the rows that pass the detector's
    row test], states=[per frame the lock state after it], state=final lock state)"""
    from visiondepth3d_amd import letterbox as lb
    boot, upd = clip(name)
    h, _, fps = geometry(name)
    t = lb.LetterboxTrackerNumpy(h, fps)
    b = t.bootstrap(boot)
    bars, gates, detect, row_ok, states = [], [], [], [], []
    for f in upd:
        bars.append(tuple(int(v) for v in t.update(f)))
        gates.append(dict(t.last))
        st = t.prev
        detect.append(lb.detect_from_stats(st))
        edge = lb.edge_density_from_counts(st["edge_counts"], st["w"])
        row_ok.append((st["row_mean"] < lb.Y_THRESH) & (st["row_var"] < np.float32(lb.VAR_THRESH)) & (st["row_sat"] < np.float32(lb.SAT_THRESH)) &
                      (edge <= lb.EDGE_MAX))
        states.append(t.state())
    return dict(boot=b, bars=bars, gates=gates, detect=detect, row_ok=row_ok, states=states, state=t.state())


def cuts(name):
    """[(frame, cooldown while the frame was judged)] of the frames of a clip that the statement takes for a scene cut"""
    from visiondepth3d_amd import letterbox as lb
    r, (_, upd) = statement_run(name), clip(name)
    out, cd = [], int(geometry(name)[2] * 3.0)
    for i, g in enumerate(r["gates"]):
        cd = max(cd - 1, 0)
        if g["mad"] is None:
            cut = i > 0 and not g["near_black"] and upd[i].shape != upd[i - 1].shape
        else:
            cut = g["mad"] > lb.MAD_THRESH or g["corr"] < lb.CORR_THRESH
        if cut:
            out.append((i, cd))
        cd = r["states"][i]["cooldown"]
    return out


# ---- Canny planes that decide a tie ------------------------------------------------------------------------------------------------------
CANNY_SIZES = [(1, 1), (1, 7), (7, 1), (2, 9), (5, 300), (16, 64), (17, 65), (33, 129)]   # below a 64 x 16 tile, one tile, one pixel past it, several


def tie_plane(h, w):
    """Blocks (4 x 4 where the plane has room, down to one pixel where it has not) of the levels {0, 60, 120, 180}: across a step between two
    blocks both pixels carry the same gradient magnitude, so the non-maximum test has to decide a tie -- and OpenCV's is asymmetric (> towards
    one neighbour, >= towards the other)."""
    bh, bw = min(4, max(1, h // 2)), min(4, max(1, w // 2))
    lv = np.random.default_rng(h * 1000 + w + 7).integers(0, 4, ((h + bh - 1) // bh, (w + bw - 1) // bw))
    return (np.repeat(np.repeat(lv, bh, 0), bw, 1)[:h, :w] * 60).astype(np.uint8)
