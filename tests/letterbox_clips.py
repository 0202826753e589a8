"""Clips of the letterbox tests (tests/test_letterbox_host.py, tests/test_hip_letterbox.py): synth content spliced into segments, dark bars of
values 0..3 painted over it (row variance <= 1.25 < the strict detector's 3.0; synth.letterbox_clip's 0..9 bars do not pass it).  Built once
per process; the statement's results on them are cached so that both test files pay for them once."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from visiondepth3d_amd import synth

H, W, FPS = 96, 128, 2          # fps 2: the 3 s cooldown is 6 frames
BARS_P, BARS_Q = (12, 10), (18, 14)   # painted (top, bottom); Q differs from P by 10 >= min_change and stays under int(0.35 * 96) = 33


def paint_bars(frame, t, top, bottom):
    f = frame.copy()
    y, x = np.mgrid[0:H, 0:W]
    bar = ((3 * x + y + 5 * t) % 4).astype(np.uint8)
    m = (y < top) | (y >= H - bottom)
    f[m] = bar[m][:, None]
    return f


def segment(start, n, bars, t0=0, mirror=False):
    """n synth frames from index ``start`` (mirrored left-right on request: another scene of the same generator) with ``bars`` painted"""
    frames, _ = synth.synth_clip(n, H, W, start=start)
    if mirror:
        frames = [np.ascontiguousarray(f[:, ::-1]) for f in frames]
    return [paint_bars(f, t0 + i, *bars) if bars != (0, 0) else f for i, f in enumerate(frames)]


def dim(frame, num, den):
    return ((frame.astype(np.int32) * num) // den).astype(np.uint8)


# scene starts far apart in the generator's time, alternately mirrored: every splice is a hard cut
_SCENES = ((0, False), (400, True), (910, False), (1370, True), (1800, False), (2300, True), (2750, False))


def _scene(k, n, bars, t0):
    s, m = _SCENES[k]
    return segment(s, n, bars, t0, m)


def clip(name):
    """(the frames the bootstrap samples, update frames).  Every update clip starts with 6 frames of the bootstrap scene (the cooldown
    runs out)."""
    from visiondepth3d_amd.letterbox import sample_indices
    head, upd = source(name)
    return [head[i] for i in sample_indices(len(head), FPS)], upd


@lru_cache(maxsize=None)
def source(name):
    """(the first 9 frames of the clip, which the bootstrap probes at 2 fps: 6 samples; the frames that go through update)"""
    boot = _scene(0, 9, BARS_P, 0)
    lead = _scene(0, 15, BARS_P, 0)[9:]
    if name == "fade":        # a fade to black and back inside one scene, then a cut to another scene with the same bars
        s = _scene(0, 24, BARS_P, 0)[15:]
        upd = lead + [s[0], dim(s[1], 1, 2), dim(s[2], 1, 16), dim(s[3], 0, 1), dim(s[4], 1, 16), s[5], s[6]] + _scene(1, 2, BARS_P, 30)
    elif name == "three_cuts":
        upd = lead + _scene(1, 2, BARS_Q, 20) + _scene(2, 2, BARS_Q, 30) + _scene(3, 3, BARS_Q, 40)
    elif name == "two_cuts":
        upd = lead + _scene(1, 2, BARS_Q, 20) + _scene(2, 4, BARS_Q, 30)
    elif name == "streak_reset":   # Q, Q, then a cut that shows the locked bars again (change < 8), then Q, Q: no switch; a third Q switches
        upd = (lead + _scene(1, 2, BARS_Q, 20) + _scene(2, 2, BARS_Q, 30) + _scene(3, 2, BARS_P, 40) + _scene(4, 2, BARS_Q, 50) +
               _scene(5, 2, BARS_Q, 60) + _scene(6, 2, BARS_Q, 70))
    elif name == "no_bars":       # a clip without bars: bootstrap stays at zero, cuts do not invent bars; the dimmed frame is a cut by the
        boot = _scene(0, 9, (0, 0), 0)   # histogram alone (MAD about 19, correlation about 0.5), and so is the frame after it
        s = _scene(2, 4, (0, 0), 0)
        upd = _scene(0, 15, (0, 0), 0)[9:] + _scene(1, 2, (0, 0), 0) + [s[0], s[1], dim(s[2], 7, 8), s[3]]
    else:
        raise KeyError(name)
    return boot, upd


CLIPS = ("fade", "three_cuts", "two_cuts", "streak_reset", "no_bars")


@lru_cache(maxsize=None)
def statement_run(name):
    """The numpy tracker on a clip: dict(boot=(top, bottom, (locked_bars, locked_zero)), bars=[(top, bottom)] per frame, gates=[per frame
    dict(near_black, mad, corr)], state=final lock state)"""
    from visiondepth3d_amd.letterbox import LetterboxTrackerNumpy
    boot, upd = clip(name)
    t = LetterboxTrackerNumpy(H, FPS)
    b = t.bootstrap(boot)
    bars, gates = [], []
    for f in upd:
        bars.append(tuple(int(v) for v in t.update(f)))
        gates.append(dict(t.last))
    return dict(boot=b, bars=bars, gates=gates, state=t.state())
