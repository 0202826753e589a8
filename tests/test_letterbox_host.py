"""CPU checks of visiondepth3d_amd/letterbox.py, the numpy statement of the depth pass's letterbox handling (core/render_depth.py:280-573,
1919-1933): the restated pairwise summation against numpy itself, Canny known answers, the tracker's rules on clips built here, the margin
every clip keeps from the scene-cut thresholds, the bar fill, and -- where the reference tree is present -- the reference's own tracker
on the same clips (recorded as tests/golden/letterbox_tracker.json: ``python tests/test_letterbox_host.py`` rewrites it)."""
import ast
import json
import os
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN
import letterbox_clips as LC
from visiondepth3d_amd import letterbox as lb

REF_FILE = os.path.join(os.environ.get("VD3D_REFERENCE", "/root/reference"), "core", "render_depth.py")
GOLDEN_JSON = os.path.join(GOLDEN, "letterbox_tracker.json")


# ---- pairwise statement ------------------------------------------------------------------------------------------------------------------
# 1, 5: a leaf shorter than 8 elements; 1920, 3840: 16 and 32 leaves; 4104: 33; 7689, 8190: 65, the most a row can have; 8192: 64
@pytest.mark.parametrize("w", [1, 5, 7, 64, 100, 129, 136, 333, 1920, 3840, 4104, 7689, 8190, 8192])
def test_pairwise_restatement_equals_numpy_mean_and_var(w):
    rng = np.random.default_rng(w)
    f = rng.integers(0, 256, (9, w, 3), dtype=np.uint8)
    y, s = lb.luma_saturation_numpy(f)
    assert y.dtype == np.float32
    for i in range(3):   # the scalar restatement, element by element
        assert lb.pairwise_sum(y[i]) == np.add.reduce(y[i])
    mean, var, sat = lb.row_uniformity_numpy(f)
    assert np.array_equal(mean, y.mean(axis=1)) and np.array_equal(var, y.var(axis=1)) and np.array_equal(sat, s.mean(axis=1))
    assert lb.luma_mean_numpy(y) == y.mean()          # the whole plane: one run of 9 * w elements
    flat = y.reshape(-1)
    if flat.size <= lb.NUMPY_BUFSIZE:
        assert lb.pairwise_sum(y) == np.add.reduce(flat)
    else:   # numpy hands a longer run to its inner loop in buffers of 8192: a pairwise sum per buffer, added up in order
        acc = np.float32(0)
        for o in range(0, flat.size, lb.NUMPY_BUFSIZE):
            acc = np.float32(acc + lb.pairwise_sum(flat[o:o + lb.NUMPY_BUFSIZE]))
        assert acc == np.add.reduce(flat)
    e = rng.random(w)
    assert lb.pairwise_sum(e, np.float64) == np.add.reduce(e)


@pytest.mark.parametrize("shape", [(64, 128), (1, 8193), (96, 136), (270, 480), (33, 1000), (81, 100), (103, 155), (1025, 8190)])
def test_whole_plane_mean_follows_numpys_reduction_buffers(shape):
    """Above 8192 elements numpy's y.mean() is not one pairwise sum: the plane goes through the 8192-element iteration buffer, a pairwise sum
    per buffer and a running sum over the buffers.  1025 x 8190 is 1025 buffers, the last one short: one more than the device's window of 1024."""
    assert np.getbufsize() == lb.NUMPY_BUFSIZE
    y = (np.random.default_rng(shape[1]).random(shape) * 255).astype(np.float32)
    assert lb.luma_mean_numpy(y) == y.mean()
    f = np.random.default_rng(shape[0]).integers(0, 256, shape + (3,), dtype=np.uint8)
    yy, _ = lb.luma_saturation_numpy(f)
    assert lb.luma_mean_numpy(yy) == yy.mean()


def test_a_shorter_run_can_have_more_leaves_than_a_full_buffer():
    """8192 elements split into 64 leaves of 128; 8100 into 65 smaller ones: what sizes the device's slot stride"""
    assert len(lb.pairwise_plan(8192)[0]) == 64 and len(lb.pairwise_plan(8100)[0]) == 65 and len(lb.pairwise_plan(7773)[0]) == 65
    assert max(len(lb.pairwise_plan(n)[0]) for n in range(7600, 8193)) == 65


def test_pairwise_plan_covers_the_range_once():
    for n in (1, 7, 128, 129, 257, 960 * 4, 96 * 128):
        leaves, comb = lb.pairwise_plan(n)
        assert [lo for lo, _ in leaves] == list(np.cumsum([0] + [m for _, m in leaves[:-1]])) and sum(m for _, m in leaves) == n
        assert all(1 <= m <= 128 for _, m in leaves) and len(comb) == len(leaves) - 1
        done = set(range(len(leaves)))
        for d, a, b in comb:   # children before parents
            assert a in done and b in done and d not in done
            done.add(d)


# ---- Canny known answers ---------------------------------------------------------------------------------------------------------------
def test_canny_vertical_step():
    g = np.zeros((32, 40), np.uint8)
    g[:, 20:] = 200
    e = lb.canny_numpy(g, 30, 90)
    assert set(np.unique(e)) == {0, 255}
    cols = np.unique(np.nonzero(e)[1])
    assert len(cols) == 1 and cols[0] in (19, 20) and np.count_nonzero(e) == 32
    g[:, 20:] = 20
    assert not lb.canny_numpy(g, 30, 90).any()


def _ramp_and_step(with_step):
    """a weak vertical edge (step of 14 levels: |dx| = 56, 56^2 = 3136 in (900, 8100]) whose lower end touches a strong step"""
    g = np.full((48, 64), 10, np.uint8)
    g[:, 32:] = 24
    if with_step:
        g[40:, :] = 200
    return g


def test_canny_weak_edge_needs_a_strong_neighbour():
    cls = lb.canny_classes_numpy(_ramp_and_step(True))
    assert (cls[5:30, 31:33] == 1).any() and not (cls[5:30] == 2).any() and (cls == 2).any()
    kept = lb.canny_numpy(_ramp_and_step(True))
    assert kept[5:30, 31:33].any(), "the weak edge is connected to the strong step: kept"
    alone = lb.canny_classes_numpy(_ramp_and_step(False))
    assert (alone == 1).any() and not (alone == 2).any()
    assert not lb.canny_numpy(_ramp_and_step(False)).any(), "the same weak edge on its own: dropped"


def test_hsv_saturation_and_gray_known_values():
    px = np.array([[[0, 0, 0], [255, 255, 255], [0, 0, 255], [10, 20, 40], [3, 3, 2]]], np.uint8)
    assert lb.hsv_saturation_numpy(px).tolist() == [[0, 0, 255, 191, 85]]
    assert lb.bgr2gray_numpy(px).tolist() == [[0, 255, 76, 25, 3]]
    assert lb.hist64_numpy(np.array([[0, 3, 4, 255]], np.uint8))[[0, 1, 63]].tolist() == [2, 1, 1]
    h = lb.hist64_numpy(np.arange(256, dtype=np.uint8))
    assert lb.hist_correlation(h, h) == 1.0                      # flat histograms: zero denominator
    a = np.zeros(64, np.int64); a[:8] = 5
    assert abs(lb.hist_correlation(a, a) - 1.0) < 1e-12 and lb.hist_correlation(a, a[::-1]) < 0


@pytest.mark.parametrize("hw", LC.CANNY_SIZES)
def test_canny_tie_planes_decide_a_tie_in_each_direction(hw):
    """The non-maximum test is > towards one neighbour and >= towards the other.  A plane whose edge map changes under a flip holds a tie that
    this asymmetry decides: a kernel with the comparison on the wrong side cannot pass on it.  (Uniform noise, the dense-edge input of the
    device test, gives an exactly mirror-symmetric map.)"""
    g = LC.tie_plane(*hw)
    e = lb.canny_numpy(g)
    assert e.any() == (hw != (1, 1))
    if hw[1] > 1:
        assert (lb.canny_numpy(g[:, ::-1])[:, ::-1] != e).any(), "no left-right tie"
    if hw[0] > 1:
        assert (lb.canny_numpy(g[::-1])[::-1] != e).any(), "no up-down tie"


# ---- tracker ---------------------------------------------------------------------------------------------------------------------------
def test_bootstrap_enables_bars_at_confidence():
    boot, _ = LC.clip("three_cuts")
    (t, b), conf = lb.multiframe_confidence_numpy(boot, LC.H)
    assert conf >= 0.7 and (t, b) != (0, 0)
    tr = lb.LetterboxTrackerNumpy(LC.H, LC.FPS)
    assert tr.bootstrap(boot) == (t, b, (True, False)) and tr.state()["cooldown"] == 6
    # the detected bars: within 2 rows of the painted ones, never beyond them, even
    assert 0 <= LC.BARS_P[0] - t <= 2 and 0 <= LC.BARS_P[1] - b <= 2 and t % 2 == 0 and b % 2 == 0
    t1, b1 = lb.detect_letterbox_strict_robust_numpy(LC.clip("three_cuts")[1][7])
    assert 0 <= LC.BARS_Q[0] - t1 <= 2 and 0 <= LC.BARS_Q[1] - b1 <= 2 and t1 % 2 == 0 and b1 % 2 == 0
    boot0, _ = LC.clip("no_bars")
    assert lb.LetterboxTrackerNumpy(LC.H, LC.FPS).bootstrap(boot0) == (0, 0, (False, True))
    # a confidence below conf_enable keeps the bars off: half of the samples without bars
    mixed = list(boot[:3]) + list(boot0[3:])
    (_, _), conf = lb.multiframe_confidence_numpy(mixed, LC.H)
    assert conf < 0.7 and lb.LetterboxTrackerNumpy(LC.H, LC.FPS).bootstrap(mixed) == (0, 0, (False, True))


def test_fade_to_black_keeps_the_bars():
    r = LC.statement_run("fade")
    assert [g["near_black"] for g in r["gates"]].count(True) == 3
    assert set(r["bars"]) == {r["boot"][:2]} and r["state"]["locked_bars"] == 1


def test_three_agreeing_cuts_switch_two_do_not():
    r3, r2 = LC.statement_run("three_cuts"), LC.statement_run("two_cuts")
    p = r3["boot"][:2]
    q = r3["bars"][-1]
    assert q != p and r3["bars"].index(q) == 10, "the third cut (frame 10) switches"
    assert 0 <= LC.BARS_Q[0] - q[0] <= 2 and 0 <= LC.BARS_Q[1] - q[1] <= 2
    assert r3["state"]["streak"] == 3 and r3["state"]["cooldown"] == 6 - 2
    assert set(r2["bars"]) == {p} and r2["state"]["streak"] == 2 and (r2["state"]["cand_top"], r2["state"]["cand_bottom"]) == q


def test_small_change_resets_the_streak():
    r = LC.statement_run("streak_reset")
    p, q = r["boot"][:2], r["bars"][-1]
    # cuts at frames 6, 8 (Q, Q), 10 (the locked bars again: streak back to 0), 12, 14 (Q, Q: still no switch), 16 (third Q: switch)
    assert r["bars"][:16] == [p] * 16 and r["bars"][16:] == [q] * 2 and q != p


def test_cuts_do_not_invent_bars():
    r = LC.statement_run("no_bars")
    assert set(r["bars"]) == {(0, 0)} and r["state"]["locked_zero"] == 1
    corr = [g["corr"] for g in r["gates"][-2:]]
    assert all(c is not None and c < lb.CORR_THRESH for c in corr), "the dimmed frame is a cut by the histogram test alone"


def _run_of(ok):
    """the rows from the top that pass the detector's row test"""
    return int(np.argmin(ok)) if not ok.all() else len(ok)


def test_every_new_clip_reaches_its_branch():
    """A clip that misses the branch it was built for would pass every comparison vacuously: the evidence, on the statement's own run."""
    run, cuts = LC.statement_run, LC.cuts
    zero, bars = dict(locked_zero=1, locked_bars=0), dict(locked_zero=0, locked_bars=1)
    has = lambda st, want: all(st[k] == v for k, v in want.items())

    r = run("bars_appear")                       # locked_zero -> bars, exactly at the third cut
    third = cuts("bars_appear")[2][0]
    assert r["boot"] == (0, 0, (False, True)) and r["state"]["locked_bars"] == 1 and len(cuts("bars_appear")) == 3
    assert r["bars"][:third] == [(0, 0)] * third and set(r["bars"][third:]) == {r["detect"][third]} != {(0, 0)}
    assert has(r["states"][third - 1], zero) and has(r["states"][third], bars)

    r = run("bars_vanish")                       # bars -> locked_zero, exactly at the third cut
    third = cuts("bars_vanish")[2][0]
    p = r["boot"][:2]
    assert r["boot"][2] == (True, False) and p != (0, 0) and r["state"]["locked_zero"] == 1 and len(cuts("bars_vanish")) == 3
    assert r["bars"][:third] == [p] * third and set(r["bars"][third:]) == {(0, 0)}
    assert has(r["states"][third - 1], bars) and has(r["states"][third], zero)

    r = run("over_cap")                          # bars inside the scan whose sum is above max_total count as (0, 0)
    live = [i for i, cd in cuts("over_cap") if cd == 0]
    max_total, scan = int(LC.H * 0.35), int(LC.H * lb.MAX_SCAN_FRAC)
    assert len(live) >= 3
    for i in live:
        t, b = r["detect"][i]
        assert t + b > max_total and 0 < t < scan and 0 < b < scan, (i, t, b)
    assert (r["state"]["cand_top"], r["state"]["cand_bottom"]) == (0, 0) and r["state"]["streak"] == 3
    assert r["boot"][2] == (True, False) and has(r["state"], zero), "the capped (0, 0) is what the three cuts agree on: the bars go"

    r = run("thin_bars")                         # rows pass the row test, but fewer than min_band of them
    min_band = int(LC.H * lb.MIN_BAND_FRAC)
    assert len(cuts("thin_bars")) >= 3 and max(LC.BARS_THIN) < min_band
    for i, _ in cuts("thin_bars"):
        # every painted row but the last passes (the last one carries the Canny edge of the bar's border): a run of 1 .. min_band - 1 rows
        top, bot = _run_of(r["row_ok"][i]), _run_of(r["row_ok"][i][::-1])
        assert top == LC.BARS_THIN[0] - 1 and bot == LC.BARS_THIN[1] - 1 and 0 < top < min_band and 0 < bot < min_band, (i, top, bot)
        assert r["detect"][i] == (0, 0)
    assert set(r["bars"]) == {(0, 0)} and r["state"]["streak"] == 0 and r["boot"] == (0, 0, (False, True))

    r = run("cooldown")                          # cuts with other bars while the cooldown of a switch runs: swallowed
    swallowed = [i for i, cd in cuts("cooldown") if cd > 0]
    assert len(swallowed) >= 1
    for i in swallowed:
        t, b = r["detect"][i]
        assert abs(t - r["bars"][i][0]) + abs(b - r["bars"][i][1]) >= 8 and r["bars"][i] != r["boot"][:2], (i, t, b)
        assert r["states"][i]["streak"] == r["states"][i - 1]["streak"] and r["states"][i]["cand_top"] == r["states"][i - 1]["cand_top"]
    after = [i for i, cd in cuts("cooldown") if cd == 0 and i > swallowed[-1]]
    assert after and r["states"][after[0]]["streak"] == 1 and (r["state"]["cand_top"], r["state"]["cand_bottom"]) == r["detect"][after[0]]

    for name in ("size_switch", "size_switch_back"):   # the first frame of the other size is a cut without a MAD
        r, (_, upd) = run(name), LC.clip(name)
        sw = [i for i in range(1, len(upd)) if upd[i].shape != upd[i - 1].shape]
        assert len(sw) == 1 and upd[0].shape[0] == LC.geometry(name)[0]
        g = r["gates"][sw[0]]
        assert g["mad"] is None and g["corr"] is None and not g["near_black"] and (sw[0], 0) in cuts(name)
        assert r["states"][sw[0]]["streak"] == 1 and r["state"]["streak"] == 3 and r["bars"][-1] != r["boot"][:2]
        assert [len(b) for b in LC.batches(upd)] == [sw[0], len(upd) - sw[0]] and max(len(b) for b in LC.batches(upd, 4)) == 4

    r = run("small_frame")                       # H < 64: bars that the row test passes are refused all the same
    assert LC.geometry("small_frame")[0] < 64 and len(cuts("small_frame")) >= 3 and all(cd == 0 for _, cd in cuts("small_frame"))
    assert set(r["bars"]) == {(0, 0)} and set(r["detect"]) == {(0, 0)} and r["state"]["streak"] == 0
    for i, _ in cuts("small_frame"):
        top, bot = _run_of(r["row_ok"][i]), _run_of(r["row_ok"][i][::-1])
        assert (top - top % 2) + (bot - bot % 2) >= 8 and min(top, bot) >= int(48 * lb.MIN_BAND_FRAC), "bars a taller frame would have counted"

    r = run("tall_frame")                        # the near-black gate reads the edge mean: at H = 150 a tree of two leaves with a tail
    leaves, comb = lb.pairwise_plan(LC.geometry("tall_frame")[0])
    assert len(leaves) == 2 and len(comb) == 1 and leaves[-1][1] % 8 != 0
    assert [g["near_black"] for g in r["gates"]].count(True) >= 1 and len(set(r["bars"])) == 2 and r["state"]["locked_bars"] == 1
    # ... and one dark frame on which that sum decides: not near-black, so a cut that takes a streak of 2 back to 1 -- with any one of the
    # tail's rows left out of the sum it would be skipped as near-black, and the next cut would be the third agreeing one
    upd = LC.clip("tall_frame")[1]
    d = [i for i, f in enumerate(upd) if np.array_equal(f, LC.dark_title())]
    assert len(d) == 1 and (d[0], 0) in LC.cuts("tall_frame") and not r["gates"][d[0]]["near_black"]
    st = lb.frame_stats_numpy(upd[d[0]])
    e = lb.edge_density_from_counts(st["edge_counts"], st["w"])
    tail = range(leaves[-1][0] + leaves[-1][1] - leaves[-1][1] % 8, len(e))
    assert float(st["frame_mean"]) < lb.BLACK_MEAN and len(tail) == 6
    assert lb._edge_mean(st) >= lb.BLACK_EDGE + 0.001 and all((e.sum() - e[i]) / len(e) < lb.BLACK_EDGE - 0.0002 for i in tail)
    assert r["states"][d[0] - 1]["streak"] == 2 and r["states"][d[0]]["streak"] == 1 and r["detect"][d[0]] != r["detect"][d[0] + 1]
    assert r["bars"].index(r["bars"][-1]) == LC.cuts("tall_frame")[-1][0] > d[0] + 1


def _margins(name):
    boot, upd = LC.clip(name)
    out, prev = [], None
    for f in boot:   # the bootstrap's own comparisons between the sampled frames
        st = lb.frame_stats_numpy(f, None if prev is None else prev["gray"])
        if prev is not None:
            out.append(lb.scene_cut_metrics(st, prev))
        prev = st
    return out + [(g["mad"], g["corr"]) for g in LC.statement_run(name)["gates"]]


@pytest.mark.parametrize("name", LC.CLIPS)
def test_every_clip_keeps_its_margin_from_the_thresholds(name):
    """A later pin of the cv2 restatements against a real OpenCV must not flip a fixture: MAD at least 0.5 from 28, correlation at least
    0.01 from 0.60, on every comparison the clips ever make."""
    n = 0
    for mad, corr in _margins(name):
        if mad is not None:
            assert abs(mad - lb.MAD_THRESH) >= 0.5, (name, mad)
            n += 1
        if corr is not None:
            assert abs(corr - lb.CORR_THRESH) >= 0.01, (name, corr)
    assert n >= 10


# ---- bar fill --------------------------------------------------------------------------------------------------------------------------
def test_letterbox_fill_on_a_ramp_plane(oracle):
    y, x = np.mgrid[0:64, 0:64]
    d = ((y * 3 + x) % 256).astype(np.uint8)
    out = lb.letterbox_fill_numpy(d, 10, 6)
    core = oracle.resize_cubic_u8(d, 48, 64)                    # the project's INTER_CUBIC statement
    assert np.array_equal(out[10:58], core) and np.array_equal(lb.resize_cubic_u8_numpy(d, 48, 64), core)
    med = int(np.median(core))
    assert (out[:10] == med).all() and (out[58:] == med).all()
    assert np.array_equal(lb.letterbox_fill_numpy(d, 0, 0), d)
    assert np.array_equal(lb.letterbox_fill_numpy(d, 40, 30), d), "bars that leave no picture are dropped"
    # an even count whose two middle values differ by an odd amount: int() truncates the .5
    e = np.zeros((64, 64), np.uint8)
    e[32:] = 255
    o = lb.letterbox_fill_numpy(e, 0, 2)
    c = oracle.resize_cubic_u8(e, 62, 64)
    assert o[63, 0] == int(np.median(c)) and np.array_equal(o[:62], c)


# ---- the reference's own tracker on the same clips ------------------------------------------------------------------------------------
def _reference_namespace():
    """The tracker part of the reference's core/render_depth.py (the module pulls in diffusers, tkinter ...: its letterbox definitions are
    located with ``ast`` and compiled on their own) over a cv2 made of the statement's functions."""
    cv2 = types.SimpleNamespace(COLOR_BGR2GRAY=6, COLOR_BGR2HSV=40, HISTCMP_CORREL=0, CAP_PROP_FRAME_COUNT=7, CAP_PROP_POS_FRAMES=1)

    def cvt(img, code):
        if code == cv2.COLOR_BGR2GRAY:
            return lb.bgr2gray_numpy(img)
        assert code == cv2.COLOR_BGR2HSV
        hsv = np.zeros(img.shape, np.uint8)
        hsv[..., 1] = lb.hsv_saturation_numpy(img)
        return hsv

    def normalize(src, dst):
        dst[...] = lb.hist_normalize_numpy(src).reshape(dst.shape)

    cv2.cvtColor = cvt
    cv2.Canny = lambda gray, low, high, apertureSize=3, L2gradient=False: lb.canny_numpy(gray, low, high)
    cv2.calcHist = lambda imgs, ch, mask, size, rng: lb.hist64_numpy(imgs[0]).astype(np.float32).reshape(64, 1)
    cv2.normalize = normalize
    cv2.compareHist = lambda a, b, m: lb.hist_correl_numpy(a, b)
    want = {"_luma_saturation", "is_scene_cut", "_row_uniformity_metrics", "_horizontal_edge_density", "detect_letterbox_strict_robust",
            "is_near_black_frame", "detect_letterbox_multiframe_confidence", "LetterboxTracker"}
    body = [n for n in ast.parse(open(REF_FILE).read()).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in want]
    assert {n.name for n in body} == want
    ns = dict(np=np, cv2=cv2)
    exec(compile(ast.Module(body=body, type_ignores=[]), REF_FILE, "exec"), ns)
    return ns, cv2


class _Cap:
    def __init__(self, frames, cv2):
        self.frames, self.pos, self.cv2 = frames, 0, cv2

    def get(self, prop):
        return float(len(self.frames)) if prop == self.cv2.CAP_PROP_FRAME_COUNT else float(self.pos)

    def set(self, prop, v):
        self.pos = int(v)

    def read(self):
        f = self.frames[self.pos].copy() if self.pos < len(self.frames) else None
        self.pos += 1
        return f is not None, f


def _reference_run(name):
    ns, cv2 = _reference_namespace()
    head, upd = LC.source(name)
    h, _, fps = LC.geometry(name)
    tr = ns["LetterboxTracker"](h, fps)
    t, b, locks = tr.bootstrap(_Cap(list(head), cv2))
    bars = [[int(v) for v in tr.update(f, i)] for i, f in enumerate(upd)]
    return dict(boot=[int(t), int(b), bool(locks[0]), bool(locks[1])], bars=bars)


@pytest.mark.skipif(not os.path.isfile(REF_FILE), reason="reference tree not present")
@pytest.mark.parametrize("name", LC.CLIPS)
def test_reference_tracker_agrees_on_the_clips(name):
    ref, r = _reference_run(name), LC.statement_run(name)
    assert ref["boot"] == [r["boot"][0], r["boot"][1], r["boot"][2][0], r["boot"][2][1]]
    assert [tuple(v) for v in ref["bars"]] == r["bars"]
    assert json.load(open(GOLDEN_JSON))[name] == ref, "tests/golden/letterbox_tracker.json is stale"


@pytest.mark.parametrize("name", LC.CLIPS)
def test_statement_tracker_equals_the_recorded_reference_sequences(name):
    rec, r = json.load(open(GOLDEN_JSON))[name], LC.statement_run(name)
    assert rec["boot"] == [r["boot"][0], r["boot"][1], r["boot"][2][0], r["boot"][2][1]]
    assert [tuple(v) for v in rec["bars"]] == r["bars"]


if __name__ == "__main__":
    with open(GOLDEN_JSON, "w") as fh:
        json.dump({n: _reference_run(n) for n in LC.CLIPS}, fh, indent=1)
        fh.write("\n")
    print("wrote", GOLDEN_JSON)
