"""GPU tests (-m gpu) of the letterbox kernels (csrc/vd3d_letterbox.hip) against the numpy statement (visiondepth3d_amd/letterbox.py), bit for
bit: the statistics pass, Canny and its hysteresis on hand-made class maps, the tracker on the host tests' clips at several batch sizes, the
bar fill and DepthPipe.depth_frames_u8(bars=...)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import letterbox_clips as LC
from visiondepth3d_amd import letterbox as lb
from visiondepth3d_amd import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [(64, 64), (72, 100), (96, 136), (270, 480)]   # W not a multiple of 8, W > 128 (a tree above the leaves), several Canny tiles


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _frames(h, w):
    """three frames: two neighbours of a synth clip and a noise frame"""
    rng = np.random.default_rng(h * 1000 + w)
    return np.stack([synth.synth_frame(3, h, w)[0], synth.synth_frame(4, h, w)[0], rng.integers(0, 256, (h, w, 3), dtype=np.uint8)])


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
# 81 x 100 = 8100 elements: the last (here the only) chunk of the whole-plane mean splits into 65 leaves, one more than a full 8192-element chunk;
# 103 x 155 = 8192 + 7773: a full chunk followed by such a tail, in every frame of the batch
# Wide rows, few of them (k_lb_rows gives a leaf to each 8-lane group, 32 leaves per sweep): 1920 is 16 leaves (wave 1 sums too), 3840 and 4096
# are 32 (every group of every wave), 4104 is 33 (a second sweep with one leaf), 7688 is 64 (two full sweeps), 7689 and 8190 are 65 leaves + 64
# steps (the largest plan there is, a third sweep), 8192 is 64 again.
WIDE = [(4, 1920), (4, 3840), (3, 4096), (3, 4104), (3, 7688), (3, 7689), (3, 8190), (2, 8192)]
# Rows shorter than 8 (the plain loop of a leaf), one leaf and no combine step, a single row, a single column, 130 = two leaves of 64 and 66
DEGENERATE = [(1, 1), (1, 7), (7, 1), (2, 9), (5, 8), (3, 130)]


@pytest.mark.parametrize("hw", SIZES + [(81, 100), (103, 155)] + WIDE + DEGENERATE)
def test_stats_bit_exact_vs_statement(R, hw):
    h, w = hw
    f = _frames(h, w)
    R.letterbox_state_reset()
    got = {k: v.cpu().numpy() for k, v in R.letterbox_stats(torch.from_numpy(f).cuda()).items()}
    prev = None
    for b in range(f.shape[0]):
        st = lb.frame_stats_numpy(f[b], prev)
        prev = st["gray"]
        y, s = lb.luma_saturation_numpy(f[b])
        assert np.array_equal(got["row_mean"][b].view(np.uint32), st["row_mean"].view(np.uint32)), (hw, b)
        assert np.array_equal(got["row_mean"][b], y.mean(axis=1)) and np.array_equal(got["row_var"][b], y.var(axis=1)), "numpy itself"
        assert np.array_equal(got["row_var"][b].view(np.uint32), st["row_var"].view(np.uint32)), (hw, b)
        assert np.array_equal(got["row_sat"][b], s.astype(np.int64).sum(axis=1)), (hw, b)
        assert np.array_equal(got["gray"][b], st["gray"]) and np.array_equal(got["hist"][b], st["hist"]), (hw, b)
        assert int(got["mad_sum"][b]) == (st["mad_sum"] if b else 0), (hw, b)
        assert got["frame_mean"][b] == st["frame_mean"] == y.mean(), (hw, b)


def test_stats_chain_compares_with_the_previous_batch(R):
    f = _frames(72, 100)
    R.letterbox_state_reset()
    dev = torch.from_numpy(f).cuda()
    a = R.letterbox_stats(dev[:2], chain=True)
    b = R.letterbox_stats(dev[2:], chain=True)
    whole = R.letterbox_stats(dev)
    assert int(a["mad_sum"][0]) == 0
    assert int(b["mad_sum"][0]) == int(whole["mad_sum"][2]) > 0
    s = R.letterbox_state_export(with_frame=True)
    assert (s["have_prev"], s["prev_h"], s["prev_w"]) == (1, 72, 100)
    assert np.array_equal(s["prev_gray"].cpu().numpy(), lb.bgr2gray_numpy(f[2])) and np.array_equal(s["prev_hist"], lb.hist64_numpy(lb.bgr2gray_numpy(f[2])))


def test_frame_mean_over_more_chunks_than_its_window(R):
    """1025 x 8190 is 1025 chunks of 8192 elements, the last one short: k_lb_frame_mean sums 1024 chunk sums per pass through its LDS window, so
    its second pass gets exactly the tail chunk.  Against numpy itself and the statement of its order; the statement's Canny is not needed."""
    h, w = 1025, 8190
    assert -(-h * w // lb.NUMPY_BUFSIZE) == 1025 and h * w % lb.NUMPY_BUFSIZE
    f = np.random.default_rng(h + w).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    R.letterbox_state_reset()
    got = {k: v.cpu().numpy() for k, v in R.letterbox_stats(torch.from_numpy(f).cuda()).items() if k != "gray"}
    y, s = lb.luma_saturation_numpy(f[0])
    assert got["frame_mean"][0] == lb.luma_mean_numpy(y), (got["frame_mean"][0], lb.luma_mean_numpy(y))
    assert got["frame_mean"][0] == y.mean(), "numpy itself"
    assert np.array_equal(got["row_mean"][0], y.mean(axis=1)) and np.array_equal(got["row_var"][0], y.var(axis=1))
    assert np.array_equal(got["row_sat"][0], s.astype(np.int64).sum(axis=1)) and int(got["mad_sum"][0]) == 0


def test_stats_chain_across_a_change_of_size(R):
    """The state's gray plane grows (72 x 100 -> 96 x 136) and is reused at a smaller size (-> 72 x 100): no comparison across the change, the
    usual one inside a size, and the state keeps the last frame each time."""
    R.letterbox_state_reset()
    for h, w in ((72, 100), (96, 136), (72, 100)):
        f = _frames(h, w)
        gray = [lb.bgr2gray_numpy(fr).astype(np.int64) for fr in f]
        dev = torch.from_numpy(f).cuda()
        a = R.letterbox_stats(dev[:2], chain=True)
        assert int(a["mad_sum"][0]) == 0, (h, w)
        assert int(a["mad_sum"][1]) == int(np.abs(gray[1] - gray[0]).sum()) > 0
        b = R.letterbox_stats(dev[2:], chain=True)
        assert int(b["mad_sum"][0]) == int(np.abs(gray[2] - gray[1]).sum()) > 0, (h, w)
        s = R.letterbox_state_export(with_frame=True)
        assert (s["have_prev"], s["prev_h"], s["prev_w"]) == (1, h, w)
        assert np.array_equal(s["prev_gray"].cpu().numpy(), gray[2]) and np.array_equal(s["prev_hist"], lb.hist64_numpy(gray[2].astype(np.uint8)))


# ---- Canny -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES)
def test_canny_equals_statement(R, hw):
    h, w = hw
    gray = np.stack([lb.bgr2gray_numpy(fr) for fr in _frames(h, w)])
    gray[2, : h // 2] = np.random.default_rng(5).integers(0, 256, (h // 2, w), dtype=np.uint8)   # noise on the gray plane itself: dense edges
    edges, counts = R.canny_u8(torch.from_numpy(gray).cuda(), 30, 90, want_counts=True)
    edges, counts = edges.cpu().numpy(), counts.cpu().numpy()
    for b in range(3):
        exp = lb.canny_numpy(gray[b], 30, 90)
        assert exp.any()
        assert np.array_equal(edges[b], exp), (hw, b, int(np.count_nonzero(edges[b] != exp)))
        assert np.array_equal(counts[b], np.count_nonzero(exp, axis=1))


@pytest.mark.parametrize("hw", LC.CANNY_SIZES)
def test_canny_small_sizes_and_tie_planes(R, hw):
    """Images smaller than the 64 x 16 tile plus halo, exactly one tile, one pixel past it; the third plane decides ties of the non-maximum test
    in both directions (tests/test_letterbox_host.py asserts that on the statement), so it goes through with both of its flips."""
    h, w = hw
    tie = LC.tie_plane(h, w)
    gray = np.stack([lb.bgr2gray_numpy(fr) for fr in _frames(h, w)[1:]] + [tie])     # a synth frame, noise, the tie plane
    flips = np.stack([np.ascontiguousarray(tie[:, ::-1]), np.ascontiguousarray(tie[::-1])])
    for planes in (gray, flips):
        edges, counts = R.canny_u8(torch.from_numpy(planes).cuda(), 30, 90, want_counts=True)
        edges, counts = edges.cpu().numpy(), counts.cpu().numpy()
        for b in range(len(planes)):
            exp = lb.canny_numpy(planes[b], 30, 90)
            assert np.array_equal(edges[b], exp), (hw, b, int(np.count_nonzero(edges[b] != exp)))
            assert np.array_equal(counts[b], np.count_nonzero(exp, axis=1)), (hw, b)
    assert lb.canny_numpy(tie).any() == (hw != (1, 1))


def _serpentine(h, w, step=4):
    """a one-pixel path that sweeps every row band of the map: right along row 1, down, left along row 1 + step, ..."""
    path, y, right = [], 1, True
    while y < h - 1:
        xs = range(1, w - 1) if right else range(w - 2, 0, -1)
        path += [(y, x) for x in xs]
        x_end = w - 2 if right else 1
        nxt = y + step
        if nxt < h - 1:
            path += [(yy, x_end) for yy in range(y + 1, nxt)]
        y, right = nxt, not right
    return path


def test_hysteresis_on_hand_made_class_maps(R):
    h, w = 96, 160
    path = _serpentine(h, w)
    ys, xs = np.array([p[0] for p in path]), np.array([p[1] for p in path])
    assert ys.max() >= h - 5 and len(path) > 3000
    with_strong = np.zeros((h, w), np.uint8)
    with_strong[ys, xs] = 1
    with_strong[path[-1]] = 2                                  # the single strong pixel at the far end
    without = (with_strong > 0).astype(np.uint8)
    diag = np.zeros((h, w), np.uint8)                          # a staircase connected through corners only, up-right then down-right
    k = np.arange(80)
    diag[90 - k, 5 + k] = 1
    diag[12 + k[:70], 85 + k[:70]] = 1
    diag[90, 5] = 2
    diag[40, 2] = 1                                            # an isolated weak pixel
    broken = diag.copy()
    broken[50, 45] = 0                                         # cut the chain: everything behind the gap goes
    maps = np.stack([with_strong, without, diag, broken])
    dev = torch.from_numpy(maps).cuda()
    got, cnt = R.canny_hysteresis_u8(dev, want_counts=True)
    got, cnt = got.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(got[0], np.where(with_strong > 0, 255, 0)), "every pixel of the serpentine hangs on its last one"
    assert not got[1].any()
    assert np.array_equal(got[2] > 0, (diag > 0) & ~((np.arange(h)[:, None] == 40) & (np.arange(w)[None, :] == 2)))
    for b in range(4):
        assert np.array_equal(got[b], lb.hysteresis_numpy(maps[b])), b
        assert np.array_equal(cnt[b], np.count_nonzero(got[b], axis=1))
    assert np.count_nonzero(got[3]) == 40 and got[3][90, 5] == 255 and got[3][49, 46] == 0
    again = R.canny_hysteresis_u8(dev).cpu().numpy()
    assert np.array_equal(again, got)


# ---- tracker ---------------------------------------------------------------------------------------------------------------------------
def _device_run(R, name, batch):
    boot, upd = LC.clip(name)
    h, _, fps = LC.geometry(name)
    t = lb.LetterboxTracker(R, h, fps)
    b = t.bootstrap(torch.from_numpy(np.stack(boot)))
    bars = torch.cat([t.update(torch.from_numpy(np.stack(fr)).cuda()) for fr in LC.batches(upd, batch)]).cpu().numpy()   # a batch has one frame size
    return b, [tuple(int(v) for v in r) for r in bars], t


@pytest.mark.parametrize("name", LC.CLIPS)
def test_tracker_equals_statement_at_every_batch_size(R, name):
    exp = LC.statement_run(name)
    rec = json.load(open(os.path.join(GOLDEN, "letterbox_tracker.json")))[name]
    for batch in (1, 4, None):
        boot, bars, t = _device_run(R, name, batch)
        assert boot == exp["boot"], (name, batch)
        assert bars == exp["bars"], (name, batch)
        assert t.state() == exp["state"], (name, batch)
        assert [list(v) for v in bars] == rec["bars"] and list(boot[:2]) == rec["boot"][:2], "the reference's own tracker, recorded"


def test_tracker_state_round_trips_through_export_and_import(R):
    name = "streak_reset"
    exp = LC.statement_run(name)
    boot, upd = LC.clip(name)
    frames = torch.from_numpy(np.stack(upd)).cuda()
    h, _, fps = LC.geometry(name)
    t = lb.LetterboxTracker(R, h, fps)
    t.bootstrap(torch.from_numpy(np.stack(boot)))
    first = t.update(frames[:9]).cpu().numpy()                  # stops between two cuts with a streak of 2 pending
    saved = R.letterbox_state_export(with_frame=True)
    assert saved["streak"] == 2 and saved["have_prev"] == 1
    R.letterbox_state_reset()
    assert R.letterbox_state_export()["have_prev"] == 0 and R.letterbox_state_export()["locked_zero"] == 1
    R.letterbox_state_import(saved)
    back = R.letterbox_state_export(with_frame=True)
    assert {k: v for k, v in back.items() if not k.startswith("prev_g") and k != "prev_hist"} == \
           {k: v for k, v in saved.items() if not k.startswith("prev_g") and k != "prev_hist"}
    assert torch.equal(back["prev_gray"], saved["prev_gray"]) and np.array_equal(back["prev_hist"], saved["prev_hist"])
    rest = t.update(frames[9:]).cpu().numpy()
    assert [tuple(int(v) for v in r) for r in np.concatenate([first, rest])] == exp["bars"]
    assert t.state() == exp["state"]


# ---- fill and DepthPipe ------------------------------------------------------------------------------------------------------------------
def _depth_planes(h, w):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(h + w)
    return np.stack([((y * 3 + x) % 256).astype(np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8),
                     (synth.synth_frame(0, h, w)[1] * 255).astype(np.uint8), np.where(y < h // 2, 0, 255).astype(np.uint8)])


@pytest.mark.parametrize("hw", [(64, 64), (90, 130)])
def test_fill_equals_statement(R, hw):
    h, w = hw
    d = _depth_planes(h, w)
    bars = np.array([[10, 6], [0, 0], [h // 2, h // 2 + 3], [0, 3]], np.int32)   # asymmetric, none, top + bottom >= h, an odd median pair
    got = R.depth_letterbox_fill(torch.from_numpy(d).cuda(), torch.from_numpy(bars).cuda()).cpu().numpy()
    for b in range(4):
        assert np.array_equal(got[b], lb.letterbox_fill_numpy(d[b], *bars[b])), (hw, b)
    assert np.array_equal(got[1], d[1]) and np.array_equal(got[2], d[2])
    one = R.depth_letterbox_fill(torch.from_numpy(d).cuda(), (7, 12)).cpu().numpy()
    for b in range(4):
        assert np.array_equal(one[b], lb.letterbox_fill_numpy(d[b], 7, 12)), (hw, b)


# core_h = 1 (one picture row, either side), core_h = 2, a single bar row (either side), no picture row left (the plane is copied); H = 1
SQUEEZES = [((40, 70), [(39, 0), (0, 39), (19, 19), (1, 0), (0, 1), (40, 0)]), ((1, 70), [(1, 0), (0, 0)])]


@pytest.mark.parametrize("hw,pairs", SQUEEZES)
def test_fill_at_the_extreme_squeezes(R, hw, pairs):
    h, w = hw
    d = _depth_planes(h, w)
    exp = {p: [lb.letterbox_fill_numpy(d[k], *p) for k in range(4)] for p in pairs}
    for p in pairs:   # one pair for every plane
        one = R.depth_letterbox_fill(torch.from_numpy(d).cuda(), p).cpu().numpy()
        for k in range(4):
            assert np.array_equal(one[k], exp[p][k]), (hw, p, k)
    # a pair per plane: every plane kind with every pair, in one batch
    planes = np.concatenate([d] * len(pairs))
    bars = np.array([p for p in pairs for _ in range(4)], np.int32)
    got = R.depth_letterbox_fill(torch.from_numpy(planes).cuda(), torch.from_numpy(bars).cuda()).cpu().numpy()
    for i, p in enumerate(pairs):
        for k in range(4):
            assert np.array_equal(got[4 * i + k], exp[p][k]), (hw, p, k)
    if (h, 0) in pairs:
        assert all(np.array_equal(exp[(h, 0)][k], d[k]) for k in range(4)), "no picture row left: the plane as it is"
    if h > 1:
        assert (exp[(h - 1, 0)][0][:h - 1] == exp[(h - 1, 0)][0][0, 0]).all() and exp[(h - 1, 0)][1][h - 1].std() > 0, "one picture row under a filled bar"


# ---- seeded sweep ------------------------------------------------------------------------------------------------------------------------
def test_seeded_sweep_of_small_geometries(R):
    """24 geometries from a fixed seed, H in 1..47, W in 1..399, a noise frame and a block frame each: statistics, Canny with its row counts and
    one fill with random valid bars, all against the statement."""
    rng = np.random.default_rng(0)
    for _ in range(24):
        h, w = int(rng.integers(1, 48)), int(rng.integers(1, 400))
        tie = LC.tie_plane(h, w)
        f = np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.stack([tie, tie[:, ::-1], tie[::-1]], axis=-1)])
        top = int(rng.integers(0, h))
        bars = np.array([[top, int(rng.integers(0, h - top))], [int(rng.integers(0, h)), 0]], np.int32)
        geo = dict(h=h, w=w, bars=bars.tolist())
        R.letterbox_state_reset()
        got = {k: v.cpu().numpy() for k, v in R.letterbox_stats(torch.from_numpy(f).cuda()).items()}
        gray = np.stack([lb.bgr2gray_numpy(f[0]), tie])
        edges, counts = R.canny_u8(torch.from_numpy(gray).cuda(), 30, 90, want_counts=True)
        edges, counts = edges.cpu().numpy(), counts.cpu().numpy()
        fill = R.depth_letterbox_fill(torch.from_numpy(gray).cuda(), torch.from_numpy(bars).cuda()).cpu().numpy()
        prev = None
        for b in range(2):
            st = lb.frame_stats_numpy(f[b], prev)
            prev = st["gray"]
            _, s = lb.luma_saturation_numpy(f[b])
            for k in ("row_mean", "row_var"):
                assert np.array_equal(got[k][b].view(np.uint32), st[k].view(np.uint32)), (geo, b, k)
            assert np.array_equal(got["row_sat"][b], s.astype(np.int64).sum(axis=1)), (geo, b)
            assert np.array_equal(got["gray"][b], st["gray"]) and np.array_equal(got["hist"][b], st["hist"]), (geo, b)
            assert int(got["mad_sum"][b]) == (st["mad_sum"] if b else 0), (geo, b)
            assert got["frame_mean"][b] == st["frame_mean"], (geo, b)
            exp = lb.canny_numpy(gray[b], 30, 90)
            assert np.array_equal(edges[b], exp), (geo, b, int(np.count_nonzero(edges[b] != exp)))
            assert np.array_equal(counts[b], np.count_nonzero(exp, axis=1)), (geo, b)
            assert np.array_equal(fill[b], lb.letterbox_fill_numpy(gray[b], *bars[b])), (geo, b)


@pytest.fixture(scope="module")
def pipe(R):
    """the smallest model of the zoo with synthetic weights.  The library GEMMs / convolutions behind the network are not bit-reproducible from
    call to call, so equal inputs get the first call's prediction: what is compared exactly is the code AROUND the network."""
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    p = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R, processor=dict(PROCESSORS["da"], size=(112, 112), multiple=14))
    real, memo = p.infer_bgr_u8, {}

    def cached(frames, inference_size=None, raw=False, at_inference_size=False):
        key = (tuple(frames.shape), int(frames.to(torch.int64).sum()), inference_size, raw, at_inference_size)
        if key not in memo:
            memo[key] = real(frames, inference_size, raw=raw, at_inference_size=at_inference_size)
        return memo[key]
    p.infer_bgr_u8 = cached
    return p


@pytest.mark.parametrize("tiled", [False, True])
def test_depth_pipe_bars_equals_its_own_output_through_the_statement(R, pipe, tiled):
    kw = dict(tiled=True, tile=64, pad=8) if tiled else {}
    frames = torch.from_numpy(np.stack(synth.synth_clip(2, 96, 128)[0])).cuda()   # tile 64, pad 8: every tile keeps a size the network takes
    plain = pipe.depth_frames_u8(frames, **kw)
    assert torch.equal(pipe.depth_frames_u8(frames, bars=None, **kw), plain), "bars=None is the call without the keyword"
    host = plain.cpu().numpy()
    assert host[0].min() != host[0].max()
    got = pipe.depth_frames_u8(frames, bars=(8, 6), **kw).cpu().numpy()
    dev_bars = torch.tensor([[8, 6], [0, 0]], dtype=torch.int32, device="cuda")   # what LetterboxTracker.update hands over
    got2 = pipe.depth_frames_u8(frames, bars=dev_bars, **kw).cpu().numpy()
    for b in range(2):
        assert np.array_equal(got[b], lb.letterbox_fill_numpy(host[b], 8, 6)), (tiled, b)
    assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[1], host[1])
