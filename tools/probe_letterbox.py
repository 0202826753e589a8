"""Letterbox-aware depth pass measured on one GPU: the device tracker (letterbox.LetterboxTracker.update) and the bar fill
(Renderer.depth_letterbox_fill) next to the depth forward they ride along with, per frame, at batch 16.

  per frame size (1080p, 4K), ms per frame, device-event time ending in a synchronise, warm-up first, `--repeats` windows of `--iters`
  batches each (median, min .. max):
    update          LetterboxTracker.update(frames[16]) = statistics pass + Canny + hysteresis + one tracker launch
    its stages      letterbox_stats, canny_u8 on the gray planes (class map + labelling) and the tracker launch's remainder
    fill            depth_letterbox_fill of 16 uint8 depth planes with bars (H/8, H/8)
    depth forward   DepthPipe.depth_frames_u8(frames[16]) -- DA-V2-Small, float32, synthetic weights, the ~518-pixel window
  and the same content check the tests make (device bars == the numpy statement on one small clip), so a timing never stands for a wrong result.

  python tools/probe_letterbox.py [--sizes 1080,2160] [--batch 16] [--repeats 3] [--iters 5] [--no-depth] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visiondepth3d_amd import letterbox as lb  # noqa: E402
from visiondepth3d_amd import synth  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402


def ev_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def spread(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def clip(n, h, w):
    """n synth frames with dark bars of h/8 rows, a hard cut in the middle (another scene, mirrored)"""
    frames = []
    for i in range(n):
        f = synth.synth_frame(i if i < n // 2 else 500 + i, h, w)[0]
        if i >= n // 2:
            f = np.ascontiguousarray(f[:, ::-1])
        f[: h // 8] = (np.arange(w)[None, :, None] + i) % 4
        f[h - h // 8:] = (np.arange(w)[None, :, None] + i) % 4
        frames.append(f)
    return np.stack(frames)


def check(R):
    """device tracker == numpy statement on a small clip (bootstrap + updates in two batches)"""
    f = clip(12, 96, 128)
    t, s = lb.LetterboxTracker(R, 96, 2), lb.LetterboxTrackerNumpy(96, 2)
    assert t.bootstrap(torch.from_numpy(f[:6])) == s.bootstrap(list(f[:6]))
    dev = torch.from_numpy(f).cuda()
    got = torch.cat([t.update(dev[:5]), t.update(dev[5:])]).cpu().numpy().tolist()
    assert got == [list(s.update(x)) for x in f], "device tracker differs from the statement"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080,2160")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-depth", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    assert torch.cuda.is_available(), "probe_letterbox measures on a GPU; there is no other path"
    R = Renderer(0)
    check(R)
    B = a.batch
    say(f"device: {torch.cuda.get_device_name(0)}; batch {B}; ms PER FRAME, median (min .. max) of {a.repeats} windows of {a.iters} batches; "
        "content check (device tracker == statement) passed")
    say("")
    say("| frame | update | of which statistics | of which Canny (NMS + labelling) | fill | depth forward (DA-V2-Small f32) | update / forward |")
    say("|---|---|---|---|---|---|---|")
    pipe = None
    if not a.no_depth:
        from visiondepth3d_amd.depth import DepthPipe
        pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R)
    for h in (int(v) for v in a.sizes.split(",")):
        w = h * 16 // 9
        frames = torch.from_numpy(clip(B, h, w)).cuda()
        trk = lb.LetterboxTracker(R, h, 24.0)
        depth = torch.from_numpy(np.stack([(synth.synth_frame(i, h, w)[1] * 255).astype(np.uint8) for i in range(2)])).cuda().repeat(B // 2 + 1, 1, 1)[:B].contiguous()
        bars = torch.tensor([[h // 8, h // 8]] * B, dtype=torch.int32, device="cuda")
        out_bars = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        out_fill = torch.empty_like(depth)
        gray = R.letterbox_stats(frames)["gray"]
        fns = dict(update=lambda: R.letterbox_track(frames, h, cooldown_frames=trk.cooldown_frames, out=out_bars),
                   stats=lambda: R.letterbox_stats(frames), canny=lambda: R.canny_u8(gray, 30, 90, want_counts=True),
                   fill=lambda: R.depth_letterbox_fill(depth, bars, out=out_fill))
        if pipe is not None:
            fns["forward"] = lambda: pipe.depth_frames_u8(frames)
        ms = {}
        for k, fn in fns.items():
            fn(); fn(); torch.cuda.synchronize()           # warm-up: code objects, workspaces, library selection
            ms[k] = [ev_ms(fn, a.iters) / B for _ in range(a.repeats)]
        med = {k: statistics.median(v) for k, v in ms.items()}
        fwd = spread(ms["forward"]) if "forward" in ms else "not measured"
        ratio = f"{med['update'] / med['forward']:.2f}" if "forward" in ms else "not measured"
        say(f"| {w}x{h} | {spread(ms['update'])} | {spread(ms['stats'])} | {spread(ms['canny'])} | {spread(ms['fill'])} | {fwd} | {ratio} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    R.close()


if __name__ == "__main__":
    main()
