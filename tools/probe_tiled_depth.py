"""Tiled high-resolution depth (DepthPipe.depth_frames_u8(tiled=True)) measured on one GPU: float32, synthetic weights, tile 512, pad 32.

  per model (DA-V2-Small, DA-V2-Base) and frame size (1080p, 4K), ms per frame, three repeats each (median, min .. max):
    tiled          depth_frames_u8(tiled=True) at tile_batch 1, 4 and 16
    protocol loop  the reference's structure on the same GPU: one tile per forward through pipe([tile], inference_size=(cws, chs)), host blend
                   (numpy), numpy hand-off; the tiles are cut on the host from the frame (wall clock, the loop synchronises per tile)
    non-tiled      depth_frames_u8(frames): one ~518-pixel window
  per kernel (gather, blend with the fused bicubic, normalise): device-event time, the bytes it must move, the share of HBM bandwidth

  python tools/probe_tiled_depth.py [--models small,base] [--sizes 1080,2160] [--repeats 3] [--out FILE.md]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visiondepth3d_amd import depth_tiles as DT  # noqa: E402
from visiondepth3d_amd import synth  # noqa: E402
from visiondepth3d_amd.depth import DepthPipe  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X data sheet
TILE, PAD = 512, 32


def ev_ms(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def spread(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def protocol_loop(pipe, frame_np):
    """infer_depth_tile's structure: host crops, one forward per tile through the reference protocol, host blend and hand-off"""
    H, W = frame_np.shape[:2]
    plan = DT.tile_plan(H, W, TILE, PAD)
    centres = []
    for t in plan.tiles:
        crop = torch.from_numpy(np.ascontiguousarray(frame_np[t.yp0:t.yp1, t.xp0:t.xp1])).cuda()
        if (t.ch, t.cw) != (t.chs, t.cws):
            crop = pipe.renderer.resize_cubic_u8(crop, t.chs, t.cws)
        rgb = crop.flip(-1).cpu().numpy()
        p = pipe([rgb], inference_size=(t.cws, t.chs))[0]["predicted_depth"].cpu().numpy()
        centres.append(p[t.yc0:t.yc0 + t.th, t.xc0:t.xc0 + t.tw])
    with np.errstate(all="ignore"):
        return DT.normalize_to_u8_numpy(DT.blend_tiles_numpy(plan, centres))


def kernels(R, pipe, say, H, W, repeats):
    plan = DT.tile_plan(H, W, TILE, PAD)
    frames = torch.from_numpy(synth.synth_frame(0, H, W)[0])[None].cuda()
    th, tw = pipe.resize_target(588, 588)
    # gather: every group once (reads the crops, writes the tiles)
    orgs = [torch.from_numpy(plan.gather_origins(g, 1)).cuda() for g in plan.groups]
    outs = [torch.empty((len(g.tiles), g.chs, g.cws, 3), dtype=torch.uint8, device="cuda") for g in plan.groups]

    def gather():
        for g, o, out in zip(plan.groups, orgs, outs):
            R.tile_gather_cubic_u8(frames, o, g.ch, g.cw, g.chs, g.cws, out=out)
    g_bytes = sum(len(g.tiles) * 3 * (g.ch * g.cw + g.chs * g.cws) for g in plan.groups)
    # blend with the fused bicubic from the network's output size (reads predictions + weights, writes the plane)
    shapes = [pipe.resize_target(g.chs, g.cws) for g in plan.groups]
    tab, off, total = plan.blend_tables(1, shapes)
    pool = torch.randn(total, device="cuda")
    tab, off, wp = torch.from_numpy(tab).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(plan.weight_pool()).cuda()
    out = torch.empty((1, H, W), dtype=torch.float32, device="cuda")

    def blend():
        R.tile_blend(pool, off, tab, wp, 1, H, W, TILE, PAD, out=out)
    b_bytes = 4 * (total + sum(t.th * t.tw for t in plan.tiles) + H * W)
    u8 = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")

    def norm():
        R.depth_normalize_pclip(out, out=u8)
    n_bytes = H * W * (5 * 4 + 1)   # four digit passes and the apply pass read the plane, one byte written
    for name, fn, nb in (("gather (all groups)", gather, g_bytes), ("blend, fused bicubic", blend, b_bytes), ("normalise (5 passes)", norm, n_bytes)):
        fn(); fn(); torch.cuda.synchronize()
        ms = [ev_ms(fn, 10) for _ in range(repeats)]
        m = statistics.median(ms)
        say(f"| {W}x{H} | {name} | {spread(ms)} | {nb / 1e6:.1f} | {nb / (m * 1e-3) / 1e12:.2f} | {100 * nb / (m * 1e-3) / HBM_PEAK:.0f} % |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="small,base")
    ap.add_argument("--sizes", default="1080,2160")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true", help="skip the one-tile-at-a-time protocol loop")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    R = Renderer(0)
    sizes = [(int(h), int(h) * 16 // 9) for h in a.sizes.split(",")]
    say(f"device: {torch.cuda.get_device_name(0)}; float32, synthetic weights, tile {TILE}, pad {PAD}; ms per frame, median (min .. max) of {a.repeats}")
    say("")
    say("| model | frame | tiles (shapes) | tiled, tile_batch 1 | tile_batch 4 | tile_batch 16 | protocol loop (one tile per forward) | non-tiled |")
    say("|---|---|---|---|---|---|---|---|")
    pipe = None
    for m in a.models.split(","):
        pipe = DepthPipe(f"depth-anything-v2-{m}", device="cuda", dtype=torch.float32, renderer=R)
        for H, W in sizes:
            plan = DT.tile_plan(H, W, TILE, PAD)
            frame_np = synth.synth_frame(0, H, W)[0]
            frames = torch.from_numpy(frame_np)[None].cuda()
            cols = []
            for tb in (1, 4, 16):
                fn = lambda tb=tb: pipe.depth_frames_u8(frames, tiled=True, tile=TILE, pad=PAD, tile_batch=tb)
                fn(); torch.cuda.synchronize()   # warm-up: library selection per batch shape
                cols.append(spread([ev_ms(fn) for _ in range(a.repeats)]))
            if a.no_loop:
                cols.append("not measured")
            else:
                protocol_loop(pipe, frame_np)
                ts = []
                for _ in range(a.repeats):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    protocol_loop(pipe, frame_np)
                    torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
                cols.append(spread(ts))
            fn = lambda: pipe.depth_frames_u8(frames)
            fn(); torch.cuda.synchronize()
            cols.append(spread([ev_ms(fn) for _ in range(a.repeats)]))
            say(f"| DA-V2-{m.capitalize()} | {W}x{H} | {plan.n_tiles} ({len(plan.groups)}) | " + " | ".join(cols) + " |")
    say("")
    say("| frame | kernel | ms, median (min .. max) | bytes it must move (MB) | TB/s | share of 8 TB/s |")
    say("|---|---|---|---|---|---|")
    for H, W in sizes:
        kernels(R, pipe, say, H, W, a.repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    R.close()


if __name__ == "__main__":
    main()
