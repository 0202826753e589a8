"""DepthPipe(gemm="fp16x2", conv="fp16x2", self_contained=True) beside the mode it completes (gemm="fp16x2", conv=None, miopen_find=True), DA-V2-Base,
16 frames at 3840 x 2160 -- tools/probe_self_contained.py for the fp16x2 pair:

  python tools/probe_fp16x2_self_contained.py --forward [--out FILE.md]   both pipes in one process, alternating windows (three windows of three forwards after
                                                                          warm-up, device events, spread stated), and the device time per kernel of one forward
  python tools/probe_fp16x2_self_contained.py --cold library|self         wall time from process start to the end of the first forward, in THIS fresh process
  rocprofv3 --kernel-trace --stats -- python tools/probe_fp16x2_self_contained.py --run library|self   two warm-up forwards and three more, nothing else: the
                                                                          process a kernel-trace run profiles (its own run: no timing is taken in it)
  python tools/probe_fp16x2_self_contained.py --shapes                    vd3d_conv3x3_s1_x2 on the neck / fusion / head shapes of DA-V2-Small, -Base and -Large at
                                                                          the 4K patch grid, one frame and sixteen, beside the float32 library convolution (MIOpen
                                                                          find mode on): the table CONV_X2_MIN_TILES (visiondepth3d_amd/depth.py) is read from"""
import time

T0 = time.perf_counter()   # process start, as near as a script can see it (the interpreter's own start-up is in front of it)

import argparse  # noqa: E402
import os  # noqa: E402
import statistics  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visiondepth3d_amd.depth import DepthPipe  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402

F = torch.nn.functional
NAME, B, H, W = "depth-anything-v2-base", 16, 2160, 3840
MODES = {"library": dict(conv=None, miopen_find=True), "self": dict(conv="fp16x2", self_contained=True)}
# (neck hidden sizes, fusion width) per model; the 4K patch grid is 37 x 66: neck.convs at 148 x 264, 74 x 132, 37 x 66, 19 x 33, the fusion units at the same
# four maps, head.conv1 at 296 x 528 (fusion -> fusion / 2), head.conv2 at 518 x 924 (fusion / 2 -> 32)
MODELS = {"small": ((48, 96, 192, 384), 64), "base": ((96, 192, 384, 768), 128), "large": ((256, 512, 1024, 1024), 256)}
MAPS = ((148, 264), (74, 132), (37, 66), (19, 33))


def bench(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def frames():
    from visiondepth3d_amd import synth
    return torch.from_numpy(synth.synth_frame(0, H, W)[0]).cuda()[None].expand(B, -1, -1, -1).contiguous()


def pipe(R, mode):
    return DepthPipe(NAME, device="cuda", dtype=torch.float32, renderer=R, gemm="fp16x2", **MODES[mode])


def probe_forward(R, say, windows=3, steps=3):
    f = frames()
    pipes = {m: pipe(R, m) for m in MODES}
    for p in pipes.values():   # warm-up of every shape (MIOpen find, the weight packs, the position embedding)
        p.infer_bgr_u8(f, raw=True); p.infer_bgr_u8(f, raw=True)
    ms = {m: [] for m in pipes}
    for _ in range(windows):   # the two modes alternate in one process
        for m, p in pipes.items():
            ms[m].append(bench(lambda: p.infer_bgr_u8(f, raw=True), steps))
    for m, v in ms.items():
        say(f"- {NAME}, {B} frames at {W} x {H}, gemm=fp16x2, {m} ({MODES[m]}): median {statistics.median(v):.2f} ms per forward, windows "
            f"{', '.join(f'{t:.2f}' for t in v)} (spread {max(v) - min(v):.2f})")
    a, b = statistics.median(ms["self"]), statistics.median(ms["library"])
    say(f"- self-contained / library = {a / b:.4f} ({a - b:+.2f} ms)")
    from torch.profiler import ProfilerActivity, profile
    for m, p in pipes.items():
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            p.infer_bgr_u8(f, raw=True); torch.cuda.synchronize()
        rows = sorted(((e.key, e.device_time_total / 1e3, e.count) for e in prof.key_averages() if e.device_time_total > 0), key=lambda r: -r[1])
        say(f"- {m}: device time of one forward by kernel (ms, launches), the sixteen largest of {len(rows)}; total {sum(r[1] for r in rows):.2f} ms")
        for k, t, n in rows[:16]:
            say(f"  - `{k[:90]}` {t:.3f} ({n})")


def probe_cold(R, say, mode):
    f = frames()
    p = pipe(R, mode)
    p.infer_bgr_u8(f, raw=True); torch.cuda.synchronize()
    say(f"- cold start, {mode}: {time.perf_counter() - T0:.1f} s from process start to the end of the first forward ({NAME}, {B} frames at {W} x {H}, gemm=fp16x2)")


def probe_run(R, say, mode):
    f = frames()
    p = pipe(R, mode)
    for _ in range(5):
        p.infer_bgr_u8(f, raw=True)
    torch.cuda.synchronize()
    say(f"- {mode}: five forwards done")


def probe_shapes(R, say):
    torch.backends.cudnn.benchmark = True
    g = torch.Generator(device="cuda").manual_seed(1)
    say("| model | module | H x W x Cin -> Cout | tiles per frame | B | conv3x3_s1_x2 ms | library f32 ms | x2 / library |")
    say("|---|---|---|---|---|---|---|---|")
    for model, (neck, fw) in MODELS.items():
        shapes = [(f"neck.convs.{i}", h, w, c, fw) for i, ((h, w), c) in enumerate(zip(MAPS, neck))]
        shapes += [("fusion unit", h, w, fw, fw) for h, w in MAPS]
        shapes += [("head.conv1", 296, 528, fw, fw // 2), ("head.conv2", 518, 924, fw // 2, 32)]
        for what, h, w, cin, cout in shapes:
            wt = torch.randn(cout, cin, 3, 3, device="cuda", generator=g) * 0.05
            img = R.conv3x3_s1_x2_pack(wt)
            for nb in (1, 16):
                x = torch.relu(torch.randn(nb, cin, h, w, device="cuda", generator=g)).contiguous(memory_format=torch.channels_last)
                fn2, fn32 = (lambda: R.conv3x3_s1_x2(x, img, cout)), (lambda: F.conv2d(x, wt, None, 1, 1))
                fn2(); fn2(); fn32(); fn32()
                n = 20 if nb * h * w < 200000 else 5
                t2, t32 = min(bench(fn2, n), bench(fn2, n)), min(bench(fn32, n), bench(fn32, n))
                say(f"| {model} | {what} | {h} x {w} x {cin} -> {cout} | {((h + 7) // 8) * ((w + 31) // 32)} | {nb} | {t2:.3f} | {t32:.3f} | {t2 / t32:.2f} |")
                del x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--cold", choices=list(MODES))
    ap.add_argument("--run", choices=list(MODES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def say(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")
    R = Renderer(0)
    if a.cold:
        probe_cold(R, say, a.cold)
    if a.run:
        probe_run(R, say, a.run)
    if a.shapes:
        probe_shapes(R, say)
    if a.forward:
        probe_forward(R, say)
    R.close()


if __name__ == "__main__":
    main()
