"""DepthPipe(self_contained=True) beside the library mode it leaves (the same gemm / conv pair with miopen_find=True), 16 frames at 3840 x 2160.  ``--model`` takes
any name of depth.MODEL_ZOO (default depth-anything-v2-base; dpt-large and the metric Depth-Anything names included), ``--pair`` bf16x3 (default) or fp16x2:

  python tools/probe_self_contained.py --forward [--out FILE.md]     both pipes in one process, alternating windows (three windows of three forwards after
                                                                     warm-up, device events, spread stated), and a per-kernel-family breakdown of the mode
  python tools/probe_self_contained.py --cold library|self           wall time from process start to the end of the first forward, in THIS fresh process
  python tools/probe_self_contained.py --shapes                      vd3d_conv3x3_s2_x3 at 16 x 37 x 66 for 384 / 768 / 1024 channels beside the float32 library
                                                                     convolution (MIOpen find mode on)"""
import time

T0 = time.perf_counter()   # process start, as near as a script can see it (the interpreter's own start-up is in front of it)

import argparse  # noqa: E402
import os  # noqa: E402
import statistics  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visiondepth3d_amd.depth import MODEL_ZOO, DepthPipe  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402

F = torch.nn.functional
NAME, PAIR, B, H, W = "depth-anything-v2-base", "bf16x3", 16, 2160, 3840   # --model / --pair replace the first two
MODES = {"library": dict(miopen_find=True), "self": dict(self_contained=True)}


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
    return DepthPipe(NAME, device="cuda", dtype=torch.float32, renderer=R, gemm=PAIR, conv=PAIR, seed=5 if NAME == "dpt-large" else 0, **MODES[mode])


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
        say(f"- {NAME}, {B} frames at {W} x {H}, gemm={PAIR}, conv={PAIR}, {m}: median {statistics.median(v):.2f} ms per forward, windows "
            f"{', '.join(f'{t:.2f}' for t in v)} (spread {max(v) - min(v):.2f})")
    a, b = statistics.median(ms["self"]), statistics.median(ms["library"])
    say(f"- self-contained / library = {a / b:.4f} ({a - b:+.2f} ms)")
    routes = pipes["library"].conv_routes
    say(f"- library mode: {sorted(k for k, v in routes.items() if v[0] == 'library')} of its {len(routes)} 3 x 3 convolutions on the library by the size rule")
    # where the mode's time goes: device time per kernel family of one forward of each pipe (torch.profiler; names of this library's kernels start with k_)
    from torch.profiler import ProfilerActivity, profile
    for m, p in pipes.items():
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            p.infer_bgr_u8(f, raw=True); torch.cuda.synchronize()
        rows = sorted(((e.key, e.device_time_total / 1e3, e.count) for e in prof.key_averages() if e.device_time_total > 0), key=lambda r: -r[1])
        say(f"- {m}: device time of one forward by kernel (ms, launches), the twelve largest of {len(rows)}; total {sum(r[1] for r in rows):.2f} ms")
        for k, t, n in rows[:12]:
            say(f"  - `{k[:90]}` {t:.3f} ({n})")


def probe_cold(R, say, mode):
    f = frames()
    p = pipe(R, mode)
    p.infer_bgr_u8(f, raw=True); torch.cuda.synchronize()
    say(f"- cold start, {mode}: {time.perf_counter() - T0:.1f} s from process start to the end of the first forward ({NAME}, gemm={PAIR}, conv={PAIR}, {B} frames at {W} x {H})")


def probe_shapes(R, say):
    torch.backends.cudnn.benchmark = True
    g = torch.Generator(device="cuda").manual_seed(1)
    say("| B x H x W x C -> C | workgroups (tiles x slices) | conv3x3_s2_x3 ms | library f32 ms | x3 / library |")
    say("|---|---|---|---|---|")
    for Cc in (384, 768, 1024):
        x = torch.relu(torch.randn(16, Cc, 37, 66, device="cuda", generator=g)).contiguous(memory_format=torch.channels_last)
        w = torch.randn(Cc, Cc, 3, 3, device="cuda", generator=g) * 0.05
        img = R.conv3x3_s2_x3_pack(w)
        fn3, fn32 = (lambda: R.conv3x3_s2_x3(x, img, Cc)), (lambda: F.conv2d(x, w, None, 2, 1))
        fn3(); fn3(); fn32(); fn32()
        t3, t32 = bench(fn3, 10), bench(fn32, 10)
        say(f"| 16 x 37 x 66 x {Cc} -> {Cc} | {16 * 3 * 2} x {Cc // 128} | {t3:.3f} | {t32:.3f} | {t3 / t32:.2f} |")


def main():
    global NAME, PAIR
    ap = argparse.ArgumentParser()
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--cold", choices=list(MODES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default=NAME, choices=sorted(MODEL_ZOO))
    ap.add_argument("--pair", default=PAIR, choices=["bf16x3", "fp16x2"])
    a = ap.parse_args()
    NAME, PAIR = a.model, a.pair

    def say(s):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")
    R = Renderer(0)
    if a.cold:
        probe_cold(R, say, a.cold)
    if a.shapes:
        probe_shapes(R, say)
    if a.forward:
        probe_forward(R, say)
    R.close()


if __name__ == "__main__":
    main()
