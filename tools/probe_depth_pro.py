"""Measurements behind profiles/r25_depth_pro.md: DepthPro's two kernels alone (time, bytes moved, fraction of the stream-copy yardstick measured in the same
process) and the 1536 x 1536 forward of DepthPipe("depth-pro") at one frame and four, beside the stock path (processor and post-process as ATen operators around the
same module) in the same process, runs alternating.  Medians of ROUNDS rounds, the spread as min .. max.  Prints one JSON line per measurement.

    python tools/probe_depth_pro.py kernels
    python tools/probe_depth_pro.py forward [--frames 1 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

T0 = time.time()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ROUNDS = 7


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def rounds(fns, iters, warm=3):
    """Alternating rounds over the callables -> {name: (median ms, min, max)}."""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            got[k].append(timed(f, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def kernels():
    from visiondepth3d_amd import _lib
    from visiondepth3d_amd.render_3d import Renderer, _ptr
    R = Renderer(0)
    n = 256 << 20
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    copy = rounds({"copy": lambda: _lib.check(R._L.vd3d_stream_copy(R._ctx, _ptr(src), _ptr(dst), n))}, 20)["copy"]
    bw = 2 * n / (copy[0] * 1e-3)
    print(json.dumps(dict(what="stream_copy_256MiB", ms=copy, bytes_per_s=bw)))
    fr = torch.randint(0, 256, (1, 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    fr8 = torch.randint(0, 256, (8, 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    fr_small = torch.randint(0, 256, (1, 540, 960, 3), dtype=torch.uint8, device="cuda")
    fr_4k = torch.randint(0, 256, (1, 2160, 3840, 3), dtype=torch.uint8, device="cuda")
    pred, fov = torch.rand(1, 1536, 1536, device="cuda") * 10 + 0.5, torch.tensor([55.0], device="cuda")
    half = (0.5, 0.5, 0.5)
    cases = {
        "preprocess_1080p_to_1536": (lambda: R.depthpro_preprocess(fr, 1536, half, half), fr.numel() + 3 * 1536 * 1536 * 4),
        "preprocess_540p_to_1536": (lambda: R.depthpro_preprocess(fr_small, 1536, half, half), fr_small.numel() + 3 * 1536 * 1536 * 4),
        "preprocess_4k_to_1536": (lambda: R.depthpro_preprocess(fr_4k, 1536, half, half), fr_4k.numel() + 3 * 1536 * 1536 * 4),
        "preprocess_8x1080p_to_1536": (lambda: R.depthpro_preprocess(fr8, 1536, half, half), fr8.numel() + 8 * 3 * 1536 * 1536 * 4),   # (past the launch floor)
        "post_1536_to_1080p_fov": (lambda: R.depthpro_post(pred, fov, 1080, 1920), pred.numel() * 4 + 1080 * 1920 * 4),
        "post_1536_raw_fov": (lambda: R.depthpro_post(pred, fov, 1536, 1536), pred.numel() * 8),
    }
    for name, (fn, nbytes) in cases.items():
        ms = rounds({name: fn}, 50)[name]
        print(json.dumps(dict(what=name, ms=ms, bytes=nbytes, bytes_per_s=nbytes / (ms[0] * 1e-3), of_stream_copy=nbytes / (ms[0] * 1e-3) / bw)))
    R.close()


def forward(frames):
    from visiondepth3d_amd import depth_pro
    from visiondepth3d_amd.depth import DepthPipe
    from visiondepth3d_amd.render_3d import Renderer
    R = Renderer(0)
    t = time.time()
    pipe = DepthPipe("depth-pro", renderer=R)
    built = time.time()
    fr = torch.randint(0, 256, (max(frames), 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    pipe.infer_bgr_u8(fr[:1])
    torch.cuda.synchronize()
    print(json.dumps(dict(what="start_to_first_forward", import_s=t - T0, construct_s=built - t, first_forward_s=time.time() - built, total_s=time.time() - T0,
                          params=pipe.n_params)))
    half = (0.5, 0.5, 0.5)

    @torch.no_grad()
    def stock(f):
        out = pipe.model(pixel_values=depth_pro.preprocess_statement(f, (1536, 1536), half, half))
        return depth_pro.post_statement(out.predicted_depth, out.field_of_view, f.shape[1], f.shape[2])

    @torch.no_grad()
    def net(x):
        return pipe.model(pixel_values=x).predicted_depth
    for B in frames:
        f = fr[:B]
        x = R.depthpro_preprocess(f, 1536, half, half)
        r = rounds({"pipe": lambda: pipe.infer_bgr_u8(f), "stock": lambda: stock(f), "network_alone": lambda: net(x)}, 2, warm=1)
        print(json.dumps(dict(what=f"forward_1536_f32_B{B}", ms=r)))
    R.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "forward"])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4])
    a = ap.parse_args()
    kernels() if a.what == "kernels" else forward(a.frames)
