"""Times RealESRGAN_x4plus (``Upscaler(..., "RealESRGAN_x4_fp16")._infer``) on the hand-written kernels (``rrdb_hip=True``) against the fp16 module graph on
MIOpen (``rrdb_hip=False``, find mode on): the same network, one process, the two configurations alternating, warm-up first, median and spread of N
forwards each.  Then the 192 -> 64 and 64 -> 32 layers alone (``vd3d_conv3x3_dense_f16`` vs MIOpen's convolution + leaky_relu on a dense tensor).
usage (GPU box): python tools/probe_rrdb.py [--n 12] [--sizes 480x270,960x540] [--json FILE]      results: profiles/r10_rrdb.md"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from visiondepth3d_amd.render_3d import Renderer
from visiondepth3d_amd.upscale import Upscaler, dense_weight_fragments

PEAK_TFLOPS = 2500.0          # MI355X dense fp16 MFMA peak
CL = torch.channels_last


def network_flops(h, w, blocks=23):
    """Multiply-adds x 2 of the convolutions the algorithm needs (conv_last counted with its 3 real output channels)."""
    rdb = 9 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64)
    lr = 27 * 64 + 3 * blocks * rdb + 9 * 64 * 64
    hr = 4 * 9 * 64 * 64 + 16 * 9 * 64 * 64 * 2 + 16 * 9 * 64 * 3
    return 2.0 * h * w * (lr + hr)


def timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e)


def stats(ts):
    q = statistics.quantiles(ts, n=4)
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), iqr_ms=q[2] - q[0], n=len(ts))


def alternate(fa, fb, n, warm=3):
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(n):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return stats(ta), stats(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--sizes", default="480x270,960x540")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_rrdb needs the GPU: a CPU timing says nothing about it")
    if args.n < 10:
        raise SystemExit("--n: at least 10 forwards per configuration")
    torch.backends.cudnn.benchmark = True          # MIOpen find mode: the library path at its best
    R = Renderer(0)
    torch.manual_seed(3)
    hip = Upscaler(R, "RealESRGAN_x4_fp16", rrdb_hip=True)
    lib = Upscaler(R, "RealESRGAN_x4_fp16", net=hip.net, rrdb_hip=False)
    assert hip._rrdb is not None and lib._rrdb is None
    res = {"device": torch.cuda.get_device_name(0), "network": [], "layers": []}
    for sz in args.sizes.split(","):
        w, h = (int(v) for v in sz.split("x"))
        frame = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda")
        d = (hip._infer(frame) - lib._infer(frame)).abs()             # faster and different is not faster
        sh, sl = alternate(lambda: hip._infer(frame), lambda: lib._infer(frame), args.n)
        fl = network_flops(h, w)
        spread = max(sh["max_ms"] - sh["min_ms"], sl["max_ms"] - sl["min_ms"])
        row = dict(size=sz, gflop=fl / 1e9, hip=sh, lib=sl, speedup=sl["median_ms"] / sh["median_ms"], gain_ms=sl["median_ms"] - sh["median_ms"], spread_ms=spread,
                   hip_tflops=fl / sh["median_ms"] / 1e9, hip_peak_share=fl / sh["median_ms"] / 1e9 / PEAK_TFLOPS, max_abs_diff=float(d.max()), mean_abs_diff=float(d.mean()))
        res["network"].append(row)
        print(f"RealESRGAN_x4plus {sz}: rrdb_hip=True {sh['median_ms']:.2f} ms (min {sh['min_ms']:.2f}, max {sh['max_ms']:.2f}) | rrdb_hip=False "
              f"{sl['median_ms']:.2f} ms (min {sl['min_ms']:.2f}, max {sl['max_ms']:.2f}) | x{row['speedup']:.2f}, gain {row['gain_ms']:.2f} ms vs spread {spread:.2f} ms | "
              f"{row['hip_tflops']:.0f} TFLOP/s end to end = {100 * row['hip_peak_share']:.1f} % of the fp16 peak | predictions differ by mean {row['mean_abs_diff']:.2e}, max {row['max_abs_diff']:.2e}",
              flush=True)
        del frame, d
        torch.cuda.empty_cache()
        for cin, cout in ((192, 64), (64, 32)):
            x = (torch.randn(1, 192, h, w, device="cuda") * 0.5).half().contiguous(memory_format=CL)
            y = torch.empty((1, 192, h, w), dtype=torch.float16, device="cuda").contiguous(memory_format=CL)
            wt = (torch.randn(cout, cin, 3, 3, device="cuda") * 0.03).half()
            b = torch.randn(cout, device="cuda") * 0.1
            wf, wc, bh = dense_weight_fragments(wt).cuda(), wt.contiguous(memory_format=CL), b.half()
            xd = x[:, :cin].contiguous(memory_format=CL)              # the library gets a dense tensor (what torch.cat hands it)
            reps = 20

            def f_hip():
                for _ in range(reps):
                    R.conv3x3_dense(x, cin, wf, b, cout, y, 64, slope=0.2)

            def f_lib():
                for _ in range(reps):
                    F.leaky_relu(F.conv2d(xd, wc, bh, padding=1), 0.2)
            kh, kl = alternate(f_hip, f_lib, args.n)
            fl = 2.0 * h * w * cin * cout * 9
            us_h, us_l = kh["median_ms"] / reps * 1e3, kl["median_ms"] / reps * 1e3
            lrow = dict(size=sz, cin=cin, cout=cout, hip_us=us_h, lib_us=us_l, hip_tflops=fl / us_h / 1e6, lib_tflops=fl / us_l / 1e6,
                        hip_peak_share=fl / us_h / 1e6 / PEAK_TFLOPS, hip_spread_us=(kh["max_ms"] - kh["min_ms"]) / reps * 1e3,
                        lib_spread_us=(kl["max_ms"] - kl["min_ms"]) / reps * 1e3)
            res["layers"].append(lrow)
            print(f"  layer {cin} -> {cout} {sz} (back to back, launch gaps included): hip {us_h:.1f} us = {lrow['hip_tflops']:.0f} TFLOP/s = {100 * lrow['hip_peak_share']:.1f} % of the fp16 peak | "
                  f"MIOpen conv + leaky_relu {us_l:.1f} us = {lrow['lib_tflops']:.0f} TFLOP/s", flush=True)
            del x, y, xd
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    R.close()


if __name__ == "__main__":
    main()
