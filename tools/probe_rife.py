"""Times the interpolation network: ``RifeSession("cuda")`` (the float32 module graph on MIOpen, find mode on) against ``RifeSession("cuda", renderer=R,
conv="bf16x3")`` (every convolution on ``vd3d_conv_ifn``, the glue on the ``vd3d_rife_*`` kernels): the same weights, one process, the two sessions alternating,
warm-up first; three alternating runs of N calls each, the median of the three run medians and their spread.  Then the 96 -> 96 3 x 3 layer alone at the three
block sizes, the MFMA work the channel padding wastes, and the per-stage share of one forward (``vd3d_set_profiling``).
``--one lib|hip`` runs ONE session a few times and exits: the process to put behind ``rocprofv3 --kernel-trace --stats --``.
usage (GPU box): python tools/probe_rife.py [--n 10] [--sizes 1920x1080,480x270] [--batches 1,2] [--json FILE]      results: profiles/r11_rife_x3.md"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from visiondepth3d_amd import _abi
from visiondepth3d_amd.render_3d import Renderer
from visiondepth3d_amd.rife import RifeSession, ifnet_plan

PEAK_TFLOPS = 2500.0          # MI355X dense bf16 MFMA peak


def timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e)


def alternate(fa, fb, n, runs=3, warm=3):
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    ma, mb = [], []
    for _ in range(runs):
        ta, tb = [], []
        for _ in range(n):
            ta.append(timed(fa))
            tb.append(timed(fb))
        ma.append(statistics.median(ta))
        mb.append(statistics.median(tb))
    return (dict(median_ms=statistics.median(ma), runs_ms=ma, spread_ms=max(ma) - min(ma)), dict(median_ms=statistics.median(mb), runs_ms=mb, spread_ms=max(mb) - min(mb)))


def mac_census(net, h, w):
    """Multiply-adds of one forward at h x w (padded to multiples of 32): what the module needs and what the padded launches issue."""
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    real = issued = 0
    for L, s in zip(ifnet_plan(net), (4, 2, 1)):
        hs, ws = hp // s, wp // s
        opix = [hs // 2 * (ws // 2), hs // 4 * (ws // 4)] + [hs // 4 * (ws // 4)] * 8 + [hs // 2 * (ws // 2), hs * ws]
        for ly, px in zip(L, opix):
            taps = 4 if ly["kind"] == _abi.IFN_T4S2 else 9          # per output pixel
            real += px * taps * ly["real"][0] * ly["real"][1]
            issued += px * taps * ly["cin"] * ly["cout"]
    return real, issued


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--sizes", default="1920x1080,480x270")
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--json", default=None)
    ap.add_argument("--one", choices=("lib", "hip"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_rife needs the GPU: a CPU timing says nothing about it")
    torch.backends.cudnn.benchmark = True          # MIOpen find mode: the library path at its best
    R = Renderer(0)
    lib = RifeSession("cuda")
    hip = RifeSession("cuda", renderer=R, conv="bf16x3")
    if args.one:
        w, h = (int(v) for v in args.sizes.split(",")[0].split("x"))
        x = torch.rand(1, 6, h, w, device="cuda")
        s = lib if args.one == "lib" else hip
        for _ in range(5):
            s(x)
        torch.cuda.synchronize()
        R.close()
        return
    res = {"device": torch.cuda.get_device_name(0), "network": [], "layers": [], "stages": []}
    for sz in args.sizes.split(","):
        w, h = (int(v) for v in sz.split("x"))
        real, issued = mac_census(lib.net, h, w)
        for nb in (int(v) for v in args.batches.split(",")):
            x = torch.rand(nb, 6, h, w, device="cuda")
            d = (hip(x) - lib(x)).abs()                                   # faster and different is not faster
            sl, sh = alternate(lambda: lib(x), lambda: hip(x), args.n)
            spread = max(sl["spread_ms"], sh["spread_ms"])
            fl = 2.0 * nb * real * 6                                      # six bf16 MFMA products per MAC
            row = dict(size=sz, batch=nb, lib=sl, hip=sh, speedup=sl["median_ms"] / sh["median_ms"], gain_ms=sl["median_ms"] - sh["median_ms"], spread_ms=spread,
                       real_gmac=nb * real / 1e9, issued_gmac=nb * issued / 1e9, padding_waste=issued / real - 1.0, hip_mfma_tflops=fl / sh["median_ms"] / 1e9,
                       max_abs_diff=float(d.max()), mean_abs_diff=float(d.mean()))
            res["network"].append(row)
            print(f"IFNet {sz} batch {nb}: MIOpen f32 {sl['median_ms']:.2f} ms (runs {', '.join(f'{v:.2f}' for v in sl['runs_ms'])}) | bf16x3 {sh['median_ms']:.2f} ms "
                  f"(runs {', '.join(f'{v:.2f}' for v in sh['runs_ms'])}) | x{row['speedup']:.2f}, gain {row['gain_ms']:.2f} ms vs spread {spread:.2f} ms | "
                  f"{row['real_gmac']:.1f} GMAC needed, {row['issued_gmac']:.1f} issued (+{100 * row['padding_waste']:.1f} % padding) | "
                  f"predictions differ by mean {row['mean_abs_diff']:.2e}, max {row['max_abs_diff']:.2e}", flush=True)
        # per stage of one bf16x3 forward
        x = torch.rand(1, 6, h, w, device="cuda")
        R._L.vd3d_set_profiling(R._ctx, 1)
        hip(x)
        torch.cuda.synchronize()
        R._L.vd3d_sync(R._ctx)
        st = {k: (float(R._L.vd3d_last_stage_ms(R._ctx, k.encode())), int(R._L.vd3d_stage_calls(R._ctx, k.encode()))) for k in ("conv_ifn", "rife_glue")}
        R._L.vd3d_set_profiling(R._ctx, 0)
        res["stages"].append(dict(size=sz, stages=st))
        print(f"  stages {sz} (last launch ms, launches so far): {st}", flush=True)
        # the 96 -> 96 layer alone at the three block sizes
        hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
        for s in (1, 2, 4):
            fh, fw = hp // s // 4, wp // s // 4
            ly = hip._layers[0][2]
            xa = torch.randn(1, fh, fw, 96, device="cuda").permute(0, 3, 1, 2)
            ya = torch.empty(1, fh, fw, 96, device="cuda").permute(0, 3, 1, 2)
            reps = 20

            def f():
                for _ in range(reps):
                    R.conv_ifn(_abi.IFN_K3S1, xa, 96, ly["img"], ly["b"], ly["slope"], 96, ya)
            for _ in range(3):
                f()
            ts = [timed(f) for _ in range(args.n)]
            us = statistics.median(ts) / reps * 1e3
            fl = 2.0 * fh * fw * 96 * 96 * 9 * 6
            tiles = ((fh + 7) // 8) * ((fw + 31) // 32)
            lrow = dict(size=sz, scale=s, map=f"{fw}x{fh}", tiles=tiles, us=us, mfma_tflops=fl / us / 1e6, peak_share=fl / us / 1e6 / PEAK_TFLOPS,
                        spread_us=(max(ts) - min(ts)) / reps * 1e3)
            res["layers"].append(lrow)
            print(f"  layer 96 -> 96 k3s1 {fw}x{fh} ({tiles} tiles, back to back, launch gaps included): {us:.1f} us = {lrow['mfma_tflops']:.0f} TFLOP/s of bf16 MFMA "
                  f"(six products per MAC) = {100 * lrow['peak_share']:.1f} % of the peak", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    R.close()


if __name__ == "__main__":
    main()
