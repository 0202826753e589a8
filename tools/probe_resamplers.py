"""The depth leg's three resampling kernels at the headline's shapes (4K, 16 frames, DA-V2-Base at 518 x 924), device events, median (min .. max) ms per call.

  default      hand-off (16 x 518 x 924 -> 2160 x 3840 u8) and input prep (16 x 2160 x 3840 x 3 u8 -> 518 x 924 x 3 f32): forms 1 (general) and 2 (fast)
               alternate in one process; per kernel the fast form's saving beside the larger (max - min) spread, and whether the two forms gave the same bits
  --upsample   the four float32 up-samplings of the DPT neck (128 channels, 19 x 33 -> ... -> 296 x 528, bias fused) with whatever library is loaded: the old
               body has no form, so two libraries are compared in alternating processes (VD3D_LIB_PATH=<the other build> python tools/probe_resamplers.py --upsample)

Beside each time: the traffic the result needs over the measured 6.29 TB/s copy rate and the float32 lane-operations it needs over the measured 50.2 T/s
(profiles/r03_ubench_valu.md), and which of the two is the larger.
Usage: python tools/probe_resamplers.py [--rounds N] [--upsample]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402

COPY_TBS, LANE_TOPS = 6.29, 50.2


def _time(runs, rounds):
    for f in runs.values():   # warm-up
        f(); f()
    torch.cuda.synchronize()
    ms = {n: [] for n in runs}
    for _ in range(rounds):
        for n, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            torch.cuda.synchronize()
            ms[n].append(e0.elapsed_time(e1))
    return {n: dict(ms=round(sorted(v)[len(v) // 2], 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for n, v in ms.items()}


def _floor(nbytes, lane_ops):
    mem, alu = nbytes / (COPY_TBS * 1e9), lane_ops / (LANE_TOPS * 1e9)
    return dict(mem_floor_ms=round(mem, 4), valu_floor_ms=round(alu, 4), binds="memory" if mem >= alu else "valu")


def _pair(row, general, fast):
    g, f = row[general], row[fast]
    row["fast_saves_ms"] = round(g["ms"] - f["ms"], 4)
    row["larger_spread_ms"] = round(max(g["max_ms"] - g["min_ms"], f["max_ms"] - f["min_ms"]), 4)
    row["clears_3x_spread"] = bool(row["fast_saves_ms"] > 3 * row["larger_spread_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--upsample", action="store_true")
    args = ap.parse_args()
    R = Renderer(0)
    B, H, W, th, tw = 16, 2160, 3840, 518, 924
    g = torch.Generator(device="cuda").manual_seed(1)
    if args.upsample:
        C = 128
        for ih, iw in [(19, 33), (37, 66), (74, 132), (148, 264)]:
            oh, ow = (37, 66) if ih == 19 else (2 * ih, 2 * iw)
            x = torch.randn(B, ih, iw, C, device="cuda", generator=g).permute(0, 3, 1, 2)
            bias = torch.randn(C, device="cuda", generator=g)
            row = dict(kernel="upsample_bilinear_bias_f32", B=B, C=C, src=[ih, iw], dst=[oh, ow], lib=os.environ.get("VD3D_LIB_PATH", "in-tree"))
            row.update(_time({"upsample": lambda: R.upsample_bilinear_bias(x, (oh, ow), bias)}, args.rounds)["upsample"])
            # every output element written once, every input element read once; 4 taps x (2 mul + 1 add) folded + the bias: ~8 lane-operations per element
            row.update(_floor(4.0 * B * C * (oh * ow + ih * iw), 8.0 * B * C * oh * ow))
            print(json.dumps(row), flush=True)
        R.close()
        return
    pred = torch.randn(B, th, tw, device="cuda", generator=g) * 3 + 5
    out = torch.empty(B, H, W, dtype=torch.uint8, device="cuda")
    row = dict(kernel="depth_handoff", src=[th, tw], dst=[H, W], B=B)
    row.update(_time({"general": lambda: R.depth_handoff(pred, H, W, out=out, form=1), "separable": lambda: R.depth_handoff(pred, H, W, out=out, form=2)}, args.rounds))
    _pair(row, "general", "separable")
    row["same_bits"] = bool(torch.equal(R.depth_handoff(pred, H, W, form=1), R.depth_handoff(pred, H, W, form=2)))
    # both passes: the plane written once, the prediction read twice; per output pixel and pass ~4 mul + 4 add of the vertical sum, ~10 of the coefficients
    # shared by 4 columns, the horizontal sums once per prediction row and column (8 per 4.17 rows), ~8 to normalise and pack in the second pass
    row.update(_floor(B * H * W + 2 * 4.0 * B * th * tw, B * H * W * (2 * (8 + 10 / 4 + 8 / 4.17) + 8)))
    print(json.dumps(row), flush=True)
    frames = torch.randint(0, 256, (B, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
    row = dict(kernel="depth_preprocess_f32", src=[H, W], dst=[th, tw], B=B)
    prep = lambda form: R.depth_preprocess(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.float32, form=form)  # noqa: E731
    row.update(_time({"tile": lambda: prep(1), "strip": lambda: prep(2)}, args.rounds))
    _pair(row, "tile", "strip")
    row["same_bits"] = bool(torch.equal(prep(1), prep(2)))
    # every input byte read once, the result written once; horizontal: every input row x output column x ~17.6 taps x 3 channels x (convert, multiply, add),
    # vertical: every output element x ~17.7 taps x (multiply, add)
    taps_w, taps_h = 4.0 * W / tw + 1, 4.0 * H / th + 1
    row.update(_floor(3.0 * B * H * W + 12.0 * B * th * tw, B * 3.0 * (H * tw * taps_w * 3 + th * tw * taps_h * 2)))
    print(json.dumps(row), flush=True)
    R.close()


if __name__ == "__main__":
    main()
