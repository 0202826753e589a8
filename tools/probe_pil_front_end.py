"""The Pillow-exact depth front end (vd3d_depth_preprocess_pil) beside the float front end's two kernels, isolated, device events, median (min .. max) ms
per call, the method of tools/probe_resamplers.py: the calls alternate in one process.

  4K      16 x 2160 x 3840 x 3 u8 -> 518 x 924 x 3 float32: k_pil_resample (one launch), k_depth_prep_strip (form 2), k_depth_prep (form 1)
  1080p   16 x 1080 x 1920 through inference_size = (896, 512): two launches of k_pil_resample (-> 512 x 896 u8 -> 518 x 910 float32); the float front
          end has no kernel for an inference size, so its one-launch form at 1080p -> 518 x 924 stands beside it for scale only

Usage: python tools/probe_pil_front_end.py [--rounds N]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visiondepth3d_amd import pil_resample  # noqa: E402
from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD, dpt_resize_target  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402


def _time(runs, rounds):
    for f in runs.values():   # warm-up (and the one-time table upload of a geometry)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    R = Renderer(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    B, H, W, th, tw = 16, 2160, 3840, 518, 924
    frames = torch.randint(0, 256, (B, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
    pil = lambda: R.depth_preprocess_pil(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.float32)  # noqa: E731
    flt = lambda form: R.depth_preprocess(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.float32, form=form)  # noqa: E731
    row = dict(shape="16 x 2160 x 3840 -> 518 x 924 f32")
    row.update(_time({"k_pil_resample": pil, "k_depth_prep_strip": lambda: flt(2), "k_depth_prep": lambda: flt(1)}, args.rounds))
    row["route"] = R.pil_route
    row["max_abs_pil_minus_float"] = float((pil() - flt(1)).abs().max())   # the 8-bit roundings, in normalised units (1 LSB = 1 / 255 / std)
    stated = pil_resample.pixel_values(frames[:2], th, tw, IMAGENET_MEAN, IMAGENET_STD).permute(0, 3, 1, 2)
    row["equals_statement_at_this_size"] = bool(torch.equal(pil()[:2], stated))
    del stated
    print(json.dumps(row), flush=True)
    del frames
    H, W = 1080, 1920
    frames = torch.randint(0, 256, (B, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)
    th2, tw2 = dpt_resize_target(512, 896)
    th1, tw1 = dpt_resize_target(H, W)
    row = dict(shape=f"16 x 1080 x 1920 -> 512 x 896 u8 -> {th2} x {tw2} f32 (two launches)")
    row.update(_time({"k_pil_resample x 2": lambda: R.depth_preprocess_pil(frames, th2, tw2, IMAGENET_MEAN, IMAGENET_STD, inference_size=(896, 512)),
                      "k_pil_resample, no inference size": lambda: R.depth_preprocess_pil(frames, th1, tw1, IMAGENET_MEAN, IMAGENET_STD),
                      "k_depth_prep_strip, no inference size": lambda: R.depth_preprocess(frames, th1, tw1, IMAGENET_MEAN, IMAGENET_STD, form=2)}, args.rounds))
    row["route"] = R.pil_route
    print(json.dumps(row), flush=True)
    R.close()


if __name__ == "__main__":
    main()
