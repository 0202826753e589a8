"""Measurements behind profiles/r32_zoedepth.md: DepthPipe("zoedepth-nyu-kitti") -- the full-size synthetic model -- on 1080p frames (384 x 672 after the padded
resize), one frame and four: the whole forward with the metric head on the two kernels and with the stock head (VD3D_ZOE_HEAD=0), the head alone on the pipe's own
features both ways, and the two ends of the image processor beside their ATen statements.  Runs alternate; medians of ROUNDS rounds, the spread as min .. max.  Prints
one JSON line per measurement.

    python tools/probe_zoedepth.py [--frames 1 4]
"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ROUNDS = 3


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def rounds(fns, iters, warm=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4])
    a = ap.parse_args()
    from visiondepth3d_amd import zoedepth
    from visiondepth3d_amd.depth import DepthPipe
    from visiondepth3d_amd.render_3d import Renderer
    R = Renderer(0)
    from transformers import ZoeDepthForDepthEstimation
    from visiondepth3d_amd.depth import build_config, synthetic_weights_
    name = "zoedepth-nyu-kitti"
    base = ZoeDepthForDepthEstimation(build_config(name)).eval()   # one synthetic model, copied per pipe
    synthetic_weights_(base, 0)
    os.environ.pop("VD3D_ZOE_HEAD", None)
    routed = DepthPipe(name, renderer=R, model=copy.deepcopy(base))
    os.environ["VD3D_ZOE_HEAD"] = "0"
    stock = DepthPipe(name, renderer=R, model=base)
    os.environ.pop("VD3D_ZOE_HEAD")
    print(json.dumps(dict(what="pipes", params=routed.n_params, routed=routed.zoe_routes, stock=stock.zoe_routes)))
    H, W = 1080, 1920
    pads = zoedepth.pad_amounts(H, W)
    target = zoedepth.resize_target(H + 2 * pads[0], W + 2 * pads[1], routed.proc["size"], routed.proc["multiple"], routed.proc["keep_aspect_ratio"])
    with torch.no_grad():
        for B in a.frames:
            fr = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda")
            kept = {}
            hooks = [p.model.metric_head.register_forward_pre_hook(lambda m, args, kw, k=k: kept.__setitem__(k, kw), with_kwargs=True)
                     for k, p in (("routed", routed), ("stock", stock))]
            d = (routed.infer_bgr_u8(fr) - stock.infer_bgr_u8(fr)).abs()
            for h in hooks:
                h.remove()
            print(json.dumps(dict(what="agreement", frames=B, target=target, max_abs_diff=float(d.max()), domain=routed.zoe_domain.tolist())))
            r = rounds({"forward_routed": lambda: routed.infer_bgr_u8(fr), "forward_stock_head": lambda: stock.infer_bgr_u8(fr)}, 3)
            print(json.dumps(dict(what="forward", frames=B, ms=r)))
            r = rounds({"head_routed": lambda: routed.model.metric_head(**kept["routed"]), "head_stock": lambda: stock.model.metric_head(**kept["stock"])}, 5)
            print(json.dumps(dict(what="metric_head", frames=B, ms=r)))
            pred = torch.rand(B, *target, device="cuda") * 9 + 0.5
            proc = routed.proc
            r = rounds({"preprocess_kernel": lambda: R.zoedepth_preprocess(fr, pads, target, proc["mean"], proc["std"], routed._zoe_table),
                        "preprocess_aten": lambda: zoedepth.preprocess_statement(fr, proc).contiguous(memory_format=torch.channels_last),
                        "post_kernel": lambda: R.zoedepth_post(pred, H, W, pads),
                        "post_aten": lambda: zoedepth.post_statement(pred, H, W)}, 10)
            print(json.dumps(dict(what="ends", frames=B, ms=r)))


if __name__ == "__main__":
    main()
