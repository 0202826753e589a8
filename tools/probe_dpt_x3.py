#!/usr/bin/env python3
"""GPU probe: DPT-Large's depth leg at 4K in the three modes -- gemm="f32" (the stock float32 module graph), "bf16x3" and "fp16x2" (the split-operand
rewrite).  16 synthetic 3840 x 2160 frames per step (inference at 384 x 384), DepthPipe.infer_bgr_u8(raw=True).  Steady state: warm-up steps first, then
HIP events around every timed step; then a torch-profiler kernel trace of a few more steps, summed per kernel family.
usage: probe_dpt_x3.py [steps] [warmup] [modes...]   (the last output line is the whole result as one JSON object)"""
import json
import os
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

FAMILIES = (   # first match wins
    ("split GEMM (vd3d_gemm_x3)", ("k_gemm_bf16x3", "k_gemm_x3")),
    ("split attention (vd3d_attention_x3)", ("k_attn_",)),
    ("split 3x3 conv (vd3d_conv3x3_x2)", ("k_conv3x3_x2",)),
    ("scatter (vd3d_depth_to_space_bias)", ("k_depth_to_space_bias",)),
    ("vd3d glue (LN, bias/act, up-sampling, head tail, front end)", ("k_add_layernorm", "k_bias_act", "k_upsample", "k_head_tail", "k_depth_prep")),
    ("library conv (MIOpen)", ("igemm_", "ck::", "_ZN2ck", "conv", "SubTensorOp", "transpose_NCHW", "transpose_NHWC", "batched_transpose")),
    ("library GEMM (hipBLASLt / rocBLAS)", ("Cijk_", "gemm", "Gemm")),
    ("library attention (SDPA)", ("attn_fwd", "flash", "aotriton", "fmha")),
    ("ATen elementwise / copies / LN / interpolate", ("at::native", "elementwise", "layer_norm", "upsample")),
)


def family(name):
    for fam, keys in FAMILIES:
        if any(k in name for k in keys):
            return fam
    return "other"


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    modes = sys.argv[3:] or ["f32", "bf16x3", "fp16x2"]
    from torch.profiler import ProfilerActivity, profile
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import DepthPipe
    from visiondepth3d_amd.render_3d import Renderer
    H, W, B = 2160, 3840, 16
    base = np.stack([synth.synth_frame(i, H, W)[0] for i in range(4)])   # 4 distinct synthetic frames, each 4 times in the batch of 16
    frames = torch.from_numpy(np.concatenate([base] * (B // 4))).cuda()
    R = Renderer(0)
    res = {}
    for mode in modes:
        pipe = DepthPipe("dpt-large", device="cuda", dtype=torch.float32, renderer=R, gemm=mode, seed=5)
        for _ in range(warmup):
            pipe.infer_bgr_u8(frames, raw=True)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record()
            pipe.infer_bgr_u8(frames, raw=True)
            b.record()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        n_prof = 3
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n_prof):
                pipe.infer_bgr_u8(frames, raw=True)
            torch.cuda.synchronize()
        fam = defaultdict(lambda: [0.0, 0])
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            if t is None:
                t = e.cuda_time_total
            if t <= 0:
                continue
            f = fam[family(e.key)]
            f[0] += t / 1e3 / n_prof
            f[1] += e.count / n_prof
        med = statistics.median(ms)
        res[mode] = dict(step_ms_median=med, step_ms_min=min(ms), step_ms_max=max(ms), frames_per_s=B / med * 1e3,
                         kernel_ms_per_step={k: round(v[0], 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1][0])},
                         launches_per_step={k: round(v[1], 1) for k, v in fam.items()}, flops_per_frame=pipe.flops_per_frame(H, W))
        print(f"== dpt-large {mode}: {med:.2f} ms / {B} frames (min {min(ms):.2f}, max {max(ms):.2f}) = {B / med * 1e3:.1f} frames/s", flush=True)
        for k, v in res[mode]["kernel_ms_per_step"].items():
            print(f"   {v:9.3f} ms/step {res[mode]['launches_per_step'][k]:7.1f} launches  {k}", flush=True)
        del pipe
        torch.cuda.empty_cache()
    if "f32" in res:
        for mode in res:
            res[mode]["speedup_vs_f32"] = res["f32"]["step_ms_median"] / res[mode]["step_ms_median"]
            print(f"{mode}: {res[mode]['speedup_vs_f32']:.2f} x the f32 frame rate")
    R.close()
    print(json.dumps(dict(steps=steps, warmup=warmup, batch=B, frame=[H, W], inference=[384, 384], modes=res)), flush=True)


if __name__ == "__main__":
    main()
