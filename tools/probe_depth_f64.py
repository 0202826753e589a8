"""How far apart are two stock float32 implementations of the depth network under the outlier weights (tests/outlier_weights.py)?  The stock Hugging Face
module in float32 on the GPU (hipBLASLt / MIOpen / SDPA) and on the CPU, both against the stock module in float64 on the CPU, seeds 0 .. 2, on the frames of
tests/test_hip_depth_f64.py.  The largest GPU / CPU ratio is what that test's K and K_RMS are derived from (profiles/r09_range_and_outliers.md).

    python tools/probe_depth_f64.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import outlier_weights as ow   # noqa: E402


@torch.no_grad()
def main():
    frames = ow.clip_frames()
    worst = dict(max_ratio=0.0, rms_ratio=0.0)
    for seed in (0, 1, 2):
        p64, p32 = ow.reference_predictions(seed)
        gpu = ow.stock_model(seed, torch.float32).cuda()(pixel_values=ow.pixel_values(frames, torch.float32).cuda()).predicted_depth
        (e_g, r_g), (e_c, r_c) = ow.errors_of_range(gpu, p64), ow.errors_of_range(p32, p64)
        row = dict(seed=seed, range=float(p64.max() - p64.min()), floor=float((p64 == 0).double().mean()), E_gpu=e_g, E_cpu=e_c, max_ratio=e_g / e_c,
                   rms_gpu=r_g, rms_cpu=r_c, rms_ratio=r_g / r_c)
        worst = dict(max_ratio=max(worst["max_ratio"], row["max_ratio"]), rms_ratio=max(worst["rms_ratio"], row["rms_ratio"]))
        print("STOCK_F32", json.dumps(row))
    k, k_rms = max(2.5, 1.5 * worst["max_ratio"]), max(1.5, 1.5 * worst["rms_ratio"])
    print("STOCK_F32_WORST", json.dumps(dict(worst, K=k, K_RMS=k_rms, device=torch.cuda.get_device_name(0), torch=torch.__version__)))


if __name__ == "__main__":
    main()
