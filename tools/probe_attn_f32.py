"""Exact-float32 attention (vd3d_attention_f32) against PyTorch's float32 SDPA (AOTriton), alternating in one process.

Shapes (B, T, H) of the depth leg's attention: (16, 2443, 12) DA-V2-Base at 4K, (16, 1370, 6) DA-V2-Small at 1080p, (16, 2443, 16) DA-V2-Large at 4K.
Per shape: AOTriton as the pipe runs it (Tq = T), AOTriton with the queries padded to a multiple of 256 (keys unpadded: what the bf16 pipe does), and the
library kernel -- as the pipe calls it (form 0) and with the workgroup form named (8 waves / 256 queries, 4 waves / 128 queries: vd3d_attention_f32_form), all
alternating; median (min .. max) ms over the rounds, TFLOP/s (4 B H T^2 64), the error of frame 0 against float64 (max abs, relative RMS), and per shape the
4-wave form's saving over the 8-wave form beside the larger of the two (max - min) spreads.
Usage: python tools/probe_attn_f32.py [--rounds N]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    args = ap.parse_args()
    R = Renderer(0)
    D = 64
    res = []
    for B, T, H in [(16, 2443, 12), (16, 1370, 6), (16, 2443, 16)]:
        g = torch.Generator(device="cuda").manual_seed(T + H)
        qkv = torch.randn(B, T, 3 * H * D, device="cuda", generator=g)
        scale = D ** -0.5
        v5 = qkv.view(B, T, 3, H, D)
        q, k, v = (v5[:, :, i].transpose(1, 2) for i in range(3))
        Tp = -(-T // 256) * 256
        qp = F.pad(v5[:, :, 0], (0, 0, 0, 0, 0, Tp - T)).transpose(1, 2)
        runs = {
            "sdpa": lambda: F.scaled_dot_product_attention(q, k, v, scale=scale),
            "sdpa_qpad": lambda: F.scaled_dot_product_attention(qp, k, v, scale=scale),
            "attention_f32": lambda: R.attention_f32(qkv, H, scale),
            "attention_f32_form8": lambda: R.attention_f32(qkv, H, scale, form=8),
            "attention_f32_form4": lambda: R.attention_f32(qkv, H, scale, form=4),
        }
        for f in runs.values():   # warm-up
            f(); f()
        torch.cuda.synchronize()
        ms = {n: [] for n in runs}
        for _ in range(args.rounds):
            for n, f in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record()
                torch.cuda.synchronize()
                ms[n].append(e0.elapsed_time(e1))
        flop = 4.0 * B * H * T * T * D
        q64, k64, v64 = (t[:1].double() for t in (q, k, v))
        ref = torch.softmax((q64 @ k64.transpose(-1, -2)) * scale, dim=-1) @ v64
        ref = ref.transpose(1, 2).reshape(1, T, H * D)
        outs = {"sdpa": runs["sdpa"]()[:1].transpose(1, 2).reshape(1, T, H * D), "attention_f32": runs["attention_f32"]()[:1]}
        row = dict(B=B, T=T, H=H)
        for n in runs:
            med = sorted(ms[n])[len(ms[n]) // 2]
            row[n] = dict(ms=round(med, 4), min_ms=round(min(ms[n]), 4), max_ms=round(max(ms[n]), 4), tflops=round(flop / med / 1e9, 1))
        for n, o in outs.items():
            d = o.double() - ref
            row[n]["max_err"] = float(d.abs().max())
            row[n]["rms_rel"] = float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
        best = min(row["sdpa"]["ms"], row["sdpa_qpad"]["ms"])
        row["speedup_vs_best_sdpa"] = round(best / row["attention_f32"]["ms"], 3)
        f8, f4 = row["attention_f32_form8"], row["attention_f32_form4"]
        row["form4_saves_ms"] = round(f8["ms"] - f4["ms"], 4)
        row["forms_larger_spread_ms"] = round(max(f8["max_ms"] - f8["min_ms"], f4["max_ms"] - f4["min_ms"]), 4)
        row["forms_same_bits"] = bool(torch.equal(runs["attention_f32_form8"](), runs["attention_f32_form4"]()))
        print(json.dumps(row), flush=True)
        res.append(row)
    R.close()


if __name__ == "__main__":
    main()
