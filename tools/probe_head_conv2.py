"""The float32 head's up-sampling + conv2 + tail: today's fused kernel (vd3d_dpt_head_conv_f32) beside the coarse GEMM + in-LDS gather form
(vd3d_head_conv_gather_f32), alternating in one process, device-event time, at the headline shape (DA-V2-Base at 4K, 16 frames: 296 x 528 x 64 -> 518 x 924) and
DA-V2-Small's channel count (32).  Reports median (min .. max) per call, TFLOP/s on the flops each form executes (the gather form: the MFMAs of every 32-pixel
group of every tile's coarse window + 36 multiply-adds per fine value), the saving as a multiple of the larger (max - min) spread, and both forms' error against
the float64 module chain on the first frame.

A library built with -DHG_ABLATE_GATHER or -DHG_ABLATE_MFMA (csrc/vd3d_head_gather.hip; results are then wrong) and given through VD3D_LIB_PATH shows the parts.

  python tools/probe_head_conv2.py [--rounds 15] [--calls 4] [--batch 16] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visiondepth3d_amd.depth import head_conv2_compose  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402

F = torch.nn.functional
CL = torch.channels_last


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def series(fns, rounds, calls):
    """The callables alternate round by round -> per callable (median, min, max)."""
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(ts, fns):
            t.append(timed(fn, calls))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(s):
    return f"{s[0]:.3f} ({s[1]:.3f} .. {s[2]:.3f})"


def window_groups(n, nc, t):
    """Per tile along one axis: the coarse pixels its windows reach (the kernel's float32 operations)."""
    s = np.float32(nc - 1) / np.float32(n - 1)
    out = []
    for p0 in range(0, n, t):
        pa, pb = max(p0 - 1, 0), min(p0 + t, n - 1)
        lo, hb = int(s * np.float32(pa)), int(s * np.float32(pb))
        out.append(hb + (1 if hb < nc - 1 else 0) - lo + 1)
    return out


def probe(R, say, label, B, ih, iw, oh, ow, Cin, rounds, calls):
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, Cin, ih, iw, device="cuda", generator=g).contiguous(memory_format=CL)
    b1 = torch.randn(Cin, device="cuda", generator=g)
    W = torch.randn(32, Cin, 3, 3, device="cuda", generator=g) / (3.0 * Cin ** 0.5)
    b2, w3 = torch.randn(32, device="cuda", generator=g), torch.randn(32, device="cuda", generator=g)
    img = R.dpt_head_conv_pack(W)
    packed = R.head_conv_gather_pack(*head_conv2_compose(W, b1))
    T = R.head_conv_gather_tile((ih, iw), (oh, ow), Cin)

    def conv():
        return R.dpt_head_conv(x, b1, (oh, ow), img, b2, w3, 0.1, 1.5)

    def gather():
        return R.dpt_head_conv(x, b1, (oh, ow), packed, b2, w3, 0.1, 1.5, form="gather")
    a, b = conv(), gather()
    up = F.interpolate(x[:1].double(), size=(oh, ow), mode="bilinear", align_corners=True) + b1.double().view(1, -1, 1, 1)
    pre = (torch.relu(F.conv2d(up, W.double(), None, padding=1) + b2.double().view(1, -1, 1, 1)) * w3.double().view(1, -1, 1, 1)).sum(1)
    ref = torch.relu(pre + 0.1) * 1.5
    ea, eb = (a[:1].double() - ref).abs(), (b[:1].double() - ref).abs()
    errs = f"{float(eb.max()):.2e} / {float(ea.max()):.2e}, {float(eb.pow(2).mean().sqrt()):.2e} / {float(ea.pow(2).mean().sqrt()):.2e}"
    del a, b, up, pre, ref, ea, eb
    for fn in (conv, gather):
        fn()
    torch.cuda.synchronize()
    sc, sg = series((conv, gather), rounds, calls)
    spread = max(sc[2] - sc[1], sg[2] - sg[1])
    flop_conv = 2.0 * B * oh * ow * 9 * Cin * 32
    groups = sum(-(-(ry * rx) // 32) for ry in window_groups(oh, ih, T[0]) for rx in window_groups(ow, iw, T[1]))
    flop_gather = B * (groups * 32 * 2.0 * Cin * 32 * 9 + oh * ow * 32 * 36 * 2.0)
    say(f"| {label} | {B} x {ih} x {iw} x {Cin} -> {oh} x {ow} | {T[0]} x {T[1]} | {fmt(sc)}: {flop_conv / (sc[0] * 1e-3) / 1e12:.1f} TFLOP/s | "
        f"{fmt(sg)}: {flop_gather / (sg[0] * 1e-3) / 1e12:.1f} TFLOP/s | {sc[0] - sg[0]:.3f} = {(sc[0] - sg[0]) / spread:.1f} x | {sc[0] / sg[0]:.2f} | "
        f"{flop_conv / 1e9:.1f} -> {flop_gather / 1e9:.1f} | {errs} |")
    del x
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    R = Renderer(0)
    say(f"{a.rounds} alternating rounds of {a.calls} calls; ms per call: median (min .. max); library {os.environ.get('VD3D_LIB_PATH', 'default')}")
    say("| shape | B x ih x iw x C_in -> fine map | fitted tile | today's kernel ms | GEMM + gather form ms | saved ms = multiple of the larger (max - min) | "
        "conv / gather | GFLOP module graph -> executed | max error vs float64 gather / conv, RMS gather / conv |")
    say("|---|---|---|---|---|---|---|---|---|")
    B = a.batch
    probe(R, say, "DA-V2-Base 4K", B, 296, 528, 518, 924, 64, a.rounds, a.calls)
    probe(R, say, "DA-V2-Small 4K", B, 296, 528, 518, 924, 32, a.rounds, a.calls)
    R.close()


if __name__ == "__main__":
    main()
