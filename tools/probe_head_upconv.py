"""The float32 head's first convolution as coarse GEMM + fine gather (depth.py head_upconv_compose + vd3d_head_upconv_gather_f32) beside today's chain -- the last
fusion layer's 1 x 1 projection (library, no bias), vd3d_upsample_bilinear_bias_nhwc_f32, head.conv1 3 x 3 (library, no bias) -- alternating in one process,
device-event time, MIOpen find mode on (what bench.py uses), at the headline shape (DA-V2-Base at 4K, 16 frames: 148 x 264 x 128 -> 296 x 528 x 64) and
DA-V2-Small's (64 -> 32).  The GEMM and the gather are also timed separately (alternating with each other), as are the chain's three launches.
Also: the GEMM's TFLOP/s, the gather's bytes (Z once + the output) against its time, and both routes' error against the float64 module chain.

  python tools/probe_head_upconv.py [--rounds 15] [--calls 4] [--batch 16] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visiondepth3d_amd.depth import head_upconv_compose  # noqa: E402
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


def probe(R, say, label, B, h, w, C, Co, rounds, calls):
    H, W = 2 * h, 2 * w
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, C, h, w, device="cuda", generator=g).contiguous(memory_format=CL)
    pw = (torch.randn(C, C, 1, 1, device="cuda", generator=g) / C ** 0.5).contiguous(memory_format=CL)
    pb = torch.randn(C, device="cuda", generator=g)
    cw = (torch.randn(Co, C, 3, 3, device="cuda", generator=g) / (3.0 * C ** 0.5)).contiguous(memory_format=CL)
    Wc, bc = head_upconv_compose(pw, pb, cw)
    rows = x.permute(0, 2, 3, 1).reshape(B * h * w, C)

    def proj():
        return F.conv2d(x, pw, None)

    def chain():
        return F.conv2d(R.upsample_bilinear_bias(proj(), (H, W), pb), cw, None, 1, 1)

    def gemm():
        return F.linear(rows, Wc, bc)

    def pair():
        return R.head_upconv_gather(gemm().view(B, h, w, -1), (H, W), Co)
    a, b = chain(), pair()   # warm-up: MIOpen find
    ref = F.conv2d(F.interpolate(F.conv2d(x[:2].double(), pw.double(), pb.double()), size=(H, W), mode="bilinear", align_corners=True), cw.double(), None, 1, 1)
    ea, eb = (a[:2].double() - ref).abs(), (b[:2].double() - ref).abs()
    errs = f"{float(eb.max()):.2e} / {float(ea.max()):.2e}, {float(eb.pow(2).mean().sqrt()):.2e} / {float(ea.pow(2).mean().sqrt()):.2e}"
    del a, b, ref, ea, eb
    p, z = proj(), gemm()
    u = R.upsample_bilinear_bias(p, (H, W), pb)

    def up():
        return R.upsample_bilinear_bias(p, (H, W), pb)

    def conv1():
        return F.conv2d(u, cw, None, 1, 1)

    def gather():
        return R.head_upconv_gather(z.view(B, h, w, -1), (H, W), Co)
    for fn in (chain, pair, proj, up, conv1, gemm, gather):
        fn()
    torch.cuda.synchronize()
    sc, sp = series((chain, pair), rounds, calls)
    s_proj, s_up, s_conv1, s_gemm, s_gather = series((proj, up, conv1, gemm, gather), rounds, calls)
    spread = max(sc[2] - sc[1], sp[2] - sp[1])
    flop_chain = 2.0 * B * h * w * C * C + 2.0 * B * H * W * 9 * C * Co
    flop_gemm = 2.0 * B * h * w * C * 9 * Co
    gather_bytes = 4.0 * B * (h * w * 9 * Co + H * W * Co)   # Z read once + the output
    say(f"| {label} | {B} x {h} x {w} x {C} -> {H} x {W} x {Co} | {fmt(sc)} | {fmt(sp)} | {sc[0] - sp[0]:.3f} = {(sc[0] - sp[0]) / spread:.1f} x | {sc[0] / sp[0]:.2f} | "
          f"{flop_chain / 1e9:.1f} -> {flop_gemm / 1e9:.1f} | {fmt(s_proj)}, {fmt(s_up)}, {fmt(s_conv1)} | {fmt(s_gemm)}: {flop_gemm / (s_gemm[0] * 1e-3) / 1e12:.1f} TFLOP/s | "
          f"{fmt(s_gather)}: {gather_bytes / 1e9:.2f} GB at {gather_bytes / (s_gather[0] * 1e-3) / 1e12:.2f} TB/s | {errs} |")
    del x, p, z, u, rows
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
    torch.backends.cudnn.benchmark = True
    R = Renderer(0)
    say(f"{a.rounds} alternating rounds of {a.calls} calls; ms per call: median (min .. max)")
    say("| shape | B x h x w x C -> fine map x C_out | today's chain ms | GEMM + gather ms | saved ms = multiple of the larger (max - min) | chain / pair | GFLOP chain -> executed | "
        "alone: projection, up-sampling, conv1 ms | GEMM alone ms | gather alone ms: Z once + output | max error vs float64 pair / chain, RMS pair / chain |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    B = a.batch
    probe(R, say, "DA-V2-Base 4K", B, 148, 264, 128, 64, a.rounds, a.calls)
    probe(R, say, "DA-V2-Small 4K", B, 148, 264, 64, 32, a.rounds, a.calls)
    R.close()


if __name__ == "__main__":
    main()
