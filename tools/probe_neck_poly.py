"""The float32 neck's polyphase launch (vd3d_neck_poly_conv_f32) beside the library chain it replaces -- ConvTranspose2d (kernel == stride == f, bias) + the bias-free
3 x 3 convolution -- alternating in one process, device-event time, MIOpen find mode on (what bench.py uses), at the headline shapes (DA-V2-Base at 4K, 16 frames:
37 x 66 coarse pixels; stage 0: 96 -> 96 (f = 4) -> 128 on 148 x 264, stage 1: 192 -> 192 (f = 2) -> 128 on 74 x 132) and DA-V2-Small's (48 / 96 -> 64).
Also: TFLOP/s on the EXECUTED flops (the composed form's 2 x blocks x C_in x C_out per coarse pixel) and both routes' error against the float64 module chain.

  python tools/probe_neck_poly.py [--rounds 15] [--calls 4] [--batch 16] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visiondepth3d_amd.depth import neck_poly_compose, neck_poly_offsets  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402

F = torch.nn.functional
CL = torch.channels_last
SUSTAINED_F32_MFMA = 134e12   # measured sustained v_mfma_f32_32x32x2_f32 rate of an MI355X


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def probe(R, say, label, B, h, w, Cin, Cout, f, rounds, calls):
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, Cin, h, w, device="cuda", generator=g).contiguous(memory_format=CL)
    wt = torch.randn(Cin, Cin, f, f, device="cuda", generator=g) / Cin ** 0.5
    bt = torch.randn(Cin, device="cuda", generator=g)
    w3 = (torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / (3.0 * Cin ** 0.5)).contiguous(memory_format=CL)
    packed = R.neck_poly_pack(*neck_poly_compose(wt, bt, w3, f), f)

    def chain():
        return F.conv2d(F.conv_transpose2d(x, wt, bt, stride=f), w3, None, 1, 1)

    def poly():
        return R.neck_poly_conv(x, packed)
    a, b = chain(), poly()   # warm-up: MIOpen find
    ref = F.conv2d(F.conv_transpose2d(x[:2].double(), wt.double(), bt.double(), stride=f), w3.double(), None, 1, 1)
    ea, eb = (a[:2].double() - ref).abs(), (b[:2].double() - ref).abs()
    errs = f"{float(eb.max()):.2e} / {float(ea.max()):.2e}, {float(eb.pow(2).mean().sqrt()):.2e} / {float(ea.pow(2).mean().sqrt()):.2e}"
    del a, b, ref, ea, eb
    chain(); poly(); torch.cuda.synchronize()
    tc, tp = [], []
    for _ in range(rounds):   # the two routes alternate
        tc.append(timed(chain, calls))
        tp.append(timed(poly, calls))
    mc, mp = statistics.median(tc), statistics.median(tp)
    spread = max(max(tc) - min(tc), max(tp) - min(tp))
    flop_chain = 2.0 * B * (f * h) * (f * w) * Cin * (Cin + 9 * Cout)
    flop_poly = 2.0 * B * h * w * len(neck_poly_offsets(f)) * Cin * Cout
    say(f"| {label} | {B} x {h} x {w} x {Cin} -> {f * h} x {f * w} x {Cout} | {mc:.3f} ({min(tc):.3f} .. {max(tc):.3f}) | {mp:.3f} ({min(tp):.3f} .. {max(tp):.3f}) | "
        f"{mc - mp:.3f} = {(mc - mp) / spread:.1f} x | {mc / mp:.2f} | {flop_chain / 1e9:.1f} -> {flop_poly / 1e9:.1f} | "
        f"{flop_poly / (mp * 1e-3) / 1e12:.1f}, {100 * flop_poly / (mp * 1e-3) / SUSTAINED_F32_MFMA:.0f} % | {flop_chain / (mc * 1e-3) / 1e12:.1f} | {errs} |")
    del x, wt, w3, packed
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
    say("| stage | B x h x w x C_in -> fine map x C_out | library chain ms | composed launch ms | saved ms = multiple of the larger (max - min) | chain / composed | "
        "GFLOP chain -> executed | composed TFLOP/s on executed flops, of 134 sustained | chain TFLOP/s on its own flops | max error vs float64 composed / chain, RMS composed / chain |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    B = a.batch
    probe(R, say, "DA-V2-Base 4K stage 0", B, 37, 66, 96, 128, 4, a.rounds, a.calls)
    probe(R, say, "DA-V2-Base 4K stage 1", B, 37, 66, 192, 128, 2, a.rounds, a.calls)
    probe(R, say, "DA-V2-Small 4K stage 0", B, 37, 66, 48, 64, 4, a.rounds, a.calls)
    probe(R, say, "DA-V2-Small 4K stage 1", B, 37, 66, 96, 64, 2, a.rounds, a.calls)
    R.close()


if __name__ == "__main__":
    main()
