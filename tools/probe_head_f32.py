"""The DPT head's fused exact-float32 kernel (vd3d_dpt_head_conv_f32) beside the launches it replaces, alternating in one process, device-event time,
MIOpen find mode on (what bench.py uses):

  conv2 + tail   up-sampling (vd3d_upsample_bilinear_bias_nhwc_f32) + library 3 x 3 convolution + vd3d_dpt_head_tail_f32   vs   one fused launch
                 at the headline shape (DA-V2-Base at 4K: 16 x 296 x 528 x 64 -> 518 x 924, 64 -> 32) and at the DA-V2-Small shape (32 -> 32)
  conv1 (stage 2) up-sampling x 2 of the last fusion layer's projection + library 3 x 3 convolution   vs   the fused launch with the plain epilogue
                 (16 x 148 x 264 x 128 -> 296 x 528, 128 -> 64)

  python tools/probe_head_f32.py [--rounds 15] [--calls 4] [--batch 16] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

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


def probe(R, say, label, B, ih, iw, oh, ow, Cin, Cout, tail, rounds, calls):
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, Cin, ih, iw, device="cuda", generator=g).contiguous(memory_format=CL)
    b_in = torch.randn(Cin, device="cuda", generator=g)
    W = (torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / (3.0 * Cin ** 0.5)).contiguous(memory_format=CL)
    b2, w3 = torch.randn(Cout, device="cuda", generator=g), torch.randn(Cout, device="cuda", generator=g)
    img = R.dpt_head_conv_pack(W)

    def parts():
        h = R.upsample_bilinear_bias(x, (oh, ow), b_in)
        y = F.conv2d(h, W, None, 1, 1)
        return R.dpt_head_tail(y.contiguous(memory_format=CL), b2, w3, 0.1, 2.0) if tail else y

    def fused():
        return R.dpt_head_conv(x, b_in, (oh, ow), img, b2, w3, 0.1, 2.0) if tail else R.dpt_head_conv(x, b_in, (oh, ow), img)

    def conv_only(h):
        return lambda: F.conv2d(h, W, None, 1, 1)
    a, b = parts(), fused()   # warm-up: MIOpen find, the LDS opt-in
    err = float((a - b).abs().max()) / max(1e-30, float(a.abs().max()))
    del a, b
    parts(); fused(); torch.cuda.synchronize()
    tp, tf = [], []
    for _ in range(rounds):   # the two routes alternate
        tp.append(timed(parts, calls))
        tf.append(timed(fused, calls))
    h = R.upsample_bilinear_bias(x, (oh, ow), b_in)
    tc = statistics.median(timed(conv_only(h), calls) for _ in range(5))
    del h
    flop = 2.0 * B * oh * ow * Cin * 9 * Cout
    mp, mf = statistics.median(tp), statistics.median(tf)
    moved_parts = 4.0 * B * (ih * iw * Cin + 2 * oh * ow * Cin + (2 * oh * ow * Cout + oh * ow if tail else oh * ow * Cout))
    moved_fused = 4.0 * B * (ih * iw * Cin + (oh * ow if tail else oh * ow * Cout))
    say(f"| {label} | {B} x {ih} x {iw} x {Cin} -> {oh} x {ow}, {Cin} -> {Cout} {'+ tail' if tail else 'plain'} | {mp:.3f} ({min(tp):.3f} .. {max(tp):.3f}) | {tc:.3f} | "
        f"{mf:.3f} ({min(tf):.3f} .. {max(tf):.3f}) | {mp / mf:.2f} | {flop / (mf * 1e-3) / 1e12:.1f}, {100 * flop / (mf * 1e-3) / SUSTAINED_F32_MFMA:.0f} % | "
        f"{flop / (tc * 1e-3) / 1e12:.1f} | {moved_parts / 1e9:.2f} -> {moved_fused / 1e9:.2f} | {err:.1e} |")
    del x, W, img
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
    say("| shape | B x ih x iw x C -> oh x ow, channels | separate launches ms | of which library conv ms | fused ms | separate / fused | fused TFLOP/s, of 134 sustained | "
        "library conv TFLOP/s | minimum HBM GB per call | max diff of max |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    B = a.batch
    probe(R, say, "DA-V2-Base 4K conv2", B, 296, 528, 518, 924, 64, 32, True, a.rounds, a.calls)
    probe(R, say, "DA-V2-Small conv2", B, 296, 528, 518, 924, 32, 32, True, a.rounds, a.calls)
    probe(R, say, "DA-V2-Base 4K conv1 (stage 2)", B, 148, 264, 296, 528, 128, 64, False, a.rounds, a.calls)
    R.close()


if __name__ == "__main__":
    main()
