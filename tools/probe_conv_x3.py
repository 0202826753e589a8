"""bf16x3 3 x 3 convolution (vd3d_conv3x3_x3) on the DPT neck / fusion / head shapes of DA-V2-Small / -Base / -Large (37 x 66 and 74 x 132 token grids times
4, 2, 1, 0.5; the head at 8 x and at the input size): device-event time beside the float32 library convolution (MIOpen find mode on -- what gemm="bf16x3" uses
today) and vd3d_conv3x3_x2 where that builds; then the whole forward with conv=None and conv="bf16x3" alternating in one process.

  python tools/probe_conv_x3.py [--shapes [--cout N] [--x3-only]] [--forward] [--out FILE.md]     (both parts when neither is named)
--x3-only times vd3d_conv3x3_x3 alone (no MIOpen find per shape: seconds instead of minutes), for A/B runs of two builds of the library through VD3D_LIB_PATH."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visiondepth3d_amd.depth import MODEL_ZOO, DepthPipe  # noqa: E402
from visiondepth3d_amd.render_3d import Renderer  # noqa: E402

F = torch.nn.functional
PEAK_BF16 = 2.5e15   # dense bf16 MFMA FLOP/s of an MI355X


def bench(fn, n=10):
    fn(); fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def shape_list():
    """(model, where, B, H, W, Cin, Cout), duplicates across models removed"""
    out, seen = [], set()
    for name in ("depth-anything-v2-small", "depth-anything-v2-base", "depth-anything-v2-large"):
        z = MODEL_ZOO[name]
        Fh = z["fusion"]
        for (gh, gw), B in (((37, 66), 16), ((74, 132), 4)):
            sc = [(4 * gh, 4 * gw), (2 * gh, 2 * gw), (gh, gw), ((gh + 1) // 2, (gw + 1) // 2)]
            rows = [("neck", h, w, c, Fh) for (h, w), c in zip(sc, z["neck"])] + [("fusion", h, w, Fh, Fh) for h, w in sc]
            rows += [("head1", 8 * gh, 8 * gw, Fh, Fh // 2), ("head2", 14 * gh, 14 * gw, Fh // 2, z["head"])]
            for where, h, w, ci, co in rows:
                key = (B, h, w, ci, co)
                if key not in seen:
                    seen.add(key)
                    out.append((name.rsplit("-", 1)[1], where, B, h, w, ci, co))
    return out


def probe_shapes(R, say, only_cout=0, x3_only=False):
    torch.backends.cudnn.benchmark = True
    g = torch.Generator(device="cuda").manual_seed(1)
    say("| model, layer | B x H x W x C_in -> C_out | 8 x 32 tiles | conv3x3_x3 ms | library f32 ms | x3 / library | conv3x3_x2 ms | bf16 MFMA TFLOP/s (6 products), of peak |")
    say("|---|---|---|---|---|---|---|---|")
    for model, where, B, H, W, Cin, Cout in shape_list():
        if only_cout and Cout != only_cout:
            continue
        x = torch.relu(torch.randn(B, Cin, H, W, device="cuda", generator=g)).contiguous(memory_format=torch.channels_last)
        w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) * 0.05
        img = R.conv3x3_x3_pack(w)
        n = 5 if B * H * W * Cin * Cout > 4e11 else 10
        t3 = bench(lambda: R.conv3x3_x3(x, img, Cout), n)
        t32 = float("nan") if x3_only else bench(lambda: F.conv2d(x, w, None, 1, 1), n)
        img2 = None if x3_only else R.conv3x3_x2_pack(w)
        t2 = bench(lambda: R.conv3x3_x2(x, img2, Cout), n) if img2 is not None else None
        fl = 6 * 2.0 * B * H * W * Cin * 9 * Cout / (t3 * 1e-3)
        tiles = B * ((H + 7) // 8) * ((W + 31) // 32)
        say(f"| {model} {where} | {B} x {H} x {W} x {Cin} -> {Cout} | {tiles} | {t3:.3f} | {'--' if x3_only else f'{t32:.3f}'} | {'--' if x3_only else f'{t3 / t32:.2f}'} | {'--' if t2 is None else f'{t2:.3f}'} | "
            f"{fl / 1e12:.0f}, {100 * fl / PEAK_BF16:.1f} % |")
        del x, w, img, img2


def probe_forward(R, say, windows=3, steps=3):
    from visiondepth3d_amd import synth
    for name, B, H, W in (("depth-anything-v2-base", 16, 2160, 3840), ("depth-anything-v2-large", 4, 1080, 1920)):
        frames = torch.from_numpy(synth.synth_frame(0, H, W)[0]).cuda()[None].expand(B, -1, -1, -1).contiguous()
        pipes = {c: DepthPipe(name, device="cuda", dtype=torch.float32, renderer=R, gemm="bf16x3", conv=c, miopen_find=True) for c in (None, "bf16x3")}
        for p in pipes.values():   # warm-up of every shape (MIOpen find, the weight packs)
            p.infer_bgr_u8(frames, raw=True); p.infer_bgr_u8(frames, raw=True)
        ms = {c: [] for c in pipes}
        for _ in range(windows):   # the two modes alternate in one process
            for c, p in pipes.items():
                ms[c].append(bench(lambda: p.infer_bgr_u8(frames, raw=True), steps))
        routes = pipes["bf16x3"].conv_routes
        for c in pipes:
            v = ms[c]
            say(f"- {name}, {B} frames at {W} x {H}, gemm=bf16x3, conv={c}: median {statistics.median(v):.2f} ms per forward, windows {', '.join(f'{t:.2f}' for t in v)} "
                f"(spread {max(v) - min(v):.2f})")
        say(f"  routes: {sum(v[0] == 'bf16x3' for v in routes.values())} of {len(routes)} convolutions on vd3d_conv3x3_x3; on the library: "
            f"{sorted(k for k, v in routes.items() if v[0] == 'library')}")
        del pipes, frames
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--cout", type=int, default=0, help="only the shapes with this many output channels")
    ap.add_argument("--x3-only", action="store_true", help="with --shapes: time vd3d_conv3x3_x3 only")
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
    if a.shapes or not a.forward:
        probe_shapes(R, say, a.cout, a.x3_only)
    if a.forward or not a.shapes:
        probe_forward(R, say)
    R.close()


if __name__ == "__main__":
    main()
