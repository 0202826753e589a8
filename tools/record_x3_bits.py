"""The cases of tests/test_hip_x3_bits.py and the recorder of tests/golden/x3_bits.json: one SHA-256 of the raw output bytes per case of vd3d_conv3x3_x3,
vd3d_conv_ifn, vd3d_conv3x3_s2_x3, vd3d_conv3x3_s1_x2 and vd3d_conv3x3_s2_x2.  The hashes pin the BITS of the tile convolutions (every entry point on the kernel
body of csrc/vd3d_conv_x3.h) across refactors of their kernel and of their launch side: record them with a library built from the commit
whose results are to be kept (a worktree build loaded through VD3D_LIB_PATH, as tools/build_ab.sh makes one), never with the library under test.

Inputs: a closed-form integer hash of the element index (no library random generator), turned into float32 words with a random sign, all 23 stored mantissa bits
random (a full 24-bit significand: all three bf16 terms and all six products are live) and a power-of-two scale per channel (2^-4 .. 2^4).

  VD3D_LIB_PATH=<library of the parent commit> python tools/record_x3_bits.py [--out tests/golden/x3_bits.json]      (GPU box)"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "x3_bits.json")
K3S1, K3S2, T4S2 = 0, 1, 2
KNAME = {K3S1: "k3s1", K3S2: "k3s2", T4S2: "t4s2"}


def hashed_f32(shape, channel_axis, seed):
    """float32 array: word i = sign(h) | exponent 127 + (7 c mod 9) - 4 | 23 mantissa bits of h, h = the 32-bit mix of the element index i and the seed."""
    n = int(np.prod(shape))
    h = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed * 0x9E3779B9 & 0xFFFFFFFF)
    h ^= h >> np.uint32(16); h *= np.uint32(0x7FEB352D); h ^= h >> np.uint32(15); h *= np.uint32(0x846CA68B); h ^= h >> np.uint32(16)
    h = h.reshape(shape)
    cs = [1] * len(shape)
    cs[channel_axis] = shape[channel_axis]
    e = ((np.arange(shape[channel_axis], dtype=np.uint32) * np.uint32(7)) % np.uint32(9) + np.uint32(123)).reshape(cs)
    return ((h & np.uint32(0x80000000)) | (e << np.uint32(23)) | ((h >> np.uint32(4)) & np.uint32(0x7FFFFF))).view(np.float32)


def cases():
    """(name, spec) in a fixed order.  conv3x3_x3: ragged tiles both ways, 2 x 2 tiles, three chunks (the A double buffer wraps), two frames; then one pixel, one
    chunk.  conv_ifn: every kind at every C_out, plain and with slope + residual + padded pitches + an output slice; stride 2 on an odd and an even size and at
    C_in 16 (the one- and two-step chunks).  conv3x3_s1_x2: conv3x3_x3's shapes.  conv3x3_s2_x3 / conv3x3_s2_x2: one and two 128-channel slices on an odd size
    (output 13 x 47: ragged tiles both ways, 2 x 2 tiles, three chunks, two frames) and on 2 x 2 (even, one output pixel, one chunk).  New cases go at the end."""
    out = []
    for co in (32, 64, 128, 256):
        out.append((f"conv3x3_x3-2x13x47x48-{co}", dict(fn="c3", B=2, H=13, W=47, Cin=48, Cout=co)))
    for co in (32, 256):
        out.append((f"conv3x3_x3-1x1x1x16-{co}", dict(fn="c3", B=1, H=1, W=1, Cin=16, Cout=co)))
    shapes = [(K3S1, 2, 9, 33, 32), (K3S2, 1, 21, 69, 32), (K3S2, 1, 18, 66, 32), (K3S2, 1, 7, 35, 16), (T4S2, 1, 11, 37, 32)]
    for kind, B, H, W, ci in shapes:
        for co in (32, 64, 96):
            for full in (0, 1):
                out.append((f"conv_ifn-{KNAME[kind]}-{B}x{H}x{W}x{ci}-{co}-{'full' if full else 'plain'}",
                            dict(fn="ifn", kind=kind, B=B, H=H, W=W, Cin=ci, Cout=co, full=full)))
    for co in (32, 64, 128, 256):
        out.append((f"conv3x3_s1_x2-2x13x47x48-{co}", dict(fn="s1_x2", B=2, H=13, W=47, Cin=48, Cout=co)))
        out.append((f"conv3x3_s1_x2-1x1x1x16-{co}", dict(fn="s1_x2", B=1, H=1, W=1, Cin=16, Cout=co)))
    for fn in ("s2_x3", "s2_x2"):
        for co in (128, 256):
            out.append((f"conv3x3_{fn}-2x25x93x48-{co}", dict(fn=fn, B=2, H=25, W=93, Cin=48, Cout=co)))
            out.append((f"conv3x3_{fn}-1x2x2x16-{co}", dict(fn=fn, B=1, H=2, W=2, Cin=16, Cout=co)))
    return out


def run_case(R, spec):
    """Runs one case on Renderer R and returns the SHA-256 (hex) of the whole output buffer's bytes, the channels outside the written slice included."""
    import torch

    def dev(a):
        return torch.from_numpy(a).cuda()
    B, H, W, ci, co = spec["B"], spec["H"], spec["W"], spec["Cin"], spec["Cout"]
    if spec["fn"] != "ifn":
        fn = "x3" if spec["fn"] == "c3" else spec["fn"]
        x = dev(hashed_f32((B, H, W, ci), 3, 1)).permute(0, 3, 1, 2)
        img = getattr(R, f"conv3x3_{fn}_pack")(dev(hashed_f32((co, ci, 3, 3), 1, 2)))
        y = getattr(R, f"conv3x3_{fn}")(x, img, co).permute(0, 2, 3, 1)
    else:
        kind, full = spec["kind"], spec["full"]
        Ho, Wo = {K3S1: (H, W), K3S2: ((H + 1) // 2, (W + 1) // 2), T4S2: (2 * H, 2 * W)}[kind]
        xs, ys, yo = (ci + 16, co + 48, 16) if full else (ci, co, 0)
        x = dev(hashed_f32((B, H, W, xs), 3, 3)).permute(0, 3, 1, 2)          # the channels behind C_in hold hashed values too: read = seen
        w = hashed_f32((ci, co, 4, 4), 0, 4) if kind == T4S2 else hashed_f32((co, ci, 3, 3), 1, 4)
        img = R.conv_ifn_pack(kind, dev(w))
        bias = dev(hashed_f32((co,), 0, 5))
        slope = dev(hashed_f32((co,), 0, 6) * np.float32(0.125)) if full else None
        res = dev(hashed_f32((B, Ho, Wo, co), 3, 7)).permute(0, 3, 1, 2) if full else None
        out = dev(hashed_f32((B, Ho, Wo, ys), 3, 8)).permute(0, 3, 1, 2)      # what is not written keeps its hashed value and is hashed below
        y = R.conv_ifn(kind, x, ci, img, bias, slope, co, out, yo, res).permute(0, 2, 3, 1)
    assert img is not None
    torch.cuda.synchronize()
    return hashlib.sha256(y.contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    from visiondepth3d_amd import _lib
    from visiondepth3d_amd.render_3d import Renderer
    R = Renderer(0)
    got = {name: run_case(R, spec) for name, spec in cases()}
    R.close()
    with open(a.out, "w") as f:
        json.dump(dict(library=os.path.basename(_lib.LIB_PATH), cases=got), f, indent=1)
        f.write("\n")
    print(f"{len(got)} cases recorded with {_lib.LIB_PATH} -> {a.out}")


if __name__ == "__main__":
    main()
