"""The cases of tests/test_hip_attention_f32_bits.py and the recorder of tests/golden/attn_f32_bits.json: per case of vd3d_attention_f32_form (csrc/vd3d_attn.hip
k_attn_f32<NW, NS>, forms 8 and 4) the SHA-256 of the raw output bytes and the first and last four output words.  The digests pin the BITS of the exact-float32
attention across reworks of its tile loop: record them with a library built from the commit whose results are to be kept (a worktree build loaded through
VD3D_LIB_PATH, as tools/build_ab.sh makes one), never with the library under test.

Inputs: a closed-form integer hash of the element index and a seed (no library random generator, the same words on every machine): q, k, v uniform on a
2^-22 grid in [-2, 2), each query row times a power of two 2^-1 .. 2^2 by token (flat and nearly one-hot softmax rows side by side: the running maximum grows
in late tiles for some queries and not for others), v times 2^1.

  VD3D_LIB_PATH=<library of the parent commit> python tools/record_attn_f32_bits.py [--out tests/golden/attn_f32_bits.json]      (GPU box)"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_f32_bits.json")
D = 64
SCALE = 0.125


def hashed_qkv(B, T, H, seed):
    """float32 [B][T][3 H 64]: element i is ((24 bits of the 32-bit mix of i and the seed) - 2^23) 2^-22, exact in float32; q rows times 2^((5 t mod 4) - 1),
    v times 2 (exact)."""
    n = B * T * 3 * H * D
    h = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed * 0x9E3779B9 & 0xFFFFFFFF)
    h ^= h >> np.uint32(16); h *= np.uint32(0x7FEB352D); h ^= h >> np.uint32(15); h *= np.uint32(0x846CA68B); h ^= h >> np.uint32(16)
    x = ((h >> np.uint32(8)).astype(np.int32) - np.int32(1 << 23)).astype(np.float32) * np.float32(2.0 ** -22)
    x = x.reshape(B, T, 3, H, D)
    t = np.arange(T, dtype=np.int64)
    x[:, :, 0] *= np.exp2(((5 * t) % 4 - 1).astype(np.float32)).reshape(1, T, 1, 1)
    x[:, :, 2] *= np.float32(2.0)
    return x.reshape(B, T, 3 * H * D)


def cases():
    """(name, spec) in a fixed order, every shape with form 8 and form 4.  T: a single tile (1 .. 64), a last tile with at most 32 live keys (65, 95, 96, 129,
    160, 257, 321: its second 32-key half is past T), with more (97, 127, 161), exactly full (64, 128); (B, H) = (3, 3) has more than 8 (b, h) pairs: a
    second XCD group with empty slots.  Then the two depth-leg lengths, and T = 64 k + 5 (k = 2 .. 7): 3 .. 8 tiles, so that the loop ends behind every copy
    of a body unrolled over the ring's two or three stages.  New cases go at the end."""
    shapes = []
    for T in (1, 11, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 161, 257, 321):
        for B, H in ((1, 1), (2, 3), (3, 3)):
            shapes.append((B, T, H))
    shapes += [(1, 2443, 2), (1, 1370, 2)]
    shapes += [(1, 64 * k + 5, 2) for k in range(2, 8)]
    return [(f"B{B}-T{T}-H{H}-form{form}", dict(B=B, T=T, H=H, form=form)) for B, T, H in shapes for form in (8, 4)]


def run_case(R, spec):
    """Runs one case on Renderer R: dict(sha256 = of the output's bytes, first / last = its first / last four float32 words as integers)."""
    import torch
    B, T, H = spec["B"], spec["T"], spec["H"]
    qkv = torch.from_numpy(hashed_qkv(B, T, H, 1 + T + 4096 * H + 65536 * B)).cuda()
    out = R.attention_f32(qkv, H, SCALE, form=spec["form"])
    torch.cuda.synchronize()
    assert out.shape == (B, T, H * D)
    o = out.contiguous().cpu().numpy()
    w = o.reshape(-1).view(np.uint32)
    return dict(sha256=hashlib.sha256(o.tobytes()).hexdigest(), first=[int(v) for v in w[:4]], last=[int(v) for v in w[-4:]])


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
        json.dump(dict(library=os.path.basename(_lib.LIB_PATH), cases=got), f, indent=0)
        f.write("\n")
    print(f"{len(got)} cases recorded with {_lib.LIB_PATH} -> {a.out}")


if __name__ == "__main__":
    main()
