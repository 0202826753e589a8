"""Host side of the float32 head's second convolution in "coarse GEMM + fine gather" form (depth.py head_conv2_compose, csrc/vd3d_head_gather.hip): the composed
form is the module chain in float64, tap order and the packed image's layout, the C boundary's refusals, the kernel's arithmetic contract restated in NumPy with an
exact fused multiply-add (the reference tests/test_hip_head_gather.py compares the kernel's bits with), and the reference-only conditions of that file's float64
cases.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from test_head_upconv_host import fma32, gather_restated
from visiondepth3d_amd import _abi, _lib
from visiondepth3d_amd.depth import HEAD_CONV2_GATHER_BUILT, HEAD_CONV2_GATHER_ROUTED, head_conv2_compose

# coarse -> fine maps of the exact family; the two tile-sized ones are added on the GPU side from the tile the library reports
MAPS = (((5, 7), (9, 13)), ((3, 3), (2, 2)), ((19, 33), (33, 57)), ((37, 41), (65, 71)), ((9, 5), (9, 5)))
MAP_IDS = ["%dx%d-%dx%d" % (a + b) for a, b in MAPS]
#          B, coarse, fine, C_in
F64_CASES = ((2, (5, 7), (9, 13), 64), (2, (19, 33), (33, 57), 64), (1, (21, 29), (37, 50), 32), (2, (37, 41), (65, 71), 64), (1, (17, 33), (33, 65), 128))
F64_IDS = ["%dx%dx%d-%dx%d-c%d" % (c[0], *c[1], *c[2], c[3]) for c in F64_CASES]


def chain64(y1, b1, W, size):
    """The module chain in float64: conv1's bias, F.interpolate(bilinear, align_corners=True), conv2 with zero padding and without its bias."""
    up = F.interpolate(y1.double() + b1.double().view(1, -1, 1, 1), size=tuple(size), mode="bilinear", align_corners=True)
    return F.conv2d(up, W.double(), None, padding=1)


def tail64(y, b2, w3, b3, scale):
    pre = (torch.relu(y + b2.double().view(1, -1, 1, 1)) * w3.double().view(1, -1, 1, 1)).sum(1)
    return pre, torch.relu(pre + b3) * scale


def f64_inputs(case):
    """tests/test_hip_dpt_head_f32.py _inputs' draws from a CPU generator, seed 1000 ih + 10 iw + C_in."""
    B, (ih, iw), _, Cin = case
    g = torch.Generator().manual_seed(1000 * ih + 10 * iw + Cin)
    x = torch.randn(B, Cin, ih, iw, generator=g)
    b_in = torch.randn(Cin, generator=g)
    W = torch.randn(32, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    b2, w3 = torch.randn(32, generator=g), torch.randn(32, generator=g)
    return x, b_in, W, b2, w3


def exact_inputs(B, hw, Cin, seed):
    """The exact family: y1 integers in [-8, 8], b1 integers in [-4, 4], W from {0, 0, 0, +-1, +-2, +-0.5}: every Z value is exact in float32 in any order."""
    g = torch.Generator().manual_seed(seed)
    y1 = torch.randint(-8, 9, (B, hw[0], hw[1], Cin), generator=g).float()                       # NHWC
    b1 = torch.randint(-4, 5, (Cin,), generator=g).float()
    vals = torch.tensor([0.0, 0.0, 0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5])
    W = vals[torch.randint(0, 9, (32, Cin, 3, 3), generator=g)]
    b2 = torch.randint(-30, 31, (32,), generator=g).float()
    w3 = torch.randn(32, generator=g)
    return y1, b1, W, b2, w3


def pack_restated(Wt):
    """The weight image: [tap 9][q C_in / 8][lane 64][4 floats]; lane = 32 kh + o holds channels 8 q + 4 kh + 0 .. 3 of row tap 32 + o of Wt [9 x 32, C_in]."""
    Wt = np.asarray(Wt, np.float32)
    Cin = Wt.shape[1]
    img = np.empty((9, Cin // 8, 64, 4), np.float32)
    for kh in range(2):
        # [tap][o][q][j] -> [tap][q][o][j]
        img[:, :, 32 * kh:32 * kh + 32, :] = Wt.reshape(9, 32, Cin // 8, 2, 4)[:, :, :, kh, :].transpose(0, 2, 1, 3)
    return img


def z_restated(y1, Wt, bc):
    """Z[b, y, x, t, o]: one fmaf chain from 0 over the channels in the order q = 0 .. C_in / 8 - 1, j = 0 .. 3: channel 8 q + j, then 8 q + 4 + j; then + bc, one
    rounding.  y1 [B, h, w, C_in] float32, Wt [9 x 32, C_in], bc [9 x 32]."""
    y1, Wt, bc = (np.asarray(v, np.float32) for v in (y1, Wt, bc))
    B, h, w, Cin = y1.shape
    acc = np.zeros((B, h, w, 288), np.float32)
    for q in range(Cin // 8):
        for j in range(4):
            for c in (8 * q + j, 8 * q + 4 + j):
                acc = fma32(y1[..., c:c + 1], Wt[None, None, None, :, c], acc)
    return (acc + bc[None, None, None, :]).astype(np.float32).reshape(B, h, w, 9, 32)


def tail_restated(a, b2, w3, b3, scale):
    """s = 0; s = fmaf(max(a[o] + b2[o], 0), w3[o], s) for o ascending; out = max(s + b3, 0) * scale.  a [B, H, W, 32]."""
    a, b2, w3 = (np.asarray(v, np.float32) for v in (a, b2, w3))
    s = np.zeros(a.shape[:3], np.float32)
    for o in range(32):
        s = fma32(np.maximum(a[..., o] + b2[o], np.float32(0)), w3[o], s).reshape(s.shape)
    return (np.maximum(s + np.float32(b3), np.float32(0)) * np.float32(scale)).astype(np.float32)


def head_restated(y1, Wt, bc, b2, w3, b3, scale, size):
    """vd3d_head_conv_gather_f32's statement, operation for operation."""
    return tail_restated(gather_restated(z_restated(y1, Wt, bc), size[0], size[1]), b2, w3, b3, scale)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.mark.parametrize("Cin", HEAD_CONV2_GATHER_BUILT)
@pytest.mark.parametrize("hw,HW", MAPS, ids=MAP_IDS)
def test_composed_form_is_the_module_chain_in_float64(hw, HW, Cin):
    g = torch.Generator().manual_seed(1000 * hw[0] + 100 * hw[1] + HW[0] + Cin)
    y1 = torch.randn(2, Cin, *hw, generator=g, dtype=torch.float64)
    b1 = torch.randn(Cin, generator=g, dtype=torch.float64)
    W = torch.randn(32, Cin, 3, 3, generator=g, dtype=torch.float64) / (3.0 * Cin ** 0.5)
    ref = chain64(y1, b1, W, HW)
    Wt, bc = head_conv2_compose(W, b1, dtype=torch.float64)
    assert Wt.shape == (288, Cin) and bc.shape == (288,)
    z = (y1.permute(0, 2, 3, 1).reshape(-1, Cin) @ Wt.t() + bc).reshape(2, hw[0], hw[1], 9, 32)
    got = torch.from_numpy(gather_restated(z.numpy(), HW[0], HW[1], np.float64)).permute(0, 3, 1, 2)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.max() - ref.min())
    # the float32 result is the float64 one rounded once; the weight is a permutation (exact)
    W32, b32 = head_conv2_compose(W.float(), b1.float())
    W64, b64 = head_conv2_compose(W.float(), b1.float(), dtype=torch.float64)
    assert W32.dtype == torch.float32 and torch.equal(W32, W64.float()) and torch.equal(b32, b64.float())
    assert torch.equal(W32.reshape(9, 32, Cin), W.float().permute(2, 3, 0, 1).reshape(9, 32, Cin))


def test_tap_order_and_packed_layout():
    g = torch.Generator().manual_seed(3)
    Cin = 16
    W, b1 = torch.randint(-3, 4, (32, Cin, 3, 3), generator=g).double(), torch.randint(-3, 4, (Cin,), generator=g).double()
    Wt, bc = head_conv2_compose(W, b1, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            for o in (0, 5, 31):
                row = (3 * ky + kx) * 32 + o
                assert torch.equal(Wt[row], W[o, :, ky, kx]) and float(bc[row]) == float(W[o, :, ky, kx] @ b1)
    img = pack_restated(Wt.numpy())
    assert img.shape == (9, Cin // 8, 64, 4)
    for tap, q, lane, j in ((0, 0, 0, 0), (4, 1, 37, 2), (8, 1, 63, 3), (2, 0, 32, 0), (7, 1, 31, 1)):
        assert img[tap, q, lane, j] == float(Wt[tap * 32 + (lane & 31), 8 * q + 4 * (lane >> 5) + j])
    for bad in ((torch.zeros(32, 8, 1, 1), torch.zeros(8)), (torch.zeros(32, 8, 3, 3), torch.zeros(9)), (torch.zeros(32, 8, 3), torch.zeros(8))):
        with pytest.raises(ValueError):
            head_conv2_compose(*bad)
    assert set(HEAD_CONV2_GATHER_ROUTED) <= set(HEAD_CONV2_GATHER_BUILT) == {32, 64, 128}


def test_c_boundary(L):
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    declared = set(re.findall(r"\b(vd3d_[a-z0-9_]+)\s*\(", hdr))
    new = {"vd3d_head_conv_gather_weight_bytes", "vd3d_head_conv_gather_tile", "vd3d_head_conv_gather_pack_weights", "vd3d_head_conv_gather_f32"}
    assert new <= declared and new <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS) and all(hasattr(L, n) for n in new)
    for n in new:
        assert re.search(r"Additions since 6 that leave the version as it is.*?" + n + r".*?\*/\s*#define VD3D_ABI_VERSION 6", hdr, re.S), n
    assert _abi.ABI_VERSION == 6 and L.vd3d_abi_version() == 6
    for Cin in (32, 64, 128):
        assert L.vd3d_head_conv_gather_weight_bytes(Cin) == 9 * 32 * Cin * 4
    for Cin in (0, 16, 48, 96, 256):
        assert L.vd3d_head_conv_gather_weight_bytes(Cin) < 0
        assert L.vd3d_head_conv_gather_pack_weights(None, None, Cin, None) == _abi.E_UNSUPPORTED and b"not built" in L.vd3d_last_error()
    f = L.vd3d_head_conv_gather_f32
    # the shape is judged first: a refusal needs neither a context nor a device
    for Cin in (16, 48, 256, 0):
        assert f(None, None, 1, 5, 7, 9, 13, Cin, None, None, None, None, 0.0, 1.0, None) == _abi.E_UNSUPPORTED and b"not built" in L.vd3d_last_error()
    for B, ih, iw, oh, ow in ((0, 5, 7, 9, 13), (1, 0, 7, 9, 13), (1, 5, 0, 9, 13), (1, 5, 7, 1, 13), (1, 5, 7, 9, 1),
                              (1, 400, 7, 2, 13),                 # a down-sampling factor of 399: no tile's reach fits the window
                              (1, 5, 400, 9, 13),
                              (1, 5, 1 << 26, 9, 13)):            # a coarse row of 2^26 x 64 elements
        assert f(None, None, B, ih, iw, oh, ow, 64, None, None, None, None, 0.0, 1.0, None) == _abi.E_UNSUPPORTED, (B, ih, iw, oh, ow)
    th, tw = C.c_int(0), C.c_int(0)
    assert L.vd3d_head_conv_gather_tile(400, 7, 2, 13, 64, C.byref(th), C.byref(tw)) == _abi.E_UNSUPPORTED
    # built shapes (any size, moderate down-sampling included) get as far as the missing arguments
    for ih, iw, oh, ow in ((5, 7, 9, 13), (9, 5, 9, 5), (3, 3, 2, 2), (296, 528, 518, 924), (40, 40, 10, 10)):
        for Cin in (32, 64, 128):
            assert f(None, None, 1, ih, iw, oh, ow, Cin, None, None, None, None, 0.0, 1.0, None) == _abi.E_INVALID, (ih, iw, oh, ow)
            assert L.vd3d_head_conv_gather_tile(ih, iw, oh, ow, Cin, C.byref(th), C.byref(tw)) == 0 and 1 <= th.value <= (16 if Cin == 128 else 32) and 1 <= tw.value <= 32


def test_fitted_tile_wastes_little_on_the_workloads_map(L):
    """296 x 528 -> 518 x 924: the largest tile whose coarse reach fits 21 x 21 is cut down to the smallest edge with the same number of tiles."""
    th, tw = C.c_int(0), C.c_int(0)
    assert L.vd3d_head_conv_gather_tile(296, 528, 518, 924, 64, C.byref(th), C.byref(tw)) == 0
    for n, t in ((518, th.value), (924, tw.value)):
        nt = -(-n // t)
        assert 28 <= t <= 32 and nt * t - n < nt, (n, t)      # fewer idle rows than tiles: no edge one shorter has as few tiles


def test_restatement_on_hand_computed_maps():
    """1 x 1 -> 2 x 2, one input channel set: every sample is the single coarse pixel with weight 1, so a value is the plain sum of the taps inside the map."""
    Cin = 32
    y1 = np.zeros((1, 1, 1, Cin), np.float32)
    y1[0, 0, 0, 9] = 2.0                                           # channel 9 = 8 q + j with q = 1, j = 1
    W = torch.zeros(32, Cin, 3, 3)
    W[4, 9] = torch.arange(1.0, 10.0).reshape(3, 3)                # output channel 4: tap t has weight t + 1
    b1 = torch.zeros(Cin)
    b1[9] = 1.0
    Wt, bc = head_conv2_compose(W, b1)
    z = z_restated(y1, Wt.numpy(), bc.numpy())
    assert z.shape == (1, 1, 1, 9, 32) and np.array_equal(z[0, 0, 0, :, 4], 3.0 * np.arange(1, 10, dtype=np.float32)) and not z[..., :4].any() and not z[..., 5:].any()
    b2, w3 = np.zeros(32, np.float32), np.zeros(32, np.float32)
    w3[4] = 1.0
    out = head_restated(y1, Wt.numpy(), bc.numpy(), b2, w3, 0.0, 1.0, (2, 2))
    # pixel (0, 0): taps with ky, kx in {1, 2}: t = 4, 5, 7, 8 -> 3 (5 + 6 + 8 + 9)
    assert out.shape == (1, 2, 2) and out[0].tolist() == [[3.0 * 28, 3.0 * 24], [3.0 * 16, 3.0 * 12]]
    out = head_restated(y1, Wt.numpy(), bc.numpy(), b2, -w3, 10.0, 0.5, (2, 2))
    assert out[0].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    b2[4] = -80.0
    out = head_restated(y1, Wt.numpy(), bc.numpy(), b2, w3, 1.0, 2.0, (2, 2))
    assert out[0].tolist() == [[10.0, 2.0], [2.0, 2.0]]


def test_exact_family_is_exact():
    """Every Z value of the exact family is an exact float32 in any summation order: the restated chain equals the float64 matrix product."""
    y1, b1, W, _, _ = exact_inputs(2, (5, 7), 64, 1)
    Wt, bc = head_conv2_compose(W, b1)
    z = z_restated(y1.numpy(), Wt.numpy(), bc.numpy())
    z64 = (y1.double().reshape(-1, 64) @ Wt.double().t() + bc.double()).reshape(z.shape).numpy()
    assert np.array_equal(z.astype(np.float64), z64) and np.abs(z64).max() < 1024


@pytest.mark.parametrize("case", F64_CASES, ids=F64_IDS)
def test_float64_cases_clip_about_half_and_leave_nothing_out(case):
    """The conditions of tests/test_hip_head_gather.py's float64 bars that depend on the reference alone: with b3 = -mean(pre) the last ReLU clips a share of the
    reference within (0.2, 0.8), and at most 1 % of the pixels lie within 1e-6 of the range of 0 in front of it."""
    _, _, size, _ = case
    x, b_in, W, b2, w3 = f64_inputs(case)
    pre, _ = tail64(chain64(x, b_in, W, size), b2, w3, 0.0, 1.0)
    b3 = -float(pre.mean())
    _, ref = tail64(chain64(x, b_in, W, size), b2, w3, b3, 1.5)
    clipped = float((ref == 0).double().mean())
    left_out = float(((pre + b3).abs() <= 1e-6 * float(pre.max() - pre.min())).double().mean())
    assert 0.2 < clipped < 0.8 and left_out <= 0.01, (clipped, left_out)
