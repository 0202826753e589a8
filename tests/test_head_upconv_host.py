"""Host side of the float32 head's "coarse GEMM + fine gather" route (depth.py head_upconv_compose, csrc/vd3d_head_upconv.hip): the composed form is the module
chain in float64, tap order and channel layout, the refusals, the C boundary, and the kernel's statement restated in NumPy with an exact fused multiply-add (the
reference tests/test_hip_head_upconv.py compares the kernel's bits with).  No GPU needed."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from visiondepth3d_amd import _abi, _lib
from visiondepth3d_amd.depth import HEAD_UPCONV_BUILT, head_upconv_compose

MAPS = (((1, 1), (2, 2)), ((2, 3), (4, 6)), ((5, 7), (10, 14)), ((5, 7), (9, 13)), ((9, 5), (9, 5)))   # the last two: a non-integer factor, factor 1
MAP_IDS = ["%dx%d-%dx%d" % (a + b) for a, b in MAPS]
TILE = (16, 32)   # the kernel's fine tile at up-sampling factors of about 2 and more (HU_TH x HU_TW)


def _taps(n_in, n_out, ft):
    """upsample_bilinear_f32_body's coordinates, operation for operation, in the float type ``ft``: s = (ft)(n_in - 1) / (ft)(n_out - 1), f = s * (ft)y, truncation,
    the < n_in - 1 clamp, l1 = f - (ft)i0, l0 = 1 - l1."""
    s = ft(n_in - 1) / ft(n_out - 1)
    f = s * np.arange(n_out).astype(ft)
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = f - i0.astype(ft)
    l0 = ft(1) - l1
    return i0, i1, l0, l1


def fma32(a, b, c):
    """round_to_float32(a * b + c), exactly, for float32 arrays: the float64 product of two float32 values is exact; the float64 sum is rounded once more before the
    rounding to float32, which differs from the single rounding only where the float64 sum is inexact AND lands on a float32 tie; those elements are redone in
    rational arithmetic."""
    a, b, c = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, np.float32)) for v in (a, b, c)))
    p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c64
    r = s.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r64 = r.astype(np.float64)
        other = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
        tie = np.isfinite(s) & np.isfinite(other) & (s != r64) & (np.abs(s - r64) == np.abs(other - s))
    if tie.any():
        r = r.copy()
        for i in zip(*np.nonzero(tie)):
            exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
            lo, hi = sorted((float(r64[i]), float(other[i])))
            mid = (Fraction(lo) + Fraction(hi)) / 2
            if exact != mid:   # (an exact tie keeps NumPy's round-half-even result)
                r[i] = np.float32(hi if exact > mid else lo)
    return r


def gather_restated(z, H, W, ft=np.float32):
    """vd3d_head_upconv_gather_f32's statement: z [B, h, w, 9, CO] -> [B, H, W, CO];
        y1[b, Y, X, o] = sum over t = 3 ky + kx ascending with (Y + ky - 1, X + kx - 1) inside [0, H) x [0, W) of bilinear(z[b, :, :, t, o]; Y + ky - 1, X + kx - 1)
    ``ft`` = float32: the kernel's arithmetic -- corner weights ly * lx as rounded products, one fused-multiply-add chain from 0, taps ascending, corners (y0, x0),
    (y0, x1), (y1, x0), (y1, x1).  ``ft`` = float64: the same statement in plain float64."""
    z = np.asarray(z, ft)
    B, h, w, nine, CO = z.shape
    assert nine == 9 and H >= 2 and W >= 2
    y0, y1, ly0, ly1 = _taps(h, H, ft)
    x0, x1, lx0, lx1 = _taps(w, W, ft)
    acc = np.zeros((B, H, W, CO), ft)
    Y, X = np.arange(H), np.arange(W)
    for ky in range(3):
        ys = Y + ky - 1
        vy = (ys >= 0) & (ys < H)
        yc = np.clip(ys, 0, H - 1)
        for kx in range(3):
            xs = X + kx - 1
            vx = (xs >= 0) & (xs < W)
            xc = np.clip(xs, 0, W - 1)
            valid = (vy[:, None] & vx[None, :])[None, :, :, None]
            zt = z[:, :, :, 3 * ky + kx, :]
            for (yi, ly), (xi, lx) in (((y0, ly0), (x0, lx0)), ((y0, ly0), (x1, lx1)), ((y1, ly1), (x0, lx0)), ((y1, ly1), (x1, lx1))):
                wgt = (ly[yc][:, None] * lx[xc][None, :]).astype(ft)[None, :, :, None]
                zc = zt[:, yi[yc]][:, :, xi[xc]]
                new = fma32(wgt, zc, acc) if ft is np.float32 else acc + wgt * zc
                acc = np.where(valid, new, acc)
    return acc


def chain64(x, pw, pb, cw, size):
    """The module chain in float64: projection with bias, F.interpolate(bilinear, align_corners=True), conv1 with zero padding and no bias."""
    up = F.interpolate(F.conv2d(x.double(), pw.double(), pb.double()), size=tuple(size), mode="bilinear", align_corners=True)
    return F.conv2d(up, cw.double(), None, padding=1)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.mark.parametrize("cc", HEAD_UPCONV_BUILT, ids=["%d-%d" % p for p in HEAD_UPCONV_BUILT])
@pytest.mark.parametrize("hw,HW", MAPS, ids=MAP_IDS)
def test_composed_form_is_the_module_chain_in_float64(hw, HW, cc):
    C, Co = cc
    g = torch.Generator().manual_seed(1000 * hw[0] + 100 * hw[1] + HW[0] + C)
    x = torch.randn(2, C, *hw, generator=g, dtype=torch.float64)
    pw = torch.randn(C, C, 1, 1, generator=g, dtype=torch.float64) / C ** 0.5
    pb = torch.randn(C, generator=g, dtype=torch.float64)
    cw = torch.randn(Co, C, 3, 3, generator=g, dtype=torch.float64) / (3.0 * C ** 0.5)
    ref = chain64(x, pw, pb, cw, HW)
    Wc, bc = head_upconv_compose(pw, pb, cw, dtype=torch.float64)
    assert Wc.shape == (9 * Co, C) and bc.shape == (9 * Co,)
    z = (x.permute(0, 2, 3, 1).reshape(-1, C) @ Wc.t() + bc).reshape(2, hw[0], hw[1], 9, Co)
    got = torch.from_numpy(gather_restated(z.numpy(), HW[0], HW[1], np.float64)).permute(0, 3, 1, 2)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.max() - ref.min())
    # a [C, C_in] projection weight is the same projection; without a bias: the same matrix and a zero bias vector
    W2, b2 = head_upconv_compose(pw.reshape(C, C), None, cw, dtype=torch.float64)
    assert torch.equal(W2, Wc) and not bool(b2.any())
    # the float32 result is the float64 one rounded once
    W32, b32 = head_upconv_compose(pw.float(), pb.float(), cw.float())
    W64, b64 = head_upconv_compose(pw.float(), pb.float(), cw.float(), dtype=torch.float64)
    assert W32.dtype == torch.float32 and torch.equal(W32, W64.float()) and torch.equal(b32, b64.float())


def test_tap_order_and_channel_layout():
    """Channel t * Co + o with t = 3 ky + kx: Wc[t Co + o, i] = sum_c conv1_w[o, c, ky, kx] proj_w[c, i], bc[t Co + o] = sum_c conv1_w[o, c, ky, kx] proj_b[c]."""
    g = torch.Generator().manual_seed(3)
    C, Ci, Co = 5, 4, 3
    pw, pb, cw = (torch.randint(-3, 4, s, generator=g).double() for s in ((C, Ci, 1, 1), (C,), (Co, C, 3, 3)))
    Wc, bc = head_upconv_compose(pw, pb, cw, dtype=torch.float64)
    assert Wc.shape == (9 * Co, Ci) and bc.shape == (9 * Co,)
    for ky in range(3):
        for kx in range(3):
            for o in range(Co):
                row = (3 * ky + kx) * Co + o
                assert torch.equal(Wc[row], cw[o, :, ky, kx] @ pw[:, :, 0, 0]) and float(bc[row]) == float(cw[o, :, ky, kx] @ pb)
    # one tap, one channel pair: exactly one row of Wc is set
    cw1 = torch.zeros(Co, C, 3, 3, dtype=torch.float64)
    cw1[2, 1, 0, 2] = 1.0
    W1, b1 = head_upconv_compose(pw, pb, cw1, dtype=torch.float64)
    rows = torch.nonzero(W1.abs().sum(1)).flatten().tolist()
    assert rows == [(3 * 0 + 2) * Co + 2] and torch.equal(W1[rows[0]], pw[1, :, 0, 0]) and float(b1[rows[0]]) == float(pb[1])


def test_wrong_argument_shapes_are_refused():
    pw, pb, cw = torch.zeros(5, 4, 1, 1), torch.zeros(5), torch.zeros(3, 5, 3, 3)
    head_upconv_compose(pw, pb, cw)
    for bad in ((pw, pb, torch.zeros(3, 5, 1, 1)),         # not a 3 x 3 convolution
                (pw, pb, torch.zeros(3, 4, 3, 3)),         # the convolution reads the projection's OUTPUT channels
                (torch.zeros(5, 4, 3, 3), pb, cw),         # not a 1 x 1 projection
                (pw, torch.zeros(4), cw),                  # the bias belongs to the projection's output channels
                (pw[0], pb, cw)):
        with pytest.raises(ValueError):
            head_upconv_compose(*bad)


def test_c_boundary(L):
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    declared = set(re.findall(r"\b(vd3d_[a-z0-9_]+)\s*\(", hdr))
    n = "vd3d_head_upconv_gather_f32"
    assert n in declared and n in _lib.EXPORTS and declared == set(_lib.EXPORTS) and hasattr(L, n)
    assert re.search(r"Additions since 6 that leave the version as it is.*?" + n + r".*?\*/\s*#define VD3D_ABI_VERSION 6", hdr, re.S)
    assert _abi.ABI_VERSION == 6 and L.vd3d_abi_version() == 6
    f = L.vd3d_head_upconv_gather_f32
    # the shape is judged first: a refusal needs neither a context nor a device
    for Cout in (16, 48, 128, 0):
        assert f(None, None, 1, 5, 7, 10, 14, Cout, None) == _abi.E_UNSUPPORTED and b"not built" in L.vd3d_last_error()
    for B, h, w, H, W in ((0, 5, 7, 10, 14), (1, 0, 7, 10, 14), (1, 5, 0, 10, 14), (1, 5, 7, 1, 14), (1, 5, 7, 10, 1),
                          (1, 400, 7, 2, 14),                 # a down-sampling factor of 399: no tile's reach fits the staged window
                          (1, 5, 1 << 22, 10, 14)):           # a coarse row of 2^22 x 576 elements
        assert f(None, None, B, h, w, H, W, 64, None) == _abi.E_UNSUPPORTED, (B, h, w, H, W)
    # built shapes (any H x W, down-sampling included) get as far as the missing arguments
    for h, w, H, W in ((5, 7, 10, 14), (5, 7, 9, 13), (9, 5, 9, 5), (1, 1, 2, 2), (148, 264, 296, 528), (40, 40, 10, 10)):
        for Cout in (64, 32):
            assert f(None, None, 1, h, w, H, W, Cout, None) == _abi.E_INVALID, (h, w, H, W)


def test_exact_fma_restatement():
    """fma32 against rational arithmetic.  The traps: c = 2^30 + 2^7 (float32 ulp 2^7, odd mantissa; the tie with its even upper neighbour is c + 2^6) and
    a * b = (2^3 + 2^-20)(2^3 - 2^-20) = 2^6 - 2^-40, an exact float64.  The exact sum lies BELOW the tie, the float64 sum (ulp 2^-22) lands ON it, and
    round-half-even would then go up to 2^30 + 2^8.  Mirrored with c = -(2^30 + 2^7): the exact sum's magnitude lies ABOVE the tie to the even -2^30."""
    a, b = np.float32(2.0 ** 3 + 2.0 ** -20), np.float32(2.0 ** 3 - 2.0 ** -20)
    assert Fraction(float(a)) * Fraction(float(b)) == Fraction(2 ** 6) - Fraction(1, 2 ** 40)
    c = np.float32(2.0 ** 30 + 2.0 ** 7)
    assert float(np.float32(np.float64(a) * np.float64(b) + np.float64(c))) == 2.0 ** 30 + 2.0 ** 8        # what the two roundings alone give
    assert float(fma32(a, b, c)[0]) == 2.0 ** 30 + 2.0 ** 7
    assert float(np.float32(np.float64(a) * np.float64(b) + np.float64(-c))) == -(2.0 ** 30)
    assert float(fma32(a, b, -c)[0]) == -(2.0 ** 30 + 2.0 ** 7)
    # exact ties go to even, and the array form treats each element on its own
    e = np.float32(2.0 ** 3)
    got = fma32(np.array([e, e, a, a], np.float32), np.array([e, e, b, b], np.float32), np.array([2.0 ** 30, c, c, -c], np.float32))
    assert got.tolist() == [2.0 ** 30, 2.0 ** 30 + 2.0 ** 8, 2.0 ** 30 + 2.0 ** 7, -(2.0 ** 30 + 2.0 ** 7)]
    # random operands: no float32 is nearer to the exact value than the result
    rng = np.random.default_rng(5)
    x, y, z = (rng.standard_normal(700).astype(np.float32) for _ in range(3))
    got = fma32(x, y, z)
    for i in range(700):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        d = abs(exact - Fraction(float(got[i])))
        for nb in (np.nextafter(got[i], np.float32(np.inf)), np.nextafter(got[i], np.float32(-np.inf))):
            assert d <= abs(exact - Fraction(float(nb)))


def test_restatement_on_a_hand_computed_map():
    """1 x 1 -> 2 x 2: every sample is the single coarse pixel with weight 1 (l1 = 0), so an output is the plain float32 sum of the taps inside the map, ascending;
    2 x 2 -> 3 x 3 centre pixel: the taps' samples at (0.5, 0.5) steps."""
    z = np.arange(1, 10, dtype=np.float32).reshape(1, 1, 1, 9, 1)
    y = gather_restated(z, 2, 2)[0, :, :, 0]
    # pixel (0, 0): taps with ky, kx in {1, 2}: t = 4, 5, 7, 8 -> z = 5 + 6 + 8 + 9
    assert y[0, 0] == 28 and y[0, 1] == 4 + 5 + 7 + 8 and y[1, 0] == 2 + 3 + 5 + 6 and y[1, 1] == 1 + 2 + 4 + 5
    z = np.zeros((1, 2, 2, 9, 1), np.float32)
    z[0, :, :, 4, 0] = [[1, 2], [3, 4]]      # the centre tap alone: the plain up-sampling
    y = gather_restated(z, 3, 3)[0, :, :, 0]
    assert np.array_equal(y, np.array([[1, 1.5, 2], [2, 2.5, 3], [3, 3.5, 4]], np.float32))
    z[0, :, :, 4, 0] = 0
    z[0, :, :, 0, 0] = [[1, 2], [3, 4]]      # tap (ky, kx) = (0, 0) alone: the up-sampled map shifted by (+1, +1), zero where the sample is outside
    y = gather_restated(z, 3, 3)[0, :, :, 0]
    assert np.array_equal(y, np.array([[0, 0, 0], [0, 1, 1.5], [0, 2, 2.5]], np.float32))
