"""GPU tests (-m gpu) of the fp16x2 tile convolutions vd3d_conv3x3_s1_x2 and vd3d_conv3x3_s2_x2 (csrc/vd3d_conv_x2t.hip: the 8 x 32 tile kernel of
vd3d_conv_x3.h with two fp16 terms per operand, three products per MAC and weights pre-scaled per output channel).

Float32-faithful against FLOAT64 beside PyTorch's float32 CPU convolution (the bars of test_conv3x3_x2_is_float32_faithful); exact integer cases that pin the
geometry, the second-term products, the channel scale and the rounding of the split; the range contract of include/vd3d.h with the statements of
tests/test_hip_operand_range.py (small magnitudes, the 65 504 ceiling, containment of a non-finite input); both device packers against the numpy statement of
tests/test_conv_fp16x2_host.py, every byte; the refusals."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
CL = torch.channels_last

from test_conv_fp16x2_host import x2_image_reference                                             # noqa: E402
from test_hip_operand_range import _pow2_uniform, _tile_max, x2_small_bound, x2_split_error     # noqa: E402
from test_hip_self_contained import S2_CASES                                                     # noqa: E402


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _conv(R, stride, x, w, img=None):
    pack, run = (R.conv3x3_s1_x2_pack, R.conv3x3_s1_x2) if stride == 1 else (R.conv3x3_s2_x2_pack, R.conv3x3_s2_x2)
    img = pack(w) if img is None else img
    assert img is not None
    return run(x.contiguous(memory_format=CL), img, w.shape[0])


S1_CASES = [(1, 1, 1, 16, 32),        # one pixel
            (1, 8, 32, 16, 64),       # exactly one tile
            (2, 9, 33, 48, 128),      # one past the tile on both axes, three chunks, batch 2
            (1, 13, 47, 48, 256),     # two channel slices, ragged
            (3, 19, 33, 64, 64),      # the small map the old size rule sent to the library
            (1, 5, 9, 1024, 256),     # 576 K steps
            (1, 37, 66, 256, 256)]    # DA-V2-Large


def _err(y, ref, scale):
    return float(((y.double() - ref).abs() / scale).max()), float((y.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


@pytest.mark.parametrize("stride,B,H,W,Cin,Cout", [(1,) + c for c in S1_CASES] + [(2,) + c for c in S2_CASES])
def test_conv_fp16x2_is_float32_faithful(R, stride, B, H, W, Cin, Cout):
    """Against a float64 convolution, beside PyTorch's float32 CPU convolution on the same operands: maximum of |y - y64| / conv(|x|, |w|) <= max(2.5 x the
    yardstick's, 2^-21), relative RMS <= 1.5 x the yardstick's + 1e-9.  Post-ReLU inputs with log-normal channel scales.  Two calls return identical bits."""
    g = torch.Generator(device="cuda").manual_seed(B * 100 + H)
    x = torch.relu(torch.randn(B, Cin, H, W, device="cuda", generator=g)) * torch.exp(torch.randn(1, Cin, 1, 1, device="cuda", generator=g))
    x = x.contiguous(memory_format=CL)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) * 0.05
    img = (R.conv3x3_s1_x2_pack if stride == 1 else R.conv3x3_s2_x2_pack)(w)
    y = _conv(R, stride, x, w, img)
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    assert y.shape == (B, Cout, Ho, Wo) and y.is_contiguous(memory_format=CL) and bool(torch.isfinite(y).all())
    ref = F.conv2d(x.double(), w.double(), None, stride, 1)
    y32 = F.conv2d(x.cpu(), w.cpu(), None, stride, 1).to(x.device)
    scale = F.conv2d(x.abs().double(), w.abs().double(), None, stride, 1) + 1e-30
    (e3, r3), (e32, r32) = _err(y, ref, scale), _err(y32, ref, scale)
    print(f"CONV_S{stride}_X2_ERR {B}x{H}x{W}x{Cin}->{Cout} max {e3:.3e} (f32 {e32:.3e}, {e3 / max(e32, 1e-30):.2f}x) rms {r3:.3e} (f32 {r32:.3e}, {r3 / max(r32, 1e-30):.2f}x)")
    assert e3 <= max(2.5 * e32, 2.0 ** -21), (e3, e32)
    assert r3 <= 1.5 * r32 + 1e-9, (r3, r32)
    assert torch.equal(_conv(R, stride, x, w, img), y)


def _exact(R, stride, x, w):
    assert float(F.conv2d(x.abs().double(), w.abs().double(), None, stride, 1).max()) < 2 ** 24    # every sum is exact in any order
    return torch.equal(_conv(R, stride, x, w).double(), F.conv2d(x.double(), w.double(), None, stride, 1))


@pytest.mark.parametrize("stride,Cout", [(1, 32), (1, 64), (1, 128), (1, 256), (2, 128), (2, 384)])
def test_conv_fp16x2_exact_small_integers_pin_the_geometry(R, stride, Cout):
    """(a) Small integers on both sides: one fp16 term per operand, power-of-two channel scales, so the answer is the integer one -- a swapped sub-pixel, a
    mirrored tap, a shifted halo, a swapped channel half, a permuted channel slice shows.  Odd sizes on both axes, two frames, three chunks."""
    B, Cin, H, W = 2, 48, 21, 45
    x = ((torch.arange(B * Cin * H * W, device="cuda").view(B, Cin, H, W) * 7) % 5 - 2).float()
    w = ((torch.arange(Cout * Cin * 9, device="cuda").view(Cout, Cin, 3, 3) * 11) % 7 - 3).float()
    assert _exact(R, stride, x, w)


def _odd_ints(shape, lo, hi, g):
    v = torch.randint(lo, hi, shape, device="cuda", generator=g) | 1
    s = torch.randint(0, 2, shape, device="cuda", generator=g) * 2 - 1
    return (v * s).float()


def _sparse_signs(Cout, Cin, g, nz=6):
    """[Cout][Cin][3][3] from {-1, 0, 1} with `nz` non-zeros per output channel."""
    idx = torch.rand(Cout, Cin * 9, device="cuda", generator=g).argsort(dim=1)[:, :nz]           # nz distinct positions per row
    sign = (torch.randint(0, 2, (Cout, nz), device="cuda", generator=g) * 2 - 1).float()
    return torch.zeros(Cout, Cin * 9, device="cuda").scatter_(1, idx, sign).view(Cout, Cin, 3, 3)


@pytest.mark.parametrize("stride,Cout", [(1, 32), (1, 64), (1, 256), (2, 128), (2, 384)])
def test_conv_fp16x2_exact_second_terms(R, stride, Cout):
    """(b) Odd integers in [2^11, 2^12) need both fp16 terms (12 significant bits).  On the activation side against sparse +-1 weights (six per output
    channel), then on the weight side (whose channel scale 2^2 must be undone exactly) against activations from {-1, 0, 1}: a dropped x2 w1 or x1 w2, or a
    channel scale that does not cancel, gives a wrong integer."""
    B, Cin, H, W = 2, 48, 13, 37
    g = torch.Generator(device="cuda").manual_seed(40 + Cout + stride)
    assert _exact(R, stride, _odd_ints((B, Cin, H, W), 2 ** 11, 2 ** 12, g), _sparse_signs(Cout, Cin, g))
    xs = torch.randint(-1, 2, (B, Cin, H, W), device="cuda", generator=g).float()
    assert _exact(R, stride, xs, _odd_ints((Cout, Cin, 3, 3), 2 ** 11, 2 ** 12, g))


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_fp16x2_split_rounds_to_nearest(R, stride):
    """x = h - (1/2 + 2^-11) with h an even integer in (2^11, 2^12): 23 significant bits that round-to-nearest splits exactly (h, then a NEGATIVE second term
    of 11 bits) and truncation cannot (its remainder 2 - 1/2 - 2^-11 needs 12).  One +-1 weight per output channel (the centre tap of one input channel; the
    other way round for the weights): every output is +-one operand, so it must come back bit for bit."""
    B, Cin, H, W, Cout = 1, 32, 11, 35, 128
    g = torch.Generator(device="cuda").manual_seed(50 + stride)
    v = lambda shape: (torch.randint(2 ** 10 + 1, 2 ** 11, shape, device="cuda", generator=g) * 2).float() - (0.5 + 2.0 ** -11)   # noqa: E731
    x = v((B, Cin, H, W))
    assert float((x.half().float() - x).min()) > 0                      # the first term rounds UP everywhere
    w = torch.zeros(Cout, Cin, 3, 3, device="cuda")
    ci = torch.arange(Cout, device="cuda") % Cin
    w[torch.arange(Cout, device="cuda"), ci, 1, 1] = (torch.arange(Cout, device="cuda") % 2 * 2 - 1).float()
    assert torch.equal(_conv(R, stride, x, w), F.conv2d(x.double(), w.double(), None, stride, 1).float())
    w2 = torch.zeros(Cout, Cin, 3, 3, device="cuda")
    w2[torch.arange(Cout, device="cuda"), ci, 1, 1] = v((Cout,))
    xs = torch.randint(-1, 2, (B, Cin, H, W), device="cuda", generator=g).float()
    assert torch.equal(_conv(R, stride, xs, w2), F.conv2d(xs.double(), w2.double(), None, stride, 1).float())


# ---- the range contract (include/vd3d.h), with the statements of tests/test_hip_operand_range.py
RB, RH, RW, RCIN, RCOUT = 2, 21, 45, 48, 64


def _rcout(stride):
    return RCOUT if stride == 1 else 128     # the stride-2 form builds multiples of 128


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("lo,hi", [(-12, -6), (-20, -12)])   # second fp16 term subnormal; second term gone
def test_conv_x2_small_magnitude_contract(R, stride, lo, hi):
    """x = +-2^u, u uniform in [lo, hi): |y - y64| <= per + 2^-21 S + 2 A per element (x2_small_bound), A the float32 CPU convolution's own error per 8 x 32
    output tile.  A split that flushes the subnormal second term to zero breaks the bound in the first range."""
    Cout = _rcout(stride)
    g = torch.Generator(device="cuda").manual_seed(2000 - lo + stride)
    x = _pow2_uniform((RB, RCIN, RH, RW), lo, hi, g).contiguous(memory_format=CL)
    w = torch.randn(Cout, RCIN, 3, 3, device="cuda", generator=g) * 0.05
    y = _conv(R, stride, x, w)
    y64 = F.conv2d(x.double(), w.double(), None, stride, 1)
    S = F.conv2d(x.abs().double(), w.abs().double(), None, stride, 1)
    y32 = F.conv2d(x.cpu(), w.cpu(), None, stride, 1).to(x.device)
    A = _tile_max((y32.double() - y64).abs().amax(dim=1, keepdim=True), (8, 32)).expand_as(y64)
    bound = x2_small_bound(F.conv2d(x2_split_error(x.abs().double()), w.abs().double(), None, stride, 1), S, A)
    err = (y.double() - y64).abs()
    print(f"CONV_S{stride}_X2_SMALL u in [{lo}, {hi}]: max err / bound {float((err / bound).max()):.3f}, err / (per + 2^-21 S) {float((err / (bound - 2 * A)).max()):.3f}")
    assert bool(torch.isfinite(y).all())
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_x2_ceiling(R, stride):
    """|x| in [2^13, 65 504) meets the faithful bar; one element 1e5 makes exactly the outputs whose 3 x 3 window holds it non-finite, over all output channels,
    and leaves every other output bit-identical to the run with 1.0 in its place."""
    Cout = _rcout(stride)
    g = torch.Generator(device="cuda").manual_seed(33 + stride)
    w = torch.randn(Cout, RCIN, 3, 3, device="cuda", generator=g) * 0.05
    img = (R.conv3x3_s1_x2_pack if stride == 1 else R.conv3x3_s2_x2_pack)(w)
    x = _pow2_uniform((RB, RCIN, RH, RW), 13.0, math.log2(65504.0), g).clamp(-65503.0, 65503.0).contiguous(memory_format=CL)
    y = _conv(R, stride, x, w, img)
    assert bool(torch.isfinite(y).all())
    ref = F.conv2d(x.double(), w.double(), None, stride, 1)
    y32 = F.conv2d(x.cpu(), w.cpu(), None, stride, 1).to(x.device)
    scale = F.conv2d(x.abs().double(), w.abs().double(), None, stride, 1)
    (e3, r3), (e32, r32) = _err(y, ref, scale), _err(y32, ref, scale)
    print(f"CONV_S{stride}_X2_CEILING max {e3:.3e} (f32 {e32:.3e}) rms {r3:.3e} (f32 {r32:.3e})")
    assert e3 <= max(2.5 * e32, 2.0 ** -21), (e3, e32)
    assert r3 <= 1.5 * r32 + 1e-9, (r3, r32)
    x = torch.randn(RB, RCIN, RH, RW, device="cuda", generator=g).contiguous(memory_format=CL)
    for bb, c, i, j in ((0, 0, 0, 0), (1, 47, 20, 44), (1, 17, 15, 32), (0, 9, 8, 31)):    # a corner, the last element, tile boundaries in both directions
        x[bb, c, i, j] = 1.0
        clean = _conv(R, stride, x, w, img)
        x[bb, c, i, j] = 1.0e5
        y = _conv(R, stride, x, w, img)
        x[bb, c, i, j] = 1.0
        q = torch.arange(y.shape[2], device="cuda").view(-1, 1) * stride
        r = torch.arange(y.shape[3], device="cuda").view(1, -1) * stride
        hit = torch.zeros(RB, 1, y.shape[2], y.shape[3], dtype=torch.bool, device="cuda")
        hit[bb, 0] = (q - 1 <= i) & (i <= q + 1) & (r - 1 <= j) & (j <= r + 1)
        assert 1 <= int(hit.sum()) <= 9
        hit = hit.expand_as(y)
        assert not bool(torch.isfinite(y[hit]).any()), (bb, c, i, j)
        assert torch.equal(y[~hit], clean[~hit]), (bb, c, i, j)


@pytest.mark.parametrize("py,px", [(4, 6), (5, 6), (4, 7), (5, 7), (0, 0), (8, 32)])
def test_conv3x3_s2_x2_nan_stays_inside_its_windows(R, py, px):
    """One NaN input pixel (each of the four sub-pixel parities, a corner, the last pixel) gives NaN in exactly the outputs whose 3 x 3 window holds it: output
    (q, r) reads rows 2 q - 1 .. 2 q + 1.  A zero-weight tap on the space-to-depth view would carry it further."""
    H, W = 9, 33
    x = torch.ones(1, 16, H, W, device="cuda")
    x[0, 5, py, px] = float("nan")
    y = _conv(R, 2, x, torch.ones(128, 16, 3, 3, device="cuda"))
    q = torch.arange((H + 1) // 2, device="cuda").view(-1, 1)
    r = torch.arange((W + 1) // 2, device="cuda").view(1, -1)
    holds = ((2 * q - 1 <= py) & (py <= 2 * q + 1) & (2 * r - 1 <= px) & (px <= 2 * r + 1))
    assert 1 <= int(holds.sum()) <= 4
    assert torch.equal(torch.isnan(y[0]), holds.expand(128, -1, -1))


@pytest.mark.parametrize("stride,Cout,Cin", [(1, 32, 16), (1, 64, 48), (1, 256, 48), (2, 128, 16), (2, 256, 48)])
def test_conv_fp16x2_weight_image_is_the_numpy_statement(R, stride, Cout, Cin):
    """The device packer against x2_image_reference, every byte: exponents, both terms, the step order, the channel scales, the zero page.  Channel magnitudes
    spread over e^+-3, one all-zero channel, one channel whose largest weight sits just below a power of two."""
    w = torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(9 + Cout)) * 0.05 * torch.exp(torch.randn(Cout, 1, 1, 1, generator=torch.Generator().manual_seed(Cout)) * 3)
    w[3] = 0.0
    w[5] = w[5].clamp(-0.2, 0.2)
    w[5, 0, 0, 0] = float(np.float32(0.25) - np.float32(2.0 ** -26))
    img = (R.conv3x3_s1_x2_pack if stride == 1 else R.conv3x3_s2_x2_pack)(w.cuda())
    assert np.array_equal(img.cpu().numpy(), x2_image_reference(w.numpy(), stride))


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_fp16x2_refuses_what_it_does_not_build(R, stride):
    from visiondepth3d_amd import _lib
    L = _lib.lib()
    pack = R.conv3x3_s1_x2_pack if stride == 1 else R.conv3x3_s2_x2_pack
    run = L.vd3d_conv3x3_s1_x2 if stride == 1 else L.vd3d_conv3x3_s2_x2
    packw = L.vd3d_conv3x3_s1_x2_pack_weights if stride == 1 else L.vd3d_conv3x3_s2_x2_pack_weights
    assert pack(torch.zeros(96, 16, 3, 3, device="cuda")) is None       # C_out 96
    assert pack(torch.zeros(128, 24, 3, 3, device="cuda")) is None      # C_in 24
    assert pack(torch.zeros(128, 16, 1, 1, device="cuda")) is None      # not 3 x 3
    assert (R.conv3x3_s2_x2_pack(torch.zeros(64, 16, 3, 3, device="cuda")) is None) and (R.conv3x3_s1_x2_pack(torch.zeros(512, 16, 3, 3, device="cuda")) is None)
    img = pack(torch.zeros(128, 16, 3, 3, device="cuda"))
    buf = torch.zeros(2 * 16 * 4 * 4 + 4, device="cuda")
    out = torch.zeros(2 * 128 * 4 * 4, device="cuda")
    vp = ctypes.c_void_p
    call = lambda xp, B, Cin=16, Cout=128, H=4, ip=img.data_ptr(): run(R._ctx, vp(xp), B, H, 4, Cin, vp(ip), Cout, vp(out.data_ptr()))   # noqa: E731
    assert call(buf.data_ptr(), 1, Cout=96) == -4 and b"C_out" in L.vd3d_last_error()
    assert call(buf.data_ptr(), 1, Cin=24) == -4 and b"C_in" in L.vd3d_last_error()
    assert call(buf.data_ptr() + 4, 1) == -4 and b"aligned" in L.vd3d_last_error()                       # a misaligned input
    assert call(buf.data_ptr(), 1, ip=img.data_ptr() + 8) == -4 and b"aligned" in L.vd3d_last_error()    # a misaligned image
    assert call(buf.data_ptr(), 0) == -4 and b"batch" in L.vd3d_last_error()
    assert call(buf.data_ptr(), 65536) == -4 and b"batch" in L.vd3d_last_error()
    assert call(buf.data_ptr(), 1, H=0) == -4 and b"map" in L.vd3d_last_error()
    assert packw(R._ctx, vp(buf.data_ptr()), 16, 96, vp(img.data_ptr())) == -4 and b"C_out" in L.vd3d_last_error()
    assert packw(R._ctx, vp(buf.data_ptr()), 16, 128, vp(img.data_ptr() + 8)) == -4 and b"aligned" in L.vd3d_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0   # nothing ran
