"""Exact-arithmetic GPU tests of the fp16 up-scale convolutions: vd3d_conv3x3_c64_f16 in every launch regime and on both sides of its kernel switch,
vd3d_conv3x3_head_f16, vd3d_conv3x3_dense_f16 and vd3d_nhwc_f16_to_planar3_f32 on BITS, at tile and range edges, and the refusals of the entry points.

Integer data (tests/upscale_exact.py; its preconditions are asserted by tests/test_upscale_exact_host.py) makes the float32 accumulator exact in any
summation order, so the expected bytes are a float64 sum, the epilogue's float32 operations in numpy and one rounding to fp16: no tolerance anywhere.
Every c64 case asserts the launch regime (one-round / persistent / tile16) it was written for from the device's CU count, so coverage cannot drift."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upscale_exact as UE  # noqa: E402
from test_hip_rrdb import SHAPES  # noqa: E402

CL = torch.channels_last


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def n_cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _bias(c, seed, zero=False):
    """Non-dyadic float32 values of both signs: `acc + bias` and `* slope` round for real.  (Zero for the scaled data sets, whose point is the bare range.)"""
    return torch.zeros(c) if zero else torch.randn(c, generator=torch.Generator().manual_seed(1000 + seed)) * 0.37


def _slope(c, seed):
    return torch.rand(c, generator=torch.Generator().manual_seed(2000 + seed)) * 0.5 + 0.01


def _same_bits(got, exp):
    """got, exp: int16 arrays of one shape.  On a mismatch the message says how many, where first, and what."""
    if np.array_equal(got, exp):
        return True
    bad = np.argwhere(got != exp)
    i = tuple(bad[0])
    print(f"{len(bad)} of {got.size} differ; first at (y, x, c) = {tuple(int(j) for j in i)}: got {float(got.view(np.float16)[i])!r} "
          f"({int(got[i]) & 0xffff:#06x}), expected {float(exp.view(np.float16)[i])!r} ({int(exp[i]) & 0xffff:#06x}); "
          f"rows {sorted(set(bad[:, 0].tolist()))[:8]}, columns {sorted(set(bad[:, 1].tolist()))[:8]}")
    return False


# ---- vd3d_conv3x3_c64_f16 ------------------------------------------------------------------------------------------------------------------
def _run_c64(R, x, w, b, sl):
    """x fp16 [H, W, 64] on the device, w fp16 [64, 64, 3, 3], b / sl float32 [64] (sl may be None) -> fp16 [H, W, 64] on the device."""
    from visiondepth3d_amd.upscale import conv_weight_fragments
    got = R.conv3x3_c64(UE.nchw(x), conv_weight_fragments(w).cuda(), b.cuda(), sl.cuda() if sl is not None else None)
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and tuple(got.shape) == (1, 64, x.shape[0], x.shape[1]) and got.is_contiguous(memory_format=CL)
    return UE.hwc(got)


def _check_c64(R, H, W, scale="unit"):
    seed = H * 7 + W
    x, w = UE.int_data(H, W, 64, 64, seed, scale=scale, device="cuda")
    acc = UE.ref_acc64(x, w)
    b = _bias(64, seed, zero=scale != "unit")
    first = None
    for sl in (None, _slope(64, seed)):
        exp = UE.expect_c64(acc, b.numpy(), None if sl is None else sl.numpy())
        assert _same_bits(UE.bits(_run_c64(R, x, w, b, sl)), exp.view(np.int16)), (H, W, scale, "slope" if sl is not None else "no slope")
        first = exp if first is None else first
    return first          # the expectation without a slope


def _persistent_shape(n_cu, kind):
    """(H, W) with 11 tile columns (W = 330, W % 32 == 10) and more tiles than workgroups, derived from the device's slots."""
    slots, ntx = UE.c64_slots(n_cu), 11

    def nty_above(lo, residue):      # the fewest tile rows with ntx * nty > lo and ntx * nty % 8 == residue (None: any but 0)
        nty = lo // ntx + 1
        while (ntx * nty) % 8 != residue if residue is not None else (ntx * nty) % 8 == 0:
            nty += 1
        return nty
    if kind == "mod8-1":
        return 8 * nty_above(slots, 1), 330
    if kind == "mod8-7-ragged":
        return 8 * nty_above(slots, 7) - 3, 330
    assert kind == "three-rounds"
    return 8 * nty_above(2 * slots, None) - 1, 330


@pytest.mark.parametrize("H,W", [(1, 1), (8, 32), (9, 33), (17, 65)])
def test_c64_one_round(R, n_cu, H, W):
    """Every workgroup of the 32 x 8 kernel has one tile: one pixel, exactly one tile, one past it both ways, 3 x 3 tiles with ragged edges."""
    assert UE.c64_regime(H, W, n_cu)[0] == "one-round"
    _check_c64(R, H, W)


@pytest.mark.parametrize("kind", ["mod8-1", "mod8-7-ragged", "three-rounds"])
def test_c64_persistent_with_a_ragged_last_band(R, n_cu, kind):
    """More tiles than workgroups, and a tile count that is no multiple of 8: the last XCD's band is short, so in a later round some workgroup finds
    `xcd * per + it >= ntiles` (its `more == false` prefetch reads pixel 0) while its neighbours go on."""
    H, W = _persistent_shape(n_cu, kind)
    regime, ntiles, per, rounds = UE.c64_regime(H, W, n_cu)
    slots = UE.c64_slots(n_cu)
    assert regime == "persistent" and slots < ntiles <= UE.C64_SWITCH and W % 32 == 10, (regime, ntiles, slots)
    assert ntiles % 8 != 0 and 8 * per > ntiles                                     # the last band is ragged ...
    wpx = slots // 8
    assert any(it >= wpx and 7 * per + it >= ntiles for it in range(per))            # ... and a workgroup meets its end in a later round
    if kind == "mod8-1":
        assert ntiles % 8 == 1
    elif kind == "mod8-7-ragged":
        assert ntiles % 8 == 7 and H % 8 != 0
    else:
        assert rounds == 3 and per % wpx != 0 and per > 2 * wpx, (per, wpx, rounds)
    _check_c64(R, H, W)


@pytest.mark.parametrize("H,regime", [(16384, "persistent"), (16385, "tile16")])
def test_c64_either_side_of_the_kernel_switch(R, n_cu, H, regime):
    """W = 64: 4096 tiles of 32 x 8 is the last size of the 32 x 8 kernel, 4097 the first of the 32 x 16 kernel."""
    got = UE.c64_regime(H, 64, n_cu)
    assert got[0] == regime and (got[1] == 4096 if regime == "persistent" else -(-H // 8) * 2 == 4098), got
    _check_c64(R, H, 64)


@pytest.mark.parametrize("H,W", [(32769, 1), (16385, 33), (1, 131073), (17, 43713), (10929, 65), (10921, 65), (10927, 65)])
def test_c64_tile16_at_ragged_edges(R, n_cu, H, W):
    """The 32 x 16 kernel (what a 1080p frame runs) at the smallest maps that reach it: W = 1 and 33, H = 1 and 17, H % 16 in {1, 9, 15} at W = 65."""
    assert UE.c64_regime(H, W, n_cu)[0] == "tile16"
    _check_c64(R, H, W)


def test_c64_the_two_kernels_produce_identical_bytes(R, n_cu):
    """vd3d_conv.hip says so of k_conv3x3_c64 and k_conv3x3_c64_s (each output = the same 36 MFMA steps in the same order).  Random NON-integer fp16 data,
    where the summation order matters: 64 x 16 400 runs the 32 x 16 kernel, its first 16 384 rows the 32 x 8 kernel; every row whose 3 x 3 window lies
    inside both maps must agree bit for bit."""
    H, W, Hs = 16400, 64, 16384
    assert UE.c64_regime(H, W, n_cu)[0] == "tile16" and UE.c64_regime(Hs, W, n_cu)[:2] == ("persistent", 4096)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = (torch.randn((H, W, 64), device="cuda", generator=gen) * 0.7).half()
    w = (torch.randn((64, 64, 3, 3), device="cuda", generator=gen) * 0.06).half().cpu()
    b, sl = _bias(64, 5), _slope(64, 5)
    full = _run_c64(R, x, w, b, sl)
    part = _run_c64(R, x[:Hs].contiguous(), w, b, sl)
    assert float(full.float().abs().mean()) > 0.05 and bool(torch.isfinite(full.float()).all())
    assert _same_bits(UE.bits(part[:Hs - 1]), UE.bits(full[:Hs - 1]))
    assert not torch.equal(part[Hs - 1], full[Hs - 1])           # the row below differs: the short map pads where the long one has data


def _edge_shape(n_cu, which):
    return (17, 65) if which == "one-round" else _persistent_shape(n_cu, "mod8-7-ragged")


@pytest.mark.parametrize("scale", ["subnormal-out", "subnormal-in", "overflow"])
@pytest.mark.parametrize("which", ["one-round", "persistent"])
def test_c64_range_edges(R, n_cu, which, scale):
    """Power-of-two scalings of the integer data: fp16-subnormal outputs, fp16-subnormal inputs, and outputs beyond 65 504 (+-inf; the rest exact)."""
    H, W = _edge_shape(n_cu, which)
    assert UE.c64_regime(H, W, n_cu)[0] == which
    exp = _check_c64(R, H, W, scale)
    mag = np.abs(exp.astype(np.float64))
    if scale == "overflow":
        assert 0.2 < np.isinf(exp).mean() < 0.9 and np.isfinite(exp).any()
    else:
        assert mag.max() < 2.0 ** -14 and (mag > 0).mean() > 0.9      # subnormal, and not flushed in the expectation


def _poison_points(H, W):
    """Two tile corners of the 32 x 8 grid (x % 32 == 31, y % 8 == 7: the 3 x 3 halo spans four tiles), far apart: (y, x, channel, value)."""
    return [(7, 31, 5, float("nan")), ((H - 9) // 8 * 8 + 7, (W - 33) // 32 * 32 + 31, 58, float("inf"))]


def _check_containment(H, W, clean, dirty, pts):
    window = np.zeros((H, W), dtype=bool)
    for (y, xx, _, _) in pts:
        assert y % 8 == 7 and xx % 32 == 31 and 0 < y < H - 1 and 0 < xx < W - 1
        window[y - 1:y + 2, xx - 1:xx + 2] = True
    assert int(window.sum()) == 9 * len(pts)
    c16, d16 = UE.bits(clean), UE.bits(dirty)
    nonfinite = ~np.isfinite(d16.view(np.float16))
    assert np.array_equal(nonfinite, np.broadcast_to(window[:, :, None], nonfinite.shape)), \
        ("non-finite outside the two windows at", np.argwhere(nonfinite & ~window[:, :, None])[:4], "finite inside at", np.argwhere(~nonfinite & window[:, :, None])[:4])
    assert _same_bits(np.where(window[:, :, None], 0, d16), np.where(window[:, :, None], 0, c16))


@pytest.mark.parametrize("which", ["one-round", "persistent"])
def test_c64_nan_and_inf_stay_in_their_windows(R, n_cu, which):
    """One NaN and one Inf input value: non-finite output on exactly the two 3 x 3 windows, in all 64 channels (0 * NaN and 0 * Inf are NaN, so a zero weight
    does not hide them), every other byte as in the clean run -- including the tiles a persistent workgroup computes AFTER the poisoned one in the same LDS."""
    H, W = _edge_shape(n_cu, which)
    regime, ntiles, per, _ = UE.c64_regime(H, W, n_cu)
    assert regime == which
    pts = _poison_points(H, W)
    if which == "persistent":     # the NaN pixel's own tile is tile 0 = workgroup 0, which goes on to tile `wpx`
        wpx = UE.c64_slots(n_cu) // 8
        assert pts[0][0] // 8 == 0 and pts[0][1] // 32 == 0 and wpx < per and wpx < ntiles
    seed = H * 7 + W
    x, w = UE.int_data(H, W, 64, 64, seed, device="cuda")
    b, sl = _bias(64, seed), _slope(64, seed)
    clean = _run_c64(R, x, w, b, sl)
    assert _same_bits(UE.bits(clean), UE.expect_c64(UE.ref_acc64(x, w), b.numpy(), sl.numpy()).view(np.int16))
    xd = x.clone()
    for (y, xx, c, v) in pts:
        xd[y, xx, c] = v
    _check_containment(H, W, clean, _run_c64(R, xd, w, b, sl), pts)


# ---- vd3d_conv3x3_head_f16 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 65), (2, 64), (3, 63), (5, 129), (32769, 1)])
def test_head_exact(R, H, W):
    """3 -> 64 head on a 64 x 2 tile: one pixel, one past the tile width, exactly one tile, odd rows, three tile columns, a one-pixel-wide column."""
    from visiondepth3d_amd.upscale import head_weight_matrix
    seed = H * 7 + W
    x, w = UE.int_data(H, W, 3, 64, seed, x_range=UE.HEAD_X_RANGE, device="cuda")
    acc = UE.ref_acc64(x, w)
    b = _bias(64, seed)
    for sl in (None, _slope(64, seed)):
        got = R.conv3x3_head(UE.nchw(x), head_weight_matrix(w).cuda(), b.cuda(), sl.cuda() if sl is not None else None)
        torch.cuda.synchronize()
        assert got.dtype == torch.float16 and tuple(got.shape) == (1, 64, H, W) and got.is_contiguous(memory_format=CL)
        exp = UE.expect_head(acc, b.numpy(), None if sl is None else sl.numpy())
        assert _same_bits(UE.bits(UE.hwc(got)), exp.view(np.int16)), (H, W, sl is not None)


# ---- vd3d_conv3x3_dense_f16 ----------------------------------------------------------------------------------------------------------------
EPILOGUES = [dict(slope=0.2), dict(slope=0.2, alpha=0.2, r1=True), dict(slope=0.2, alpha=0.2, r1=True, beta=0.2, r2=True),
             dict(slope=0.3, alpha=0.2, r1=True, beta=0.7, r2=True)]     # the last: slope != alpha, so their ORDER shows (tests/test_upscale_exact_host.py)
DENSE_SIZES = [(1, 1), (8, 32), (9, 33), (17, 65), (135, 240)]
DENSE_SIZES_UP2 = [(1, 1), (5, 7), (9, 33), (17, 65), (67, 119)]         # the INPUT's size, odd: the output is twice that


def _junk(c, h, w, seed, scale=0.7):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(h, w, c, generator=gen) * scale).half().cuda()


def _dense_setup(cin, cout, up2, H, W, scale="unit"):
    """The set-up of test_hip_rrdb.test_dense_kernel_vs_float32_reference with integer data: the input is the first C_in channels of a 192-stride buffer, the
    output the next slice of that buffer (192 -> 64 and up2: the slice [64, 128) of a second one); everything else is a canary.  r1 / r2: random fp16 at
    pixel strides 64 and 192."""
    seed = H * 1000 + W + cin * 7 + cout
    x, w = UE.int_data(H, W, cin, cout, seed, scale=scale, device="cuda")
    xb = _junk(192, H, W, seed + 1)
    xb[..., :cin] = x
    OH, OW = (2 * H, 2 * W) if up2 else (H, W)
    in_place = cin + cout <= 192 and not up2
    yb = xb if in_place else _junk(192, OH, OW, seed + 2)
    off = cin if in_place else 64
    r1, r2 = _junk(64, OH, OW, seed + 3), _junk(192, OH, OW, seed + 4)
    return x, w, xb, yb, off, r1, r2, seed


def _run_dense(R, xb, cin, w, b, cout, yb, off, ep, r1, r2, up2):
    from visiondepth3d_amd.upscale import dense_weight_fragments
    before = yb.clone()
    R.conv3x3_dense(UE.nchw(xb), cin, dense_weight_fragments(w).cuda(), b.cuda(), cout, UE.nchw(yb), off, slope=ep["slope"],
                    r1=UE.nchw(r1) if ep.get("r1") else None, alpha=ep.get("alpha", 1.0), r2=UE.nchw(r2) if ep.get("r2") else None, beta=ep.get("beta", 1.0),
                    up2=up2)
    torch.cuda.synchronize()
    keep = torch.ones(192, dtype=torch.bool, device="cuda")
    keep[off:off + cout] = False
    assert torch.equal(yb[..., keep].view(torch.int16), before[..., keep].view(torch.int16))      # the canary: nothing outside the slice was touched
    return yb[..., off:off + cout].contiguous()


def _expect_dense(acc, b, cout, ep, r1, r2):
    return UE.expect_dense(acc, b.numpy(), ep["slope"], r1[..., :cout].cpu().numpy() if ep.get("r1") else None, ep.get("alpha", 1.0),
                           r2[..., :cout].cpu().numpy() if ep.get("r2") else None, ep.get("beta", 1.0))


@pytest.mark.parametrize("size", range(len(DENSE_SIZES)))
@pytest.mark.parametrize("cin,cout,up2", SHAPES)
def test_dense_exact(R, cin, cout, up2, size):
    """Non-zero integer weights: the K loop (2 to 6 chunks of 32 channels through the LDS ring) and the residual epilogue meet in one bit-exact check, in
    place in the 192-stride buffer."""
    H, W = (DENSE_SIZES_UP2 if up2 else DENSE_SIZES)[size]
    x, w, xb, yb, off, r1, r2, seed = _dense_setup(cin, cout, up2, H, W)
    acc = UE.ref_acc64(x, w, up2=up2)
    b = _bias(cout, seed)
    for ep in EPILOGUES:
        got = _run_dense(R, xb, cin, w, b, cout, yb, off, ep, r1, r2, up2)
        assert _same_bits(UE.bits(got), _expect_dense(acc, b, cout, ep, r1, r2).view(np.int16)), (cin, cout, up2, H, W, ep)


@pytest.mark.parametrize("scale", ["subnormal-out", "subnormal-in", "overflow"])
def test_dense_range_edges_at_192_channels(R, scale):
    H, W = 17, 65
    x, w, xb, yb, off, r1, r2, seed = _dense_setup(192, 64, False, H, W, scale)
    acc = UE.ref_acc64(x, w)
    b = _bias(64, seed, zero=True)
    ep = dict(slope=0.2)
    exp = _expect_dense(acc, b, 64, ep, r1, r2)
    assert _same_bits(UE.bits(_run_dense(R, xb, 192, w, b, 64, yb, off, ep, r1, r2, False)), exp.view(np.int16))
    mag = np.abs(exp.astype(np.float64))
    if scale == "overflow":
        assert 0.2 < np.isinf(exp).mean() < 0.95 and np.isfinite(exp).any()
    else:
        assert mag.max() < 2.0 ** -14 and (mag > 0).mean() > 0.9
    if scale == "overflow":       # a finite residual does not bring an overflowed value back: inf * 0.2 + r1 is inf
        ep = dict(slope=0.2, alpha=0.2, r1=True)
        assert _same_bits(UE.bits(_run_dense(R, xb, 192, w, b, 64, yb, off, ep, r1, r2, False)), _expect_dense(acc, b, 64, ep, r1, r2).view(np.int16))


def test_dense_nan_and_inf_stay_in_their_windows_at_192_channels(R):
    """The NaN sits in the LAST 32-channel chunk of the ring, the Inf in the first."""
    H, W = 17, 65
    x, w, xb, yb, off, r1, r2, seed = _dense_setup(192, 64, False, H, W)
    b = _bias(64, seed)
    ep = dict(slope=0.2, alpha=0.2, r1=True)
    clean = _run_dense(R, xb, 192, w, b, 64, yb, off, ep, r1, r2, False)
    assert _same_bits(UE.bits(clean), _expect_dense(UE.ref_acc64(x, w), b, 64, ep, r1, r2).view(np.int16))
    pts = [(7, 31, 170, float("nan")), (15, 63, 9, float("inf"))]
    for (y, xx, c, v) in pts:
        xb[y, xx, c] = v
    _check_containment(H, W, clean, _run_dense(R, xb, 192, w, b, 64, yb, off, ep, r1, r2, False), pts)


# ---- vd3d_nhwc_f16_to_planar3_f32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 255), (16, 16), (3, 86), (17, 65)])
def test_nhwc_f16_to_planar3_values(R, H, W):
    """One pixel, one short of a 256-thread workgroup, exactly one, one past it (258), several: bit for bit t[:, :3].float(), every fp16 class included."""
    t = _junk(32, H, W, H * 31 + W, 3.0)
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), 2.0 ** -24, -2.0 ** -15, 65504.0, -0.0], dtype=torch.float16, device="cuda")
    idx = torch.arange(min(3 * H * W, 7), device="cuda")
    t.view(-1, 32)[idx // 3, idx % 3] = special[:len(idx)]           # in the three channels that are read, of the first pixels
    got = R.nhwc_f16_to_planar3(UE.nchw(t))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, H, W) and got.is_contiguous()
    exp = UE.nchw(t)[:, :3].float().contiguous()
    assert torch.equal(got.view(torch.int32), exp.view(torch.int32))


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _other_error(R):
    """Leave a KNOWN message of another entry point in vd3d_last_error, so that the message found after a refusal is that refusal's own."""
    from visiondepth3d_amd import _abi
    assert R._L.vd3d_conv3x3_dense_f16(R._ctx, None, 1, 1, 64, 64, None, None, 64, 1.0, 1.0, None, 0, 1.0, None, 0, 0, None, 64, 0) == _abi.E_INVALID
    msg = R._L.vd3d_last_error()
    assert msg.startswith(b"conv3x3_dense_f16")
    return msg


def _refused(R, cases, code, outs):
    """cases: name -> thunk returning the entry point's code.  Each: `code`, a message of its own, and (at the end) every output's bits as before."""
    before = [o.clone() for o in outs]
    for name, call in cases.items():
        other = _other_error(R)
        rc = call()
        assert rc == code, (name, rc)
        msg = R._L.vd3d_last_error()
        assert len(msg) > 0 and msg != other, (name, msg)
    torch.cuda.synchronize()
    for o, o0 in zip(outs, before):
        assert torch.equal(o.view(torch.int16), o0.view(torch.int16))


def test_nhwc_f16_to_planar3_refusals(R):
    """Every buffer has the size the refused call names (and one pixel more behind a shifted pointer)."""
    from visiondepth3d_amd import _abi
    f = R._L.vd3d_nhwc_f16_to_planar3_f32
    H = 32769
    t = torch.zeros((H + 1, 1, 32), dtype=torch.float16, device="cuda")
    out = torch.full((3, H + 1, 1), 7.0, dtype=torch.float32, device="cuda")
    _refused(R, {
        "H = 32 769": lambda: f(R._ctx, _p(t), H, 1, _p(out)),
        "W = 32 769": lambda: f(R._ctx, _p(t), 1, H, _p(out)),
        "H = 0": lambda: f(R._ctx, _p(t), 0, 1, _p(out)),
        "misaligned t": lambda: f(R._ctx, _p(t, 8), 16, 16, _p(out)),
        "misaligned out": lambda: f(R._ctx, _p(t), 16, 16, _p(out, 2)),
    }, _abi.E_UNSUPPORTED, [out.view(torch.int16)])
    _refused(R, {
        "null t": lambda: f(R._ctx, None, 16, 16, _p(out)),
        "null out": lambda: f(R._ctx, _p(t), 16, 16, None),
        "null context": lambda: f(None, _p(t), 16, 16, _p(out)),
    }, _abi.E_INVALID, [out.view(torch.int16)])
    assert f(R._ctx, _p(t), 16, 16, _p(out)) == 0                    # and the same buffers, aligned, are taken
    torch.cuda.synchronize()
    assert float(out.view(-1)[:3 * 256].abs().max()) == 0.0


def test_c64_head_and_tail_refusals(R):
    """Every rule of the three entry points in vd3d_api.hip: VD3D_E_INVALID, a message, and the output keeps its bits (nothing was launched).  The buffers
    have one row more than the size passed, so a shifted pointer stays inside them."""
    from visiondepth3d_amd import _abi
    from visiondepth3d_amd.upscale import conv_weight_fragments, head_weight_matrix
    H, W = 8, 32
    gen = torch.Generator().manual_seed(3)
    x64, y64, x3 = _junk(64, H + 1, W, 1), _junk(64, H + 1, W, 2), _junk(3, H + 1, W, 3)
    wf = torch.cat([conv_weight_fragments(torch.randn(64, 64, 3, 3, generator=gen) * 0.06).view(-1), torch.zeros(8, dtype=torch.float16)]).cuda()
    w27 = torch.cat([head_weight_matrix(torch.randn(64, 3, 3, 3, generator=gen) * 0.2).view(-1), torch.zeros(4)]).cuda()
    bias, slope = torch.zeros(68, device="cuda"), torch.ones(68, device="cuda")
    out4 = torch.full((3, (H + 1) * 4, W * 4), 7.0, dtype=torch.float32, device="cuda")
    ctx = R._ctx

    def c64(c=ctx, x=_p(x64), h=H, w_=W, wp=_p(wf), b=_p(bias), s=_p(slope), y=_p(y64)):
        return R._L.vd3d_conv3x3_c64_f16(c, x, h, w_, wp, b, s, y)
    _refused(R, {
        "null context": lambda: c64(c=None), "null x": lambda: c64(x=None), "null w": lambda: c64(wp=None), "null bias": lambda: c64(b=None),
        "null y": lambda: c64(y=None), "H = 0": lambda: c64(h=0), "W = 0": lambda: c64(w_=0), "H = -1": lambda: c64(h=-1),
        "x == y": lambda: c64(x=_p(y64)),
        "misaligned x": lambda: c64(x=_p(x64, 8)), "misaligned y": lambda: c64(y=_p(y64, 2)), "misaligned w": lambda: c64(wp=_p(wf, 8)),
        "misaligned bias": lambda: c64(b=_p(bias, 4)), "misaligned slope": lambda: c64(s=_p(slope, 8)),
    }, _abi.E_INVALID, [y64, x64])
    assert c64() == 0 and c64(s=None) == 0                           # the same arguments, unbroken, are taken (slope may be null)

    def head(c=ctx, x=_p(x3), h=H, w_=W, wp=_p(w27), b=_p(bias), s=None, y=_p(y64)):
        return R._L.vd3d_conv3x3_head_f16(c, x, h, w_, wp, b, s, y)
    torch.cuda.synchronize()
    _refused(R, {
        "null context": lambda: head(c=None), "null x": lambda: head(x=None), "null w": lambda: head(wp=None), "null bias": lambda: head(b=None),
        "null y": lambda: head(y=None), "H = 0": lambda: head(h=0), "W = 0": lambda: head(w_=0),
        "misaligned y": lambda: head(y=_p(y64, 8)), "misaligned w": lambda: head(wp=_p(w27, 4)),
    }, _abi.E_INVALID, [y64])
    assert head() == 0

    def tail(c=ctx, t=_p(x64), x=_p(x3), h=H, w_=W, r=4, o=_p(out4)):
        return R._L.vd3d_esr_tail_f32(c, t, x, h, w_, r, o)
    _refused(R, {
        "null context": lambda: tail(c=None), "null t": lambda: tail(t=None), "null x": lambda: tail(x=None), "null out": lambda: tail(o=None),
        "H = 0": lambda: tail(h=0), "W = 0": lambda: tail(w_=0), "r = 1": lambda: tail(r=1), "r = 3": lambda: tail(r=3), "r = 8": lambda: tail(r=8),
        "r = 0": lambda: tail(r=0), "misaligned t": lambda: tail(t=_p(x64, 8)),
    }, _abi.E_INVALID, [out4.view(torch.int16)])
    assert tail() == 0 and tail(r=2) == 0
    torch.cuda.synchronize()
