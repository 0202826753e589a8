"""vd3d_neck_poly_conv_f32 (csrc/vd3d_conv_poly.hip): the neck's ConvTranspose2d (kernel == stride == f, bias) and the bias-free 3 x 3 convolution behind it as one
exact-float32 MFMA launch on the coarse map, against the float64 module chain and beside the library chain it replaces.

The kernel has no two-dimensional tile: a wave takes 32 consecutive pixels of the flat [B h w] coarse pixel list, a workgroup 128.  Maps: 1 x 1, one row, one column,
a frame that is exactly one workgroup (8 x 16), one pixel past it in either direction (3 x 43, 43 x 3: waves and workgroups straddle rows and frames), a list with a
partial last wave (5 x 7 x 3 = 105) and a few workgroups (11 x 37 x 3 = 1221 = 9.54 of them).  Bars against float64 are RELATIVE to the library chain's own error
(max <= 2 x, RMS <= 1.25 x: the bars of tests/test_hip_dpt_head_f32.py); the integer cases are bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BASE = ((96, 128, 4), (192, 128, 2))
SMALL = ((48, 64, 4), (96, 64, 2))
SHAPE_IDS = lambda s: "c%d-%d-f%d" % s
MAPS = ((1, 1), (1, 7), (5, 1), (8, 16), (3, 43), (43, 3), (5, 7), (11, 37))


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _chain64(x, wt, bt, w3, f):
    return F.conv2d(F.conv_transpose2d(x.double(), wt.double(), bt.double(), stride=f), w3.double(), None, padding=1)


def _packed(R, wt, bt, w3, f):
    from visiondepth3d_amd.depth import neck_poly_compose
    p = R.neck_poly_pack(*neck_poly_compose(wt, bt, w3, f), f)
    assert p is not None
    return p


@pytest.fixture(scope="module")
def int_weights(R):
    """Per shape: integer weights in {-1, 0, 1}, biases in {-2 .. 2}: with |x| <= 2 the absolute values of everything that enters one output element sum to at most
    9 C (2 C_in + 2) <= 9 x 192 x 386 = 667 008 < 2^24, so every partial sum of every summation order is an exactly represented integer, and so is every composed
    weight (at most 4 C = 768).  Packed once per shape."""
    out = {}
    for Cin, Cout, f in BASE + SMALL:
        g = torch.Generator(device="cuda").manual_seed(Cin + Cout + f)
        wt = torch.randint(-1, 2, (Cin, Cin, f, f), device="cuda", generator=g).float()
        bt = torch.randint(-2, 3, (Cin,), device="cuda", generator=g).float()
        w3 = torch.randint(-1, 2, (Cout, Cin, 3, 3), device="cuda", generator=g).float()
        out[Cin, Cout, f] = (wt, bt, w3, _packed(R, wt, bt, w3, f))
    return out


@pytest.mark.parametrize("hw", MAPS, ids=["%dx%d" % m for m in MAPS])
@pytest.mark.parametrize("shape", BASE + SMALL, ids=SHAPE_IDS)
def test_integer_operands_are_bit_exact(R, int_weights, shape, hw):
    """Batch 3, a frame of NaNs behind the last input frame and a sentinel frame behind the output: equality with the float64 module chain pins every index -- phase,
    offset, border (zero padding of the FINE map: neither product nor bias from outside), channel order of the weight image, frame seams -- and nothing is read or
    written past the batch."""
    from visiondepth3d_amd.render_3d import _ptr
    Cin, Cout, f = shape
    h, w = hw
    wt, bt, w3, packed = int_weights[shape]
    g = torch.Generator(device="cuda").manual_seed(7 * h + w)
    xs = torch.full((4, h, w, Cin), float("nan"), device="cuda")
    xs[:3] = torch.randint(-2, 3, (3, h, w, Cin), device="cuda", generator=g).float()
    x = xs[:3].permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=CL)
    ref = _chain64(x, wt, bt, w3, f)
    assert float(ref.abs().max()) < 2 ** 24
    outs = torch.full((4, f * h, f * w, Cout), -7.0, device="cuda")
    torch.cuda.synchronize()
    img, bc = packed[0], packed[1]
    R._enter(x, img, bc, outs)
    assert R._L.vd3d_neck_poly_conv_f32(R._ctx, _ptr(xs), 3, h, w, Cin, _ptr(img), _ptr(bc), Cout, f, _ptr(outs)) == 0, R._L.vd3d_last_error()
    torch.cuda.synchronize()
    got = outs[:3].permute(0, 3, 1, 2)
    assert torch.equal(got.double(), ref), float((got.double() - ref).abs().max())
    assert bool((outs[3] == -7.0).all())
    via = R.neck_poly_conv(x, packed)
    assert via.shape == (3, Cout, f * h, f * w) and via.is_contiguous(memory_format=CL) and torch.equal(via, got)


@pytest.fixture(scope="module")
def random_case():
    def make(shape, B, h, w, seed):
        Cin, Cout, f = shape
        g = torch.Generator(device="cuda").manual_seed(seed)
        x = torch.randn(B, Cin, h, w, device="cuda", generator=g).contiguous(memory_format=CL)
        wt = torch.randn(Cin, Cin, f, f, device="cuda", generator=g) / Cin ** 0.5
        bt = torch.randn(Cin, device="cuda", generator=g)
        w3 = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / (3.0 * Cin ** 0.5)
        return x, wt, bt, w3
    return make


@pytest.mark.parametrize("shape", BASE + SMALL, ids=SHAPE_IDS)
def test_error_against_float64_is_the_library_chains(R, random_case, shape):
    """Reference: the module chain in torch float64.  The composed launch and the library chain (float32 conv_transpose2d + conv2d) are both measured against it:
    max error <= 2 x and RMS error <= 1.25 x the library chain's."""
    Cin, Cout, f = shape
    x, wt, bt, w3 = random_case(shape, 2, 19, 33, 23)
    ref = _chain64(x, wt, bt, w3, f)
    lib = F.conv2d(F.conv_transpose2d(x, wt, bt, stride=f), w3, None, padding=1)
    got = R.neck_poly_conv(x, _packed(R, wt, bt, w3, f))
    e_got, e_lib = (got.double() - ref).abs(), (lib.double() - ref).abs()
    mx, mx_lib = float(e_got.max()), float(e_lib.max())
    rms, rms_lib = float(e_got.pow(2).mean().sqrt()), float(e_lib.pow(2).mean().sqrt())
    print("NECK_POLY_F64", SHAPE_IDS(shape), dict(max=mx, max_lib=mx_lib, rms=rms, rms_lib=rms_lib, max_ratio=mx / mx_lib, rms_ratio=rms / rms_lib))
    assert mx <= 2.0 * mx_lib and rms <= 1.25 * rms_lib, (mx, mx_lib, rms, rms_lib)


@pytest.mark.parametrize("shape", BASE, ids=SHAPE_IDS)
def test_same_bits_from_call_to_call_and_from_batch_to_batch(R, random_case, shape):
    """No split-K, no atomics, and the flat pixel list puts frame 0's pixels into other lanes once a batch follows it: two calls give equal bits, and frame 0 alone
    equals frame 0 of a batch of 3 (11 x 37: 407 pixels per frame, so the batch's wave and workgroup seams fall elsewhere)."""
    Cin, Cout, f = shape
    x, wt, bt, w3 = random_case(shape, 3, 11, 37, 5)
    packed = _packed(R, wt, bt, w3, f)
    a, b = R.neck_poly_conv(x, packed), R.neck_poly_conv(x, packed)
    one = R.neck_poly_conv(x[:1].contiguous(memory_format=CL), packed)
    two = R.neck_poly_conv(x[1:].contiguous(memory_format=CL), packed)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(one[0], a[0]) and torch.equal(two, a[1:])


def test_packed_image_is_the_restated_layout(R):
    from test_neck_poly_host import BUILT, pack_restated
    for Cin, Cout, f in BUILT:
        Wc = torch.randn((f + 2) ** 2, Cout, Cin, device="cuda")
        bc = torch.randn((f + 2) ** 2, Cout, device="cuda")
        img, b, ci, co, ff = R.neck_poly_pack(Wc, bc, f)
        assert (ci, co, ff) == (Cin, Cout, f) and torch.equal(b, bc)
        assert torch.equal(img.view(torch.float32), pack_restated(Wc))


def test_refusals_launch_nothing(R):
    """A shape that is not built, a misaligned pointer, a map that is not channels_last, weights of another shape: VD3D_E_UNSUPPORTED, None or ValueError, and the
    output buffer keeps its bytes."""
    from visiondepth3d_amd import _abi
    from visiondepth3d_amd.render_3d import _ptr
    L, ctx = R._L, R._ctx
    assert R.neck_poly_pack(torch.zeros(36, 128, 64), torch.zeros(36, 128), 4) is None         # 64 -> 128 is not built
    assert R.neck_poly_pack(torch.zeros(25, 128, 96), torch.zeros(25, 128), 3) is None         # factor 3
    assert R.neck_poly_pack(torch.zeros(36, 256, 256), torch.zeros(36, 256), 4) is None        # DA-V2-Large keeps the library
    with pytest.raises(ValueError):
        R.neck_poly_pack(torch.zeros(16, 128, 96), torch.zeros(16, 128), 4)                     # 16 blocks belong to factor 2
    with pytest.raises(ValueError):
        R.neck_poly_pack(torch.zeros(36, 128, 96), torch.zeros(36, 64), 4)
    packed = R.neck_poly_pack(torch.randn(36, 128, 96), torch.randn(36, 128), 4)
    img, bc = packed[0], packed[1]
    x = torch.randn(1, 6, 7, 96, device="cuda")                    # NHWC storage, room for the misaligned view
    out = torch.full((1, 20, 28, 128), -7.0, device="cuda")
    torch.cuda.synchronize()

    def call(xp, Cin, Cout, f, B=1, h=5, w=7, o=out, b=bc):
        return L.vd3d_neck_poly_conv_f32(ctx, xp, B, h, w, Cin, _ptr(img), _ptr(b) if b is not None else None, Cout, f, _ptr(o))
    assert call(_ptr(x), 64, 128, 4) == _abi.E_UNSUPPORTED and b"not built" in L.vd3d_last_error()
    assert call(_ptr(x), 96, 128, 2) == _abi.E_UNSUPPORTED
    assert call(_ptr(x), 96, 32, 4) == _abi.E_UNSUPPORTED
    assert call(_ptr(x), 96, 128, 4, h=0) == _abi.E_UNSUPPORTED
    assert call(_ptr(x), 96, 128, 4, B=0) == _abi.E_UNSUPPORTED
    assert call(C.c_void_p(x.data_ptr() + 4), 96, 128, 4) == _abi.E_UNSUPPORTED and b"aligned" in L.vd3d_last_error()
    assert L.vd3d_neck_poly_conv_f32(ctx, _ptr(x), 1, 5, 7, 96, _ptr(img), C.c_void_p(bc.data_ptr() + 4), 128, 4, _ptr(out)) == _abi.E_UNSUPPORTED
    assert call(_ptr(x), 96, 128, 4, b=None) == _abi.E_INVALID
    assert L.vd3d_neck_poly_pack_f32(ctx, _ptr(x), 64, 128, 4, _ptr(img)) == _abi.E_UNSUPPORTED
    assert L.vd3d_neck_poly_pack_f32(ctx, C.c_void_p(x.data_ptr() + 4), 96, 128, 4, _ptr(img)) == _abi.E_UNSUPPORTED and b"aligned" in L.vd3d_last_error()
    with pytest.raises(ValueError):
        R.neck_poly_conv(torch.randn(1, 96, 5, 7, device="cuda"), packed)                       # NCHW-contiguous
    with pytest.raises(ValueError):
        R.neck_poly_conv(torch.randn(1, 10, 7, 96, device="cuda").permute(0, 3, 1, 2)[:, :, ::2], packed)   # rows with gaps
    with pytest.raises(ValueError):
        R.neck_poly_conv(torch.randn(1, 192, 5, 7, device="cuda").contiguous(memory_format=CL), packed)     # weights of another shape
    with pytest.raises(ValueError):
        R.neck_poly_conv(torch.randn(1, 96, 5, 7, device="cuda").contiguous(memory_format=CL), None)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_pipe_prediction_is_the_library_routes(R, monkeypatch):
    """DepthPipe("depth-anything-v2-small"), two 270 x 480 frames: VD3D_NECK_POLY=0 and =1 give the same raw prediction to 1e-4 of its range and the same uint8
    hand-off plane on >= 99.5 % of the bytes, never more than one level apart (tests/test_hip_depth_e2e.py's bars); both routes are named in conv_routes, the composed
    launch runs twice per forward with the switch on and never with it off, and the counted FLOPs are the module graph's either way."""
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import DepthPipe
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, 270, 480)[0] for i in range(2)])).cuda()
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R)
    calls = [0]
    real = R.neck_poly_conv
    monkeypatch.setattr(R, "neck_poly_conv", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real(*a, **k))[1])
    names = ["neck.reassemble_stage.layers.0.resize", "neck.convs.0", "neck.reassemble_stage.layers.1.resize", "neck.convs.1"]
    monkeypatch.setenv("VD3D_NECK_POLY", "0")
    p0 = pipe.infer_bgr_u8(frames, raw=True).clone()
    assert calls[0] == 0 and all(pipe.conv_routes[n] == ("library", "VD3D_NECK_POLY=0") for n in names), pipe.conv_routes
    monkeypatch.setenv("VD3D_NECK_POLY", "1")
    p1 = pipe.infer_bgr_u8(frames, raw=True).clone()
    assert calls[0] == 2 and all(pipe.conv_routes[n][0] == "f32-poly" for n in names), pipe.conv_routes
    assert "48 -> 64 channels, factor 4" in pipe.conv_routes[names[0]][1] and "96 -> 64 channels, factor 2" in pipe.conv_routes[names[3]][1]
    pipe.infer_bgr_u8(frames, raw=True)
    assert calls[0] == 4                                   # twice per forward, from the blocks cached per parameter version (the rest of the forward holds library
                                                           # launches that do not repeat their own bits, so whole predictions are compared by the bars below only)
    assert p0.shape == p1.shape
    rng = float(p0.max() - p0.min())
    err = float((p1 - p0).abs().max()) / rng
    u0, u1 = R.depth_handoff(p0, 270, 480), R.depth_handoff(p1, 270, 480)
    d = (u0.to(torch.int16) - u1.to(torch.int16)).abs()
    exact, mx = float((d == 0).float().mean()), int(d.max())
    print("NECK_POLY_PIPE", dict(pred_err_of_range=err, u8_exact=exact, u8_max=mx))
    assert err < 1e-4, err
    assert exact >= 0.995 and mx <= 1, (exact, mx)
    fl1 = pipe.flops_per_frame(270, 480)                   # the record's FLOP count stays the module graph's: the bypassed transposed convolution is counted
    monkeypatch.setenv("VD3D_NECK_POLY", "0")
    assert pipe.flops_per_frame(270, 480) == fl1
