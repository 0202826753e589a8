"""GPU tests (-m gpu) of the three resampling kernels of the depth leg that exist in a general and a fast form, or were rebuilt in place:

  depth hand-off   vd3d_depth_handoff_form: 1 = k_handoff (sixteen taps from memory per output pixel), 2 = k_handoff_sep (one wave walks a band of output rows with
                   the four horizontally interpolated prediction rows in registers) -- bit for bit against the C oracle and against each other
  input prep       vd3d_depth_preprocess_form: 1 = k_depth_prep (32 x 8 tiles), 2 = k_depth_prep_strip (32-column strips of 32-row bands, dword loads) -- torch.equal
  up-sampling      k_upsample_bilinear[_bias]_nhwc_f32 -- torch.equal against the expression of include/vd3d.h stated with element-wise float32 torch operations;
                   k_upsample_bilinear_nhwc (bf16) -- the same expression on the widened bf16 inputs, rounded once with the kernel's f2bf, on bits

Every kernel is a fixed sequence of IEEE float32 operations (the library is built with -ffp-contract=off), so every comparison here is an equality."""
import numpy as np
import pytest

from visiondepth3d_amd import _abi, _lib
from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    r = Renderer(0)
    yield r
    r.close()


def _pred(B, ph, pw, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, ph, pw, generator=g) * 3 + 5).float()


# ------------------------------------------------------------------------------------------ hand-off
HANDOFF_SHAPES = [
    ((74, 132), (216, 384)),
    ((37, 66), (155, 277)),        # odd W: unaligned rows, tail of 1
    ((19, 33), (33, 100)),         # one row past a 32-row band
    ((5, 7), (64, 300)),
    ((3, 3), (9, 1030)),           # just past four 256-column workgroups
    ((2, 2), (7, 5)),
    ((1, 1), (8, 8)),              # flat: zeros
    ((518, 924), (2160, 3840)),    # the headline's, once
]


@pytest.mark.parametrize("src,dst", HANDOFF_SHAPES, ids=lambda s: "%dx%d" % s)
def test_handoff_forms_bit_exact_vs_oracle(R, oracle, src, dst):
    (ph, pw), (H, W) = src, dst
    pred = _pred(1, ph, pw, 11 + ph)
    exp = oracle.depth_handoff(pred[0].numpy(), H, W)
    p = pred.cuda()
    general = R.depth_handoff(p, H, W, form=1).cpu().numpy()
    for form in (0, 2):
        got = R.depth_handoff(p, H, W, form=form).cpu().numpy()
        inv = R.depth_handoff(p, H, W, invert=True, form=form).cpu().numpy()
        assert np.array_equal(got[0], exp), form
        assert np.array_equal(inv[0], 255 - exp), form
        assert np.array_equal(got, general), form
    if (ph, pw) == (1, 1):
        assert not exp.any()


def test_handoff_batch_of_three_ranges_and_a_flat_frame(R, oracle):
    H, W = 155, 277
    ranges = _pred(3, 37, 66, 5)
    ranges[1] = ranges[1] * 1e-3 - 40.0      # a small range far from zero
    ranges[2] = ranges[2] * 1e4              # a large one across zero
    flat = ranges.clone()
    flat[1] = 1.25                           # exactly flat between two others: the interpolated plane spreads over a few ulp of 1.25, at the edge of the flat rule
    for pred in (ranges, flat):
        p = pred.cuda()
        general = R.depth_handoff(p, H, W, form=1).cpu().numpy()
        for form in (0, 2):
            got = R.depth_handoff(p, H, W, form=form).cpu().numpy()
            for b in range(3):
                assert np.array_equal(got[b], oracle.depth_handoff(pred[b].numpy(), H, W)), (form, b)
            assert np.array_equal(got, general), form
    assert got[0].any() and got[2].any()
    zero = torch.zeros(3, 37, 66)
    zero[0], zero[2] = ranges[0], ranges[2]                # a plane of zeros interpolates to exact zeros: flat, the reference writes zeros
    for form in (1, 2):
        got = R.depth_handoff(zero.cuda(), H, W, form=form).cpu().numpy()
        assert not got[1].any() and got[0].any() and got[2].any(), form


def test_handoff_nan_frame_is_zeros_in_both_forms(R):
    pred = _pred(2, 19, 33, 3)
    pred[0, 7, 11] = float("nan")
    p = pred.cuda()
    a = R.depth_handoff(p, 64, 100, form=1).cpu().numpy()
    b = R.depth_handoff(p, 64, 100, form=2).cpu().numpy()
    assert np.array_equal(a, b)
    assert not a[0].any() and a[1].any()


@pytest.mark.parametrize("src,dst", [((80, 120), (40, 60)), ((74, 132), (74, 132))], ids=["down", "same"])
def test_handoff_general_path_keeps_down_scaling_and_identity(R, oracle, src, dst):
    (ph, pw), (H, W) = src, dst
    pred = _pred(1, ph, pw, 9)
    exp = oracle.depth_handoff(pred[0].numpy(), H, W)
    p = pred.cuda()
    assert np.array_equal(R.depth_handoff(p, H, W, form=0).cpu().numpy()[0], exp)
    assert np.array_equal(R.depth_handoff(p, H, W, form=1).cpu().numpy()[0], exp)
    with pytest.raises(_lib.Vd3dError) as e:
        R.depth_handoff(p, H, W, form=2)
    assert e.value.code == _abi.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------ input prep
PREP_SHAPES = [
    (1, (2160, 3840), (518, 924), 0),     # the headline's
    (2, (1080, 1920), (518, 924), 0),     # the 1080p sub-record's
    (3, (97, 131), (28, 42), 1),          # called on frames[1:]: odd row and frame strides, an unaligned base
    (1, (120, 250), (24, 47), 0),         # scales 5.0 / 5.32: 22 - 23 taps, just inside the tap budget; tw no multiple of the strip width
    (1, (64, 64), (64, 64), 0),           # scale 1, support 2
    (1, (56, 84), (14, 21), 0),
    (1, (33, 65), (8, 16), 0),            # narrower than a strip
]


def _frames(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,src,dst,skip", PREP_SHAPES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_prep_strip_form_equals_tile_form(R, B, src, dst, skip, dtype):
    (H, W), (th, tw) = src, dst
    frames = _frames(B, H, W, H + W)[skip:]
    if skip:
        assert frames.data_ptr() % 4 != 0
    tile = R.depth_preprocess(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=dtype, form=1)
    strip = R.depth_preprocess(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=dtype, form=2)
    auto = R.depth_preprocess(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=dtype, form=0)
    assert strip.shape == (B - skip, 3, th, tw) and strip.dtype == dtype and strip.is_contiguous(memory_format=torch.channels_last)
    assert bool(torch.isfinite(tile.float()).all())
    assert torch.equal(strip, tile)
    assert torch.equal(auto, tile)


def test_prep_scale_past_the_tap_budget_fails_in_every_form(R):
    """(56, 84) -> (14, 14): the horizontal scale of 6 needs 26 taps, two more than the tile kernel's budget, so there is no form 1 result to compare with
    (the neighbouring (56, 84) -> (14, 21) is in PREP_SHAPES instead); what holds for this shape is that no form accepts what the tile kernel refuses."""
    frames = _frames(1, 56, 84, 3)
    for dtype in (torch.float32, torch.bfloat16):
        for form in (0, 1, 2):
            with pytest.raises(_lib.Vd3dError) as e:
                R.depth_preprocess(frames, 14, 14, IMAGENET_MEAN, IMAGENET_STD, dtype=dtype, form=form)
            assert e.value.code == _abi.E_UNSUPPORTED and "tap budget" in str(e.value), (dtype, form)


def test_prep_up_scaling_stays_on_the_tile_form_and_the_tap_budget_holds(R):
    frames = _frames(2, 40, 60, 1)
    tile = R.depth_preprocess(frames, 70, 126, IMAGENET_MEAN, IMAGENET_STD, form=1)
    assert torch.equal(R.depth_preprocess(frames, 70, 126, IMAGENET_MEAN, IMAGENET_STD, form=0), tile)
    with pytest.raises(_lib.Vd3dError) as e:
        R.depth_preprocess(frames, 70, 126, IMAGENET_MEAN, IMAGENET_STD, form=2)
    assert e.value.code == _abi.E_UNSUPPORTED
    frames = _frames(1, 120, 250, 2)
    for form in (0, 1, 2):                                 # scale 6: 26 taps, past the budget of 24 whatever the form
        with pytest.raises(_lib.Vd3dError) as e:
            R.depth_preprocess(frames, 20, 40, IMAGENET_MEAN, IMAGENET_STD, form=form)
        assert e.value.code == _abi.E_UNSUPPORTED and "tap budget" in str(e.value)


# ------------------------------------------------------------------------------------------ up-sampling
UPSAMPLE_SHAPES = [
    (2, 128, (19, 33), (37, 66)),
    (1, 128, (37, 66), (74, 132)),
    (3, 12, (5, 7), (11, 14)),            # c4 = 3: no power of two
    (1, 8, (1, 5), (4, 9)),               # ih = 1
    (1, 4, (3, 3), (2, 2)),
    (1, 128, (5, 3), (10, 6)),
]


def _upsample_ref(x_nhwc, oh, ow, bias):
    """(ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11)) [+ bias], every operator its own float32 torch kernel (nothing to contract)."""
    B, ih, iw, C = x_nhwc.shape
    dev = x_nhwc.device
    sh = float(np.float32(ih - 1) / np.float32(oh - 1))
    sw = float(np.float32(iw - 1) / np.float32(ow - 1))

    def taps(n_out, n_in, s):
        f = torch.arange(n_out, device=dev, dtype=torch.float32) * s
        i0 = f.to(torch.int64)
        i1 = i0 + (i0 < n_in - 1).to(torch.int64)
        l1 = f - i0.to(torch.float32)
        return i0, i1, 1.0 - l1, l1

    y0, y1, ly0, ly1 = taps(oh, ih, sh)
    x0, x1, lx0, lx1 = taps(ow, iw, sw)
    ly0, ly1 = ly0.view(1, oh, 1, 1), ly1.view(1, oh, 1, 1)
    lx0, lx1 = lx0.view(1, 1, ow, 1), lx1.view(1, 1, ow, 1)
    r0, r1 = x_nhwc[:, y0], x_nhwc[:, y1]
    p00, p01, p10, p11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    out = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11)
    return out + bias.view(1, 1, 1, C) if bias is not None else out


@pytest.mark.parametrize("B,C,src,dst", UPSAMPLE_SHAPES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_upsample_f32_bit_exact(R, B, C, src, dst):
    (ih, iw), (oh, ow) = src, dst
    g = torch.Generator(device="cuda").manual_seed(C + ih)
    buf = torch.randn(B + 1, ih, iw, C, device="cuda", generator=g)
    buf[B] = float("nan")                                  # behind the last image: a tap that leaves the map (an unclamped x1 or y1, weight 0) poisons the result
    x = buf[:B]
    bias = torch.randn(C, device="cuda", generator=g)
    x_cl = x.permute(0, 3, 1, 2)                           # channels_last [B,C,h,w] view of the NHWC storage
    got = R.upsample_bilinear(x_cl, (oh, ow))
    assert torch.equal(got.permute(0, 2, 3, 1), _upsample_ref(x, oh, ow, None))
    got = R.upsample_bilinear_bias(x_cl, (oh, ow), bias)
    assert torch.equal(got.permute(0, 2, 3, 1), _upsample_ref(x, oh, ow, bias))


def _f2bf_bits(f):
    """The kernel's f2bf on a float32 tensor -> bf16 bits as int16: (b + 0x7fff + ((b >> 16) & 1)) >> 16 in 32-bit arithmetic that wraps, as the device's does."""
    b = f.contiguous().view(torch.int32)
    return (((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff).to(torch.int16)


@pytest.mark.parametrize("B,C,src,dst", UPSAMPLE_SHAPES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_upsample_bf16_bit_exact(R, B, C, src, dst):
    """One thread = 8 channels: C doubled where it is no multiple of 8 (12 -> 24 keeps a c8 = 3 that is no power of two).  float32 blend of the widened inputs
    in the float32 kernel's association, one rounding to bf16."""
    (ih, iw), (oh, ow) = src, dst
    C = C if C % 8 == 0 else 2 * C
    assert C % 8 == 0
    g = torch.Generator(device="cuda").manual_seed(C + ih)
    buf = (torch.randn(B + 1, ih, iw, C, device="cuda", generator=g) * 3).to(torch.bfloat16)
    buf[B] = float("nan")                                  # behind the last image: an unclamped x1 or y1 tap of weight 0 poisons the result
    x = buf[:B]
    got = R.upsample_bilinear(x.permute(0, 3, 1, 2), (oh, ow))
    assert got.dtype == torch.bfloat16 and got.shape == (B, C, oh, ow) and got.is_contiguous(memory_format=torch.channels_last)
    want = _f2bf_bits(_upsample_ref(x.float(), oh, ow, None))
    assert not bool(torch.isnan(got.float()).any())
    assert torch.equal(got.permute(0, 2, 3, 1).contiguous().view(torch.int16), want)
