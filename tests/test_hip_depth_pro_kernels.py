"""GPU tests (-m gpu) of the two kernels of csrc/vd3d_depthpro.hip alone, through the C entry points: the image processor's front end and the post-process, at
the smallest shapes at which they can still go wrong (odd frame sizes, a one-pixel frame, an axis that is the identity, odd output sizes, an unaligned output,
more than one workgroup), each against the processor restated in torch on the CPU.  Where ATen's CPU kernel may round differently (contracted multiply-adds) the
bound is derived, never picked: depth_pro_cases.bilinear_bound states the derivation."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F   # noqa: E402

import depth_pro_cases as cases   # noqa: E402

U = cases.U
HALF = (0.5, 0.5, 0.5)


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


# ---------------------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("H,W,S", [(270, 481, 256), (270, 481, 1536), (64, 1536, 1536), (1, 1, 4), (300, 256, 256)])
def test_preprocess_is_the_processor(R, H, W, S):
    """Against the processor's statement in torch on the CPU (rescale + normalise, then F.interpolate bilinear without antialias): an odd-sized frame, a frame
    already 1536 wide (that axis is the identity), a one-pixel frame and a down-scale.  The normalised values lie in [-1, 1]: A = 1, D = 2 in bilinear_bound."""
    from visiondepth3d_amd import depth_pro
    B = 2 if S < 1536 else 1
    fr = cases.frames(B, H, W, 100 + H + W)
    got = R.depthpro_preprocess(fr.cuda(), S, HALF, HALF).cpu()
    ref = cases.processor_in_torch(fr, S)
    assert got.shape == ref.shape == (B, 3, S, S) and got.is_contiguous()
    assert torch.equal(depth_pro.preprocess_statement(fr, (S, S), HALF, HALF), ref)            # the package's statement is the processor's
    lim = cases.bilinear_bound(1.0, 2.0, H, W)
    d = float((got - ref).abs().max())
    print("DEPTH_PRO_PREPROCESS", dict(H=H, W=W, S=S, max_diff=d, bound=lim, exact=float((got == ref).float().mean())))
    assert d <= lim
    tab = depth_pro.normalize_table(HALF, HALF)
    assert float(tab.min()) == -1.0 and float(tab.max()) == 1.0 and float(got.min()) >= -1.0 and float(got.max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- post-process
def _pred(B, S, seed):
    """Depths that straddle both clamp limits: a smooth field between 0.05 and 40, with exact 1e-4 and 1e4, values beyond both, 0 and a negative planted."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:S, 0:S]
    p = (0.05 + 40.0 * ((y * 3 + x * 5) % (2 * S)) / (2 * S) + rng.uniform(0, 0.5, (B, S, S))).astype(np.float32)
    p[:, 2, 3], p[:, 2, 4], p[:, 5, 1], p[:, 5, 2], p[:, 7, 7], p[:, 9, 2] = 1e-4, 1e4, 3e-5, 7e4, 0.0, -2.5
    return torch.from_numpy(p)


def _local(src, oH, oW):
    """Per output pixel: max |v| and the range of the source over the 5 x 5 neighbourhood of its first tap (a superset of the taps and of the cells beside them)."""
    from visiondepth3d_amd.depth_pro import aten_linear_taps
    S = src.shape[-1]
    y0, x0 = aten_linear_taps(S, oH)[0], aten_linear_taps(S, oW)[0]
    v = src[:, None]
    mx, mn = F.max_pool2d(v, 5, 1, 2), -F.max_pool2d(-v, 5, 1, 2)
    A, D = torch.maximum(mx.abs(), mn.abs())[:, 0], (mx - mn)[:, 0]
    return A[:, y0][:, :, x0], D[:, y0][:, :, x0]


@pytest.mark.parametrize("fov", [False, True], ids=["no-fov", "fov"])
@pytest.mark.parametrize("S,oH,oW", [(24, 24, 24), (24, 31, 45), (64, 135, 241), (64, 33, 17)])
def test_post_process_is_the_processors(R, fov, S, oH, oW):
    """Against post_process_depth_estimation restated in torch on the CPU, B = 2, one field of view narrow and one wide.  Bound, per element:
      the scaled depth v = (d * width) / focal: d * width is the same float in both; tan differs by <= 3 U relative (the kernel's is evaluated in float64 and
      narrowed, <= U up to a double rounding far below it; ATen's float32 tan is within 1 ulp = 2 U), focal = fl(0.5 width / tan) adds one rounding each (2 U), the division by focal one each (2 U):
      <= 7 U, taken as 8 U relative for the second-order terms (0 without a field of view);
      the resize: depth_pro_cases.bilinear_bound with the local A and D and that relative difference (no resize for oH = oW = S: the values themselves);
      clamp is 1-Lipschitz; r = fl(1 / c): |1 / c1 - 1 / c2| <= delta / (c1 c2), c >= 1e-4, plus one rounding each, 2 U r."""
    B = 2
    pred = _pred(B, S, S + oH)
    fv = torch.tensor([27.5, 91.0]) if fov else None
    got = R.depthpro_post(pred.cuda(), fv.cuda() if fov else None, oH, oW).cpu()
    ref = torch.stack(cases.post_process_in_torch(pred, fv, [(oH, oW)] * B))
    assert got.shape == ref.shape == (B, oH, oW) and bool(torch.isfinite(got).all())
    assert float(got.min()) >= float(np.float32(1.0) / np.float32(1e4)) and float(got.max()) <= float(np.float32(1.0) / np.float32(1e-4))   # 1 / the clamp limits, in float32
    scale = torch.ones(B) if not fov else oW / (0.5 * oW / torch.tan(0.5 * torch.deg2rad(fv)))
    scaled = pred * scale.view(B, 1, 1)
    rel = 8 * U if fov else 0.0
    if (oH, oW) == (S, S):
        delta = rel * scaled.abs()
        c = torch.clamp(scaled, 1e-4, 1e4)
    else:
        A, D = _local(scaled, oH, oW)
        delta = cases.bilinear_bound(A, D, S, S, rel)
        c = torch.clamp(F.interpolate(scaled[:, None], size=(oH, oW), mode="bilinear")[:, 0], 1e-4, 1e4)
    lim = delta / (c * torch.clamp(c - delta, min=1e-4)) + 2 * U * ref
    d = (got - ref).abs()
    print("DEPTH_PRO_POST", dict(fov=fov, S=S, out=(oH, oW), max_diff=float(d.max()), max_ratio_to_bound=float((d / lim).max()), exact=float((got == ref).float().mean())))
    assert bool((d <= lim).all())
    if not fov and (oH, oW) == (S, S):
        assert torch.equal(got, ref)                                       # clamp and one correctly rounded division: the same bits


@pytest.mark.parametrize("oH,oW", [(24, 24), (31, 45)])
def test_post_process_keeps_nan_and_makes_nothing_else_non_finite(R, oH, oW):
    pred = _pred(1, 24, 5)
    pred[0, 12, 12] = float("nan")
    pred[0, 0, 23] = float("inf")
    got = R.depthpro_post(pred.cuda(), torch.tensor([60.0]).cuda(), oH, oW).cpu()
    assert bool(torch.isfinite(got[~torch.isnan(got)]).all())
    if (oH, oW) == (24, 24):   # no interpolation: exactly the NaN stays NaN and the infinity clamps to 1e4 -> 1e-4.  (ATen's identity resize still multiplies a
        # second tap by zero, which turns the infinity into a NaN: the raw form's documented deviation, depth_pro.post_statement(resize=False).)
        from visiondepth3d_amd.depth_pro import post_statement
        assert int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[0, 12, 12])) and float(got[0, 0, 23]) == float(1.0 / torch.tensor(1e4))
        assert torch.equal(torch.isnan(got), torch.isnan(post_statement(pred, torch.tensor([60.0]), 24, 24, resize=False)))
    else:                      # the NaN and the infinity spread to every pixel that taps them, zero weights included, exactly as in ATen
        ref = torch.stack(cases.post_process_in_torch(pred, torch.tensor([60.0]), [(oH, oW)]))
        assert torch.equal(torch.isnan(got), torch.isnan(ref)) and int(torch.isnan(got).sum()) > 1


def test_post_process_takes_an_unaligned_output(R):
    """The 4-byte store form: an output that starts 4 bytes past a 16-byte boundary gives the same bits."""
    pred, fv = _pred(2, 24, 6).cuda(), torch.tensor([40.0, 70.0]).cuda()
    a = R.depthpro_post(pred, fv, 31, 45)
    buf = torch.full((2 * 31 * 45 + 1,), float("nan"), device="cuda")
    b = R.depthpro_post(pred, fv, 31, 45, out=buf[1:].view(2, 31, 45))
    assert torch.equal(a, b) and bool(torch.isnan(buf[0]))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(R):
    """Misaligned pointers, a side that is no multiple of 4 and empty shapes: VD3D_E_UNSUPPORTED with the message; the output keeps its NaNs."""
    from visiondepth3d_amd import _abi
    L, ctx = R._L, R._ctx

    def ptr(t, off=0):
        return C.c_void_p(t.data_ptr() + off)

    def refused(rc, word):
        assert rc == _abi.E_UNSUPPORTED and word in L.vd3d_last_error().decode(), (rc, L.vd3d_last_error())
    out = torch.full((3 * 16 * 16 + 4,), float("nan"), device="cuda")
    fr = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda")
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    refused(L.vd3d_depthpro_preprocess_u8(ctx, ptr(fr), 1, 8, 8, 16, m, m, ptr(out, 4)), "16-byte aligned")
    refused(L.vd3d_depthpro_preprocess_u8(ctx, ptr(fr), 1, 8, 8, 18, m, m, ptr(out)), "multiple of 4")
    refused(L.vd3d_depthpro_preprocess_u8(ctx, ptr(fr), 1, 0, 8, 16, m, m, ptr(out)), "at least one")
    pred = torch.zeros(1, 8, 8, device="cuda")
    refused(L.vd3d_depthpro_post_f32(ctx, ptr(pred), None, 1, 8, 0, 8, ptr(out)), "empty shape")
    refused(L.vd3d_depthpro_post_f32(ctx, ptr(pred), None, 1, 8, 8, 8, ptr(out, 2)), "4-byte aligned")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
