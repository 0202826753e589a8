"""CPU tests (no GPU) of the restatement that tests/test_hip_depthprep_bits.py holds vd3d_depth_preprocess (csrc/vd3d_depthprep.hip, both kernels, float32 and bf16)
to, bit for bit; of the cases both files share; and of the launcher's host arithmetic against the restatement's tap windows.

The restatement (prep_statement) is NumPy float32, one NumPy operation per float32 operation of the kernel and in its order (the library is built with
-ffp-contract=off; float32 division is correctly rounded): scale = (float)in / (float)out; support = 2 scale, invscale = 1 / scale for scale >= 1, else 2 and 1;
center = scale * ((float)i + 0.5f); xmin = max((int)((center - support) + 0.5f), 0), xend = min((int)((center + support) + 0.5f), in), (int) truncating; the
taps dp_cubic((((float)(j + xmin) - center) + 0.5f) * invscale), a = -0.5, in the kernel's two Horner forms; total summed over ascending j from +0, every weight
divided by it when it is not 0; per input row the horizontal sums s += (float)byte * w_j over ascending j from +0, BGR -> RGB; the vertical sums of those in the
same way; ((s / 255.0f) - mean[c]) / std[c]; bf16: round to nearest even on the bits.  It has no clamp: a window that leaves the image is an IndexError.

Against the same operator in float64 (reference), per element.  The reference takes the float32 value of scale, widened (a float64 in / out moves every centre
by ~6e-8 x the index, which dominates the arithmetic), and sums over ALL input pixels with the cubic's own support: a tap is inside [xmin, xend) exactly when
-2 < x <= 2, and dp_cubic(2) = 0, so the window needs no restating.  With u = 2^-24, one axis, output i, x_k the exact argument of input pixel k,
c_k = cubic(x_k), T = sum c_k, W_k = c_k / T, d_k = k - center, sums over the n taps in ascending order:
  the centre    center = scale * (i + 0.5f) rounds once: |dcenter| <= u |center|.  It grows with the index and is the SAME for every tap of the window, so it is
                carried with its sign, through G_k = dW_k / dcenter = (c'_k - W_k sum c'_k) / T, c'_k = -invscale cubic'(x_k) -- not tap by tap in absolute value
  the argument  but for the centre: the subtraction, the + 0.5f, invscale and the product round once each:   e_k = invscale u (|d_k| + |d_k + 0.5|) + 2 u |x_k|
  the polynomial  running error of the Horner form, every operation rounding its own result once (P_k, cubic_rounding below); with the argument's error
                |dv_k| <= |cubic'(x_k)| e_k + 2.5 (e_k + invscale u |center|)^2 + P_k      (|cubic''| <= 5; the square term also covers a tap that enters or
                leaves the window at |x| = 2, where the cubic has a double root)
  the total     every partial sum rounds once:   |dT| <= sum |dv_k| + u sum_j |c_0 + .. + c_j|
  the division  |dW_k| <= |dv_k| / |T| + |W_k| |dT| / |T| + u |W_k|
  a filter sum  sum_k p_k w_k over the n taps: every product and every partial sum round once,
                |d sum| <= sum |p_k| |dW_k| + u (sum |p_k W_k| + sum_j |p_0 W_0 + .. + p_j W_j|) =: sum |p_k| |dW_k| + R(p, W)     (~ n u sum |p_k W_k| at the most)
so with p the bytes, h_r the exact horizontal sums of input row r, s the exact 2-D sum, m = mean_c and sd = std_c (the float32 values, widened):
  Eh_r = sum_k p_rk |dWx_k| + R(p_r, Wx)
  Es   = sum_r |Wy_r| Eh_r + sum_r |h_r| |dWy_r| + R(h, Wy) + u |center_x| |sum_r Wy_r sum_k p_rk Gx_k| + u |center_y| |sum_r h_r Gy_r|
  |err| <= (Es / 255 + u |s| / 255 + u |s / 255 - m|) / sd + u |out|          [+ 2^-8 (|out| + that) for the bf16 result's one rounding]
(first order but for the square term; the float64 reference's own rounding, 2^-40 of the same scales, is added).  The weights have negative lobes (sum |W| is
1.1 - 1.3), so the bytes enter through sum p |W| and the partial sums, the tap counts n_x and n_y through the number of partial sums, 1 / std_c multiplies all
of it.  Nothing in it is fitted.

Measured on CASES (float32, ImageNet and DPT normalisation; worst ratio of |err| to the bound over the elements of a case), test_statement_is_within_the_bound:
  the restatement              0.59 x the bound at the worst (hd1080_16); 0.33 - 0.59 x on headline16, hd1080_16, up, tile_edge, where the centre's rounding leads
                               (max |err| 1.0e-5 - 3.4e-5); 0.03 - 0.19 x on the small geometries (max |err| 2.5e-7 - 5.4e-6), where what is left is sums of absolute
                               values over 2 x 4 .. 2 x 23 taps of random bytes whose roundings cancel as 1 / sqrt(taps)
  torch CPU float32 (ATen)     0.59 x at the worst, 0.03 - 0.59 x, case by case within 1.6 x of the restatement's ratio; the same bits as the restatement at scale 1
  bf16                         0.76 - 0.99 x   (a correctly rounded bf16 result is off by up to 2^-8 of its value; the bound has that term alone on top)
A first form of the bound, with the centre's rounding taken tap by tap in absolute value and n u sum |p W| for every sum, measured 0.03 - 0.19 x everywhere: too
loose at the large indices, and tightened to the above.  The mutants measure, on the cases named for each (test_each_mutant_falls_outside_the_bound):
no antialias 1.1e5 - 1.4e5 x, a = -0.75 3.6e3 - 3.1e4 x, no half-pixel centre 2.9e4 - 4.7e5 x, weights not normalised 8.6e4 - 4.5e6 x, channels not swapped
8.7e4 - 1.9e6 x, xend one short 1.2e4 - 5.7e4 x the bound (a = -0.75 changes nothing at scale 1, whose taps fall on the cubic's zeros).

The launcher sweep (test_launcher_bounds_hold_the_statement_windows) restates vd_launch_depth_prep's host arithmetic and walks every (in, out) pair with out in
1 .. 199 and {518, 924, 1022} and every `in` the tap budget admits."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
F = np.float32
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DPT_MEAN, DPT_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
MUTANTS = ("no_antialias", "a_075", "no_half_pixel", "unnormalised", "no_swap", "xend_short")

# name -> (B, (H, W), (th, tw)): the geometries both files run (tests/test_hip_depthprep_bits.py says what each is there for)
CASES = {
    "headline16": (2, (1080, 320), (259, 77)),
    "hd1080_16": (2, (540, 160), (259, 77)),
    "scale5p7": (2, (57, 114), (10, 20)),
    "scale5_5p32": (2, (120, 250), (24, 47)),
    "scale1": (2, (64, 64), (64, 64)),
    "up": (2, (40, 60), (70, 126)),
    "mixed": (2, (108, 54), (20, 60)),
    "small": (2, (33, 65), (8, 16)),
    "tiny": (2, (7, 9), (3, 4)),
    "tw33": (2, (50, 100), (12, 33)),
    "phases": (3, (97, 131), (28, 42)),
    "band_edge": (2, (327, 64), (75, 16)),
    "tile_edge": (2, (13, 46), (21, 67)),
}


def frames_u8(name):
    """The case's random bytes [B, H, W, 3] (BGR), the same in both files."""
    B, (H, W), _ = CASES[name]
    return np.random.default_rng(1000 + list(CASES).index(name)).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def f2bf(f):
    """The kernel's dp_bf16: round to nearest even on the bits, uint32 arithmetic."""
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf2f(h):
    return (np.asarray(h).astype(np.uint32) << np.uint32(16)).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------- the statement
def dp_cubic(x, a=-0.5):
    """dp_cubic on a float32 array: both Horner forms as written, left to right."""
    a = F(a)
    x = np.abs(x)
    p1 = ((a + F(2)) * x - (a + F(3))) * x * x + F(1)
    p2 = (((x - F(5)) * x + F(8)) * x - F(4)) * a
    return np.where(x < F(1), p1, np.where(x < F(2), p2, F(0))).astype(F)


def axis_windows(n_in, n_out, mut=None):
    """dp_weights' window of every output index: (scale, support, invscale, center[n_out], xmin[n_out], xend[n_out]); float32 / int32."""
    scale = F(n_in) / F(n_out)
    down = scale >= F(1) and mut != "no_antialias"
    support = F(2) * scale if down else F(2)
    invscale = F(1) / scale if down else F(1)
    i = np.arange(n_out).astype(F)
    center = scale * i if mut == "no_half_pixel" else scale * (i + F(0.5))
    xmin = np.maximum(((center - support) + F(0.5)).astype(np.int32), 0)          # astype truncates toward zero, as (int) does
    xend = np.minimum(((center + support) + F(0.5)).astype(np.int32), n_in)
    if mut == "xend_short":
        xend = xend - 1
    return scale, support, invscale, center, xmin, xend


def axis_taps(n_in, n_out, mut=None):
    """dp_weights of every output index: (xmin[n_out], n[n_out], w[n_out, max n]); w[i, j] means something for j < n[i] only."""
    _, _, invscale, center, xmin, xend = axis_windows(n_in, n_out, mut)
    n = xend - xmin
    nmax = int(n.max())
    v = np.zeros((n_out, nmax), F)
    total = np.zeros(n_out, F)
    for j in range(nmax):
        vj = dp_cubic((((j + xmin).astype(F) - center) + F(0.5)) * invscale, -0.75 if mut == "a_075" else -0.5)
        live = j < n
        v[:, j] = np.where(live, vj, F(0))
        total = np.where(live, total + vj, total)
    if mut != "unnormalised":
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.where(total[:, None] != F(0), v / total[:, None], v)
    return xmin, n, v.astype(F)


_SUMS = {}


def _filter_sums(frames, th, tw, mut, key):
    """The 2-D filter sums s [B, th, tw, 3] (RGB) in float32: horizontal sums per input row first, then the vertical sums, every sum over ascending j from +0."""
    if key is not None and (key, th, tw, mut) in _SUMS:
        return _SUMS[(key, th, tw, mut)]
    B, H, W, _ = frames.shape
    img = (frames if mut == "no_swap" else frames[..., ::-1]).astype(F)
    x0, nx, wx = axis_taps(W, tw, mut)
    y0, ny, wy = axis_taps(H, th, mut)
    hs = np.empty((B, H, tw, 3), F)
    for ox in range(tw):
        s = np.zeros((B, H, 3), F)
        for j in range(int(nx[ox])):
            s = s + img[:, :, int(x0[ox]) + j, :] * wx[ox, j]
        hs[:, :, ox, :] = s
    out = np.empty((B, th, tw, 3), F)
    for oy in range(th):
        s = np.zeros((B, tw, 3), F)
        for j in range(int(ny[oy])):
            s = s + hs[:, int(y0[oy]) + j] * wy[oy, j]
        out[:, oy] = s
    if key is not None:
        out.setflags(write=False)
        _SUMS[(key, th, tw, mut)] = out
    return out


def prep_statement(frames, th, tw, mean, std, dtype, mut=None, key=None):
    """k_depth_prep / k_depth_prep_strip: uint8 BGR [B, H, W, 3] -> NHWC [B, th, tw, 3], float32 for dtype "f32", bf16 bits (uint16) for "bf16".  `key` names the
    frames for the cache of filter sums (which do not depend on mean, std or dtype)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3
    s = _filter_sums(frames, int(th), int(tw), mut, key)
    m, sd = np.asarray(mean, F).reshape(1, 1, 1, 3), np.asarray(std, F).reshape(1, 1, 1, 3)
    out = ((s / F(255.0)) - m) / sd
    assert out.dtype == F
    return out if dtype == "f32" else f2bf(out)


# ---------------------------------------------------------------------------------------------------------------------------- reference and bound
def _cubic64(x):
    x = np.abs(x)
    return np.where(x < 1, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2, -0.5 * (((x - 5) * x + 8) * x - 4), 0.0))


def cubic_rounding(x):
    """Running error of dp_cubic's float32 evaluation at the exact argument x (every operation rounds its own result once; the constants are exact)."""
    x = np.abs(x)
    t1 = 1.5 * x
    q1 = t1 - 2.5
    q2 = q1 * x
    q3 = q2 * x
    e = U * np.abs(t1) + U * np.abs(q1)
    e = e * x + U * np.abs(q2)
    e = e * x + U * np.abs(q3)
    inner = e + U * np.abs(q3 + 1)
    r1 = x - 5
    r2 = r1 * x
    r3 = r2 + 8
    r4 = r3 * x
    r5 = r4 - 4
    e = U * np.abs(r1) * x + U * np.abs(r2)
    e = e + U * np.abs(r3)
    e = e * x + U * np.abs(r4)
    outer = 0.5 * (e + U * np.abs(r5))                   # * a = -0.5 is exact
    return np.where(x < 1, inner, np.where(x < 2, outer, 0.0))


def _cubic_dx(x):
    """d cubic / dx, signed."""
    ax = np.abs(x)
    return np.sign(x) * np.where(ax < 1, 4.5 * ax * ax - 5 * ax, np.where(ax < 2, -0.5 * (3 * ax * ax - 10 * ax + 8), 0.0))


def axis_reference(n_in, n_out):
    """One axis in float64 over all input pixels -> dict: W [n_out, n_in] the normalised weights, dW the bound of their float32 error but for the centre's
    rounding, G = dW / dcenter (signed), dcen [n_out] = u |center|, k0 / k1 [n_out] the range of the taps either evaluation can see."""
    scale = float(F(n_in) / F(n_out))                     # the float32 value, widened
    invscale = 1.0 / scale if scale >= 1 else 1.0
    center = scale * (np.arange(n_out) + 0.5)
    d = np.arange(n_in)[None, :] - center[:, None]
    x = (d + 0.5) * invscale
    c = _cubic64(x)
    ex = invscale * U * (np.abs(d) + np.abs(d + 0.5)) + 2 * U * np.abs(x)
    ex_all = ex + invscale * U * np.abs(center)[:, None]
    near = np.abs(x) <= 2 + ex_all                        # the taps either evaluation can see
    dv = np.where(near, np.abs(_cubic_dx(x)) * ex + 2.5 * ex_all * ex_all + cubic_rounding(x), 0.0)
    T = c.sum(1, keepdims=True)
    dT = dv.sum(1, keepdims=True) + U * np.where(near, np.abs(np.cumsum(c, 1)), 0.0).sum(1, keepdims=True)
    W = c / T
    dW = dv / np.abs(T) + np.abs(W) * dT / np.abs(T) + U * np.abs(W)
    dc = -invscale * _cubic_dx(x)
    G = (dc - W * dc.sum(1, keepdims=True)) / T
    k0 = near.argmax(1)
    k1 = n_in - near[:, ::-1].argmax(1)
    return dict(W=W, dW=dW, G=G, dcen=U * np.abs(center), k0=k0, k1=k1)


def _sum_rounding(p, axis, A):
    """u (sum |p_k W_k| + sum_j |partial sum j|) of the filter sums of p along `axis` (1 = rows, 2 = columns) with the weights of A: the products' roundings
    and the running sum's.  -> the shape of p with that axis replaced by the outputs."""
    out = []
    for i in range(A["W"].shape[0]):
        k0, k1 = int(A["k0"][i]), int(A["k1"][i])
        w = A["W"][i, k0:k1]
        t = (p[:, :, k0:k1] * w[None, None, :, None]) if axis == 2 else (p[:, k0:k1] * w[None, :, None, None])
        out.append(U * (np.abs(t).sum(axis) + np.abs(np.cumsum(t, axis)).sum(axis)))
    return np.stack(out, axis)


_REF = {}


def reference_and_bound(name, mean, std):
    """-> (float64 reference [B, th, tw, 3], the float32 bound of the module docstring per element)."""
    key = (name, tuple(mean), tuple(std))
    if key in _REF:
        return _REF[key]
    B, (H, W), (th, tw) = CASES[name]
    p = frames_u8(name)[..., ::-1].astype(np.float64)
    X, Y = axis_reference(W, tw), axis_reference(H, th)
    hx, vy = "bhwc,xw->bhxc", "bhxc,yh->byxc"
    h = np.einsum(hx, p, X["W"])
    Eh = np.einsum(hx, p, X["dW"]) + _sum_rounding(p, 2, X)
    s = np.einsum(vy, h, Y["W"])
    Es = np.einsum(vy, Eh, np.abs(Y["W"])) + np.einsum(vy, np.abs(h), Y["dW"]) + _sum_rounding(h, 1, Y)
    Es = Es + np.abs(np.einsum(vy, np.einsum(hx, p, X["G"]), Y["W"])) * X["dcen"][None, None, :, None]
    Es = Es + np.abs(np.einsum(vy, h, Y["G"])) * Y["dcen"][None, :, None, None]
    m, sd = (np.asarray(v, F).astype(np.float64).reshape(1, 1, 1, 3) for v in (mean, std))
    ref = (s / 255.0 - m) / sd
    bnd = (Es / 255.0 + U * np.abs(s) / 255.0 + U * np.abs(s / 255.0 - m)) / sd + U * np.abs(ref)
    bnd = bnd + 2.0 ** -40 * (np.abs(s) / 255.0 / sd + np.abs(ref) + 1e-30)
    _REF[key] = (ref, bnd)
    return _REF[key]


def ratio_to_bound(got, name, mean, std, bf16=False):
    ref, bnd = reference_and_bound(name, mean, std)
    if bf16:
        bnd = bnd + 2.0 ** -8 * (np.abs(ref) + bnd)
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float((err / bnd).max()), float(err.max())


def statement_of_case(name, dtype, mean=IMAGENET_MEAN, std=IMAGENET_STD, mut=None):
    _, _, (th, tw) = CASES[name]
    return prep_statement(frames_u8(name), th, tw, mean, std, dtype, mut, key=name)


def aten_f32(name, mean, std):
    """torch's CPU float32 evaluation of the same operator, NHWC."""
    _, _, (th, tw) = CASES[name]
    x = torch.from_numpy(np.ascontiguousarray(frames_u8(name)[..., ::-1])).permute(0, 3, 1, 2).float()
    x = torch.nn.functional.interpolate(x, size=(th, tw), mode="bicubic", antialias=True, align_corners=False)
    m, sd = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1) for v in (mean, std))
    return (((x / 255.0) - m) / sd).permute(0, 2, 3, 1).numpy()


# ---------------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_is_within_the_bound(name, record_property):
    """The restatement and ATen's CPU float32 kernel, both against the float64 reference, both inside the derived bound; bf16 inside it with its one rounding.
    test_the_bound_bites holds the ratio from below."""
    for mean, std in ((IMAGENET_MEAN, IMAGENET_STD),) + (((DPT_MEAN, DPT_STD),) if name in ("scale5_5p32", "tiny") else ()):
        got = statement_of_case(name, "f32", mean, std)
        r, e = ratio_to_bound(got, name, mean, std)
        yard = aten_f32(name, mean, std)
        ra, ea = ratio_to_bound(yard, name, mean, std)
        rb, _ = ratio_to_bound(bf2f(statement_of_case(name, "bf16", mean, std)), name, mean, std, bf16=True)
        same = bool(np.array_equal(got, yard))
        print(f"PREP_HOST {name} std {std[0]}: statement {r:.3f} x the bound (max err {e:.2e}), ATen f32 cpu {ra:.3f} x ({ea:.2e}), bf16 {rb:.3f} x, "
              f"statement == ATen: {same}")
        record_property(f"ratio_{std[0]}", r)
        assert np.isfinite(got).all()
        assert r <= 1.0, (name, r)
        assert ra <= 1.0, (name, ra)
        assert rb <= 1.0, (name, rb)
        if name == "scale1":
            assert same                                   # scale 1: four taps 0, 1, 0, 0 -- the same float32 operations in any order


@pytest.mark.parametrize("name", ["hd1080_16", "headline16", "up"])
def test_the_bound_bites(name):
    """A bound twenty times the error would catch nothing.  Where the centre's rounding (u x the index) leads, the restatement comes within 2 - 3 x of it."""
    r, _ = ratio_to_bound(statement_of_case(name, "f32"), name, IMAGENET_MEAN, IMAGENET_STD)
    assert r > 0.05, (name, r)


def test_f2bf_is_atens_rounding():
    a = (np.random.default_rng(5).standard_normal(4096) * 3).astype(F)
    assert np.array_equal(bf2f(f2bf(a)), torch.from_numpy(a).to(torch.bfloat16).float().numpy())


def test_statement_windows_are_the_cubics_support():
    """[xmin, xend) holds exactly the pixels with -2 < x <= 2 (in float64 on the widened scale, away from the float32 rounding of the edge), which is what lets
    the reference sum over all pixels; and no window is empty."""
    for name in sorted(CASES):
        _, (H, W), (th, tw) = CASES[name]
        for n_in, n_out in ((H, th), (W, tw)):
            scale, _, _, _, xmin, xend = axis_windows(n_in, n_out)
            assert (xend > xmin).all()
            inv = 1.0 / float(scale) if scale >= 1 else 1.0
            x = (np.arange(n_in)[None, :] - float(scale) * (np.arange(n_out) + 0.5)[:, None] + 0.5) * inv
            k = np.arange(n_in)[None, :]
            inside = (k >= xmin[:, None]) & (k < xend[:, None])
            edge = np.abs(np.abs(x) - 2) < 1e-4
            assert np.array_equal(inside | edge, ((x > -2) & (x <= 2)) | edge), (name, n_in, n_out)


# the cases on which each mutant must be outside the bound
MUTANT_CASES = {"no_antialias": ["headline16", "scale5p7"], "a_075": ["up", "headline16", "tiny"], "no_half_pixel": ["scale1", "up", "scale5p7"],
                "unnormalised": ["tiny", "scale5p7", "up"], "no_swap": ["scale1", "headline16"], "xend_short": ["hd1080_16", "scale5_5p32"]}


@pytest.mark.parametrize("mut", MUTANTS)
def test_each_mutant_falls_outside_the_bound(mut, record_property):
    """No antialias (support and argument not scaled), a = -0.75, the half-pixel centre dropped, weights not normalised (it shows where the border clips a
    window), channels not swapped, xend one short: each is outside the derived bound on every case named for it, where the restatement is inside."""
    assert set(MUTANT_CASES) == set(MUTANTS)
    for name in MUTANT_CASES[mut]:
        r, _ = ratio_to_bound(statement_of_case(name, "f32", mut=mut), name, IMAGENET_MEAN, IMAGENET_STD)
        r0, _ = ratio_to_bound(statement_of_case(name, "f32"), name, IMAGENET_MEAN, IMAGENET_STD)
        print(f"PREP_MUTANT {mut} {name}: {r:.3e} x the bound (statement {r0:.3f} x)")
        record_property(f"{mut}_{name}", r)
        assert r0 <= 1.0 < r, (mut, name, r, r0)


# ---------------------------------------------------------------------------------------------------------------------------- the launcher's arithmetic
_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "visiondepth3d_amd", "csrc", "vd3d_depthprep.hip")
PINNED = {"DP_TX": 32, "DP_TY": 8, "DP_KMAX": 24, "DPF_SX": 32, "DPF_BY": 32, "DPF_HROWS": 160, "DPF_CH": 16, "DPF_ROWB": 640, "DPF_RS": 168, "DPF_NLD": 11}
SWEEP_OUT = tuple(range(1, 200)) + (518, 924, 1022)


def launcher_axis(n_in, n_out):
    """vd_launch_depth_prep's host arithmetic for one axis, for an array of input sizes: float32 like the launcher's, (int) truncating.  -> dict of arrays:
    admitted (the tap budget), cols_max / rows_max (the tile kernel's capacities if this axis is the horizontal / the vertical one), down (scale >= 1),
    rowb_ok (the strip's DPF_ROWB test), by (the strip's band height after the halving against DPF_HROWS, 0 = the strip kernel does not apply)."""
    K = PINNED
    n_in = np.asarray(n_in)
    scale = n_in.astype(F) / F(n_out)
    down = scale >= F(1)
    sup = np.where(down, F(2) * scale, F(2)).astype(F)
    admitted = (F(2) * sup).astype(np.int32) + 2 <= K["DP_KMAX"]
    cols_max = (scale * F(K["DP_TX"]) + F(2) * sup).astype(np.int32) + 4
    rows_max = (scale * F(K["DP_TY"]) + F(2) * sup).astype(np.int32) + 4
    rowb_ok = down & (((scale * F(K["DPF_SX"]) + F(2) * sup).astype(np.int32) + 4) * 3 <= K["DPF_ROWB"])
    by = np.where(down, K["DPF_BY"], 0)
    for _ in range(3):                                                     # 32 -> 16 -> 8 -> 4 (< 8: none)
        over = (by >= 8) & ((scale * by.astype(F) + F(2) * sup).astype(np.int32) + 4 > K["DPF_HROWS"])
        by = np.where(over, by >> 1, by)
    by = np.where(by < 8, 0, by)
    return dict(scale=scale, admitted=admitted, cols_max=cols_max, rows_max=rows_max, down=down, rowb_ok=rowb_ok, by=by)


def _windows_2d(n_in, n_out):
    """axis_windows for an array of input sizes at once: xmin, xend [len(n_in), n_out] (the same float32 operations, element for element)."""
    scale = (n_in.astype(F) / F(n_out))[:, None]
    support = np.where(scale >= F(1), F(2) * scale, F(2)).astype(F)
    center = scale * (np.arange(n_out).astype(F) + F(0.5))[None, :]
    xmin = np.maximum(((center - support) + F(0.5)).astype(np.int32), 0)
    xend = np.minimum(((center + support) + F(0.5)).astype(np.int32), n_in[:, None].astype(np.int32))
    return xmin, xend


def _tile_spans(xmin, xend, T):
    """Input span [c_lo, c_hi) of every tile of T outputs, as the kernels take it: first window's start to last window's end.  [geometries, tiles]."""
    n_out = xmin.shape[1]
    first = np.arange(0, n_out, T)
    last = np.minimum(first + T, n_out) - 1
    return xend[:, last] - xmin[:, first]


def test_launcher_constants_are_the_sources():
    text = open(_SRC).read()
    for k, v in PINNED.items():
        m = re.search(r"^#define %s (\d+)\b" % k, text, re.M)
        assert m and int(m.group(1)) == v, k
    assert "(int)(2.f * sup_w) + 2 > DP_KMAX" in text and "a.in_cols_max = (int)(a.scale_w * DP_TX + 2.f * sup_w) + 4;" in text
    assert "a.in_rows_max = (int)(a.scale_h * DP_TY + 2.f * sup_h) + 4;" in text
    assert "for (by = DPF_BY; by >= 8 && (int)(a.scale_h * by + 2.f * sup_h) + 4 > DPF_HROWS; by >>= 1) {}" in text
    assert "((int)(a.scale_w * DPF_SX + 2.f * sup_w) + 4) * 3 <= DPF_ROWB" in text and "if (lds > 150 * 1024) return 1;" in text


def test_statement_windows_match_their_batched_form():
    for n_in, n_out in ((1080, 259), (57, 10), (40, 70), (114, 20), (9, 4)):
        _, _, _, _, a, b = axis_windows(n_in, n_out)
        a2, b2 = _windows_2d(np.array([n_in]), n_out)
        assert np.array_equal(a, a2[0]) and np.array_equal(b, b2[0])


def test_launcher_bounds_hold_the_statement_windows():
    """Every (in, out) with out in 1 .. 199 and {518, 924, 1022} and every `in` the tap budget admits, each axis in both roles (columns: 32-wide tiles and strips;
    rows: 8-row tiles and bands of `by` rows).  The kernels clamp silently at each of these capacities; the statement has no clamp, so equal bits need every one
    of them to hold.  Pinned result: 128 467 geometries, at most 23 taps, least slack 3 columns, 3 rows and 7 band rows."""
    K = PINNED
    count, max_taps = 0, 0
    slack_cols = slack_rows = slack_band = slack_stage = 10 ** 9
    min_by = 10 ** 9
    worst_cols = worst_rows = 0
    for n_out in SWEEP_OUT:
        cand = np.arange(1, 6 * n_out + 8)
        plan = launcher_axis(cand, n_out)
        assert not plan["admitted"][-4:].any()                              # the candidates run past the last admitted size
        for lo in range(0, len(cand), 1024):
            sel = np.nonzero(plan["admitted"][lo:lo + 1024])[0] + lo
            if not len(sel):
                continue
            n_in = cand[sel]
            p = {k: v[sel] for k, v in plan.items()}
            xmin, xend = _windows_2d(n_in, n_out)
            taps = xend - xmin
            assert int(taps.min()) >= 1, n_out                              # no window is empty
            assert int(taps.max()) <= K["DP_KMAX"], n_out                   # dp_weights' n > DP_KMAX never holds
            # windows start and end in ascending order: every window of a tile lies inside [first window's start, last window's end)
            assert (np.diff(xmin, axis=1) >= 0).all() and (np.diff(xend, axis=1) >= 0).all(), n_out
            assert (xmin >= 0).all() and (xend <= n_in[:, None]).all()
            cols = _tile_spans(xmin, xend, K["DP_TX"]).max(1)
            rows = _tile_spans(xmin, xend, K["DP_TY"]).max(1)
            assert (cols <= p["cols_max"]).all(), n_out                     # min(c_hi - c_lo, in_cols_max) never clamps
            assert (rows <= p["rows_max"]).all(), n_out                     # min(r_hi - r_lo, in_rows_max) never clamps
            slack_cols = min(slack_cols, int((p["cols_max"] - cols).min()))
            slack_rows = min(slack_rows, int((p["rows_max"] - rows).min()))
            worst_cols, worst_rows = max(worst_cols, int(p["cols_max"].max())), max(worst_rows, int(p["rows_max"].max()))
            dn = p["down"]
            if dn.any():
                # the strip kernel applies to every admitted down-scale, with bands of 16 rows at the least
                assert p["rowb_ok"][dn].all() and (p["by"][dn] >= 16).all(), n_out
                min_by = min(min_by, int(p["by"][dn].min()))
                assert (cols[dn] * 3 <= K["DPF_ROWB"]).all()                # min(c_hi - c_lo, DPF_ROWB / 3) never clamps
                # the strip's horizontal pass reads dwords (start >> 2) .. (start >> 2) + 3 ceil(n / 4) of a staged row of DPF_RS, start = phase + 3 (x0 - c_lo)
                first = (np.arange(n_out) // K["DPF_SX"]) * K["DPF_SX"]
                start = 3 + 3 * (xmin[dn] - xmin[dn][:, first])
                reach = (start >> 2) + 3 * ((taps[dn] + 3) >> 2)
                slack_stage = min(slack_stage, K["DPF_RS"] - 1 - int(reach.max()))
                assert int(reach.max()) < K["DPF_RS"]
                for by in (16, 32):
                    m = dn & (p["by"] == by)
                    if m.any():
                        band = _tile_spans(xmin[m], xend[m], by).max(1)
                        assert (band <= K["DPF_HROWS"]).all(), (n_out, by)  # min(r_hi - r_lo, DPF_HROWS) and min(y0s[..], nrow - rb) never clamp
                        slack_band = min(slack_band, int((K["DPF_HROWS"] - band).min()))
            max_taps = max(max_taps, int(taps.max()))
            count += len(sel)
    # the general kernel's dynamic LDS at the largest capacities of both axes together: the launcher's 150 KB test refuses nothing the tap budget admits
    lds = 4 * (K["DP_TX"] + K["DP_TY"]) * K["DP_KMAX"] + 4 * 2 * (K["DP_TX"] + K["DP_TY"]) + 4 * worst_rows * K["DP_TX"] * 3 + worst_rows * worst_cols * 3
    assert ((lds + 15) & ~15) <= 150 * 1024
    # a fetched row: 16 lanes x DPF_NLD dwords cover the phase, the row and the three bytes that complete its last dword
    assert 16 * K["DPF_NLD"] >= (3 + K["DPF_ROWB"] + 3) >> 2 and 16 * K["DPF_NLD"] >= K["DPF_RS"]
    print(f"PREP_SWEEP {count} geometries, at most {max_taps} taps, least slack {slack_cols} columns, {slack_rows} rows, {slack_band} band rows, "
          f"{slack_stage} staged dwords; least band height {min_by}; largest tile {worst_rows} x {worst_cols}")
    assert (count, max_taps, slack_cols, slack_rows, slack_band, min_by) == (128467, 23, 3, 3, 7, 16)


def test_the_cases_are_what_they_are_named_for():
    """The tap counts, band heights and slacks the shared cases were chosen for, from the restated launcher and windows."""
    def win(n_in, n_out):
        return axis_windows(n_in, n_out)[4:]

    def taps(n_in, n_out):
        a, b = win(n_in, n_out)
        return int((b - a).max())

    def plan(n_in, n_out):
        p = launcher_axis(np.array([n_in]), n_out)
        assert bool(p["admitted"][0])
        return {k: v[0] for k, v in p.items()}

    def span(n_in, n_out, T):
        a, b = win(n_in, n_out)
        return int(_tile_spans(a[None], b[None], T).max())
    assert [int(plan(*g)["by"]) for g in ((1080, 259), (327, 75), (540, 259), (57, 10), (120, 24), (64, 64))] == [32, 32, 32, 16, 16, 32]
    assert (taps(57, 10), taps(114, 20), taps(250, 47), taps(1080, 259), taps(320, 77)) == (23, 23, 22, 17, 17)     # the strip pads 17, 22 and 23 to 20 and 24
    assert {int(n) for n in np.subtract(*win(114, 20)[::-1])} >= {22, 23}
    assert F(1080) / F(259) == F(2160) / F(518) and F(320) / F(77) == F(3840) / F(924) and F(540) / F(259) == F(1080) / F(518) and F(160) / F(77) == F(1920) / F(924)
    assert not launcher_axis(np.array([114]), 19)["admitted"][0] and F(57) / F(10) == F(5.7)     # 4 x 5.7 = 22.8 -> 24 taps budgeted; 4 x 5.75 = 23 -> 25: refused
    assert not launcher_axis(np.array([115]), 20)["admitted"][0]
    assert PINNED["DPF_HROWS"] - span(327, 75, 32) == 7                                          # band_edge: the least band slack of the sweep
    assert int(plan(13, 21)["rows_max"]) - span(13, 21, 8) == 3 and int(plan(46, 67)["cols_max"]) - span(46, 67, 32) == 3     # tile_edge: the least tile slack
    for name, (_, (Hh, W), (th, tw)) in CASES.items():
        down = bool(plan(Hh, th)["down"]) and bool(plan(W, tw)["down"])
        assert down == (name not in ("up", "mixed", "tile_edge")), name
    assert 47 % 32 and 33 % 32 == 1 and 77 % 32 and 20 < 32 and 4 < 32 and 3 < 8
