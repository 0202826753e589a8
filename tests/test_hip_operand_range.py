"""GPU tests (-m gpu) of the split-operand matrix kernels at the EDGES of their operand range -- vd3d_gemm_x3, vd3d_conv3x3_x2 / _x3, vd3d_attention_x3,
vd3d_attention_f32 against float64 torch on the same operands.  The accuracy tests beside them (test_hip_gemm.py, test_hip_conv_x3.py,
test_hip_attention_f32.py) feed well-conditioned operands; these state what include/vd3d.h promises where a trained network goes:

  * fp16x2 below 2^-2, where the second fp16 term of an operand is subnormal (|x - h1 - h2| <= 2^-25), and below 2^-12, where it is gone;
  * fp16x2 at its ceiling (65 504 for the GEMM and the convolution, 4 094 for the attention, which scales q, k, v by 2^4): faithful just below, Inf / NaN
    -- never a finite wrong number -- above, and only in the outputs that depend on the offending element;
  * bf16x3 and float32 have float32's exponent: stated as EXACT invariance under scaling by 2^+-60;
  * the online-softmax state machine of the three attention kernels where the running maximum arrives late: known answers with a rescale by an exact
    zero in every tile, a maximum in the masked last tile, probabilities that underflow to exactly 0, logits that are all hugely negative; NaN containment;
  * the > 64 KB dynamic-LDS opt-in on a second device.

Every case runs in a second or two.  profiles/r09_range_and_outliers.md has the measured figures and what each test showed on a deliberately broken build."""
import math

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
CL = torch.channels_last
D = 64


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _pow2_uniform(shape, lo, hi, g, device="cuda"):
    """+-2^u, u uniform in [lo, hi): every binade equally likely, full random mantissas."""
    u = torch.rand(shape, device=device, generator=g) * (hi - lo) + lo
    s = torch.randint(0, 2, shape, device=device, generator=g).float() * 2 - 1
    return s * torch.exp2(u)


# ---------------------------------------------------------------------------------------------------------------- fp16x2: small operands
def x2_split_error(ax):
    """include/vd3d.h on the two-term split of an activation |x|: 2^-25 absolute below 2^-2 (the second fp16 term is subnormal), 2^-22 |x| from there."""
    return torch.where(ax < 2.0 ** -2, torch.full_like(ax, 2.0 ** -25), ax * 2.0 ** -22)


def x2_small_bound(per, S, A):
    """Per element: |y - y64| <= per + 2^-21 S + 2 A.  per = sum_k x2_split_error(x_k) |w_k| is the header's statement; S = sum |x||w| (+ |b|), and 2^-21 S
    covers the weight split (2^-22 relative) and the dropped x2 w2; A is the float32 accumulation term: the float32 library result's own |y32 - y64|, the
    maximum over the element's output tile, measured beside the kernel."""
    return per + 2.0 ** -21 * S + 2.0 * A


def _tile_max(err, tiles):
    """err [..., R, C] -> each element replaced by the maximum of its (tr x tc) tile (ragged last tiles included)."""
    tr, tc = tiles
    Rr, Cc = err.shape[-2:]
    p = F.pad(err, (0, -Cc % tc, 0, -Rr % tr))
    lead = p.shape[:-2]
    t = p.reshape(*lead, p.shape[-2] // tr, tr, p.shape[-1] // tc, tc).amax(dim=(-3, -1), keepdim=True)
    return t.expand(*lead, p.shape[-2] // tr, tr, p.shape[-1] // tc, tc).reshape(p.shape)[..., :Rr, :Cc]


SMALL_RANGES = [(-12, -6), (-20, -12)]   # second fp16 term subnormal; second term gone (the first one subnormal below 2^-14)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("lo,hi", SMALL_RANGES)
def test_gemm_fp16x2_small_magnitude_contract(R, lo, hi, bias):
    """x = +-2^u, u uniform in [lo, hi], M, K, N = 300, 256, 96 (two row tiles, a ragged column tile).  A correct split sits at 0.16 of per + 2^-21 S in
    both ranges (CPU emulation, double accumulation); one that flushes the subnormal second term is 10.6 x over it in the first range."""
    M, K, N = 300, 256, 96
    g = torch.Generator(device="cuda").manual_seed(1000 - lo + bias)
    x = _pow2_uniform((M, K), lo, hi, g)
    w = torch.randn(N, K, device="cuda", generator=g) * 0.05
    b = torch.randn(N, device="cuda", generator=g) * 2.0 ** (hi - 3) if bias else None    # of the size of the products: a large bias would hide them in S
    y = R.linear_x3(x, R.gemm_x3_pack(w, "fp16x2"), N, b, mode="fp16x2")
    y64 = F.linear(x.double(), w.double(), None if b is None else b.double())
    S = x.abs().double() @ w.abs().double().T + (0.0 if b is None else b.abs().double())
    A = _tile_max((F.linear(x, w, b).double() - y64).abs(), (256, 256))    # the float32 library GEMM beside it, per 256 x 256 output tile
    per = x2_split_error(x.abs().double()) @ w.abs().double().T
    bound = x2_small_bound(per, S, A)
    err = (y.double() - y64).abs()
    print(f"GEMM_X2_SMALL u in [{lo}, {hi}] bias {bias}: max err / bound {float((err / bound).max()):.3f}, err / (per + 2^-21 S) {float((err / (bound - 2 * A)).max()):.3f}, "
          f"per / bound {float((per / bound).mean()):.2f}, A / bound {float((A / bound).mean()):.3f}")
    assert bool(torch.isfinite(y).all())
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("lo,hi", SMALL_RANGES)
def test_conv_x2_small_magnitude_contract(R, lo, hi):
    """The same statement for vd3d_conv3x3_x2 at (2, 21, 45, 48 -> 64): ragged 16 x 32 tiles, three input-channel chunks; the float32 yardstick is PyTorch's
    CPU convolution, as in test_conv3x3_x2_is_float32_faithful."""
    B, H, W, Cin, Cout = 2, 21, 45, 48, 64
    g = torch.Generator(device="cuda").manual_seed(2000 - lo)
    x = _pow2_uniform((B, Cin, H, W), lo, hi, g).contiguous(memory_format=CL)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) * 0.05
    y = R.conv3x3_x2(x, R.conv3x3_x2_pack(w), Cout)
    y64 = F.conv2d(x.double(), w.double(), None, 1, 1)
    S = F.conv2d(x.abs().double(), w.abs().double(), None, 1, 1)
    y32 = F.conv2d(x.cpu(), w.cpu(), None, 1, 1).to(x.device)
    A = _tile_max((y32.double() - y64).abs().amax(dim=1, keepdim=True), (16, 32)).expand_as(y64)   # per 16 x 32 output tile, all channels
    bound = x2_small_bound(F.conv2d(x2_split_error(x.abs().double()), w.abs().double(), None, 1, 1), S, A)
    err = (y.double() - y64).abs()
    print(f"CONV_X2_SMALL u in [{lo}, {hi}]: max err / bound {float((err / bound).max()):.3f}, err / (per + 2^-21 S) {float((err / (bound - 2 * A)).max()):.3f}")
    assert bool(torch.isfinite(y).all())
    assert bool((err <= bound).all()), float((err / bound).max())


# ---------------------------------------------------------------------------------------------------------------- fp16x2: the ceiling
def _gemm_err(y, x, w, b):
    ref = F.linear(x.double(), w.double(), b.double())
    scale = x.abs().double() @ w.abs().double().T + b.abs().double()
    d = (y.double() - ref).abs()
    return float((d / scale).max()), float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def test_gemm_fp16x2_just_below_the_ceiling_is_faithful(R):
    """|x| in [2^13, 65 504): the fp16x2 bar of test_gemm_x3_is_float32_faithful (K >= 64): maximum <= max(2 x the float32 library GEMM's, 2^-22), RMS <= 1.5 x."""
    M, K, N = 300, 256, 96
    g = torch.Generator(device="cuda").manual_seed(31)
    x = _pow2_uniform((M, K), 13.0, math.log2(65504.0), g).clamp(-65503.0, 65503.0)
    x[0, 0], x[299, 255] = 65503.0, -65503.0
    w = torch.randn(N, K, device="cuda", generator=g) * 0.05
    b = torch.randn(N, device="cuda", generator=g)
    y = R.linear_x3(x, R.gemm_x3_pack(w, "fp16x2"), N, b, mode="fp16x2")
    assert bool(torch.isfinite(y).all())
    (e3, r3), (e32, r32) = _gemm_err(y, x, w, b), _gemm_err(F.linear(x, w, b), x, w, b)
    print(f"GEMM_X2_CEILING max {e3:.3e} (f32 {e32:.3e}) rms {r3:.3e} (f32 {r32:.3e})")
    assert e3 <= max(2.0 * e32, 2.0 ** -22), (e3, e32)
    assert r3 <= 1.5 * r32 + 1e-9, (r3, r32)


def test_gemm_fp16x2_above_the_ceiling_is_not_finite_and_contained(R):
    """One element 1e5 (> 65 504): its whole output row is Inf / NaN -- not a finite wrong number -- and every other row is bit-identical to the run with 1.0
    in its place."""
    M, K, N = 300, 256, 96
    g = torch.Generator(device="cuda").manual_seed(32)
    x = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * 0.05
    b = torch.randn(N, device="cuda", generator=g)
    img = R.gemm_x3_pack(w, "fp16x2")
    for r, c in ((0, 0), (257, 131), (299, 255)):      # first tile, second tile, the very last element
        x[r, c] = 1.0
        clean = R.linear_x3(x, img, N, b, mode="fp16x2")
        assert bool(torch.isfinite(clean).all())
        x[r, c] = 1.0e5
        y = R.linear_x3(x, img, N, b, mode="fp16x2")
        x[r, c] = 1.0
        assert not bool(torch.isfinite(y[r]).any()), (r, c, int(torch.isfinite(y[r]).sum()))
        keep = torch.arange(M, device="cuda") != r
        assert torch.equal(y[keep], clean[keep]), (r, c)


def test_conv_x2_ceiling(R):
    """vd3d_conv3x3_x2 at (2, 21, 45, 48 -> 64): |x| in [2^13, 65 504) meets the bar of test_conv3x3_x2_is_float32_faithful; one element 1e5 makes its 3 x 3
    neighbourhood non-finite over all output channels and leaves every other output bit-identical to the run with 1.0 in its place."""
    B, H, W, Cin, Cout = 2, 21, 45, 48, 64
    g = torch.Generator(device="cuda").manual_seed(33)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) * 0.05
    img = R.conv3x3_x2_pack(w)
    x = _pow2_uniform((B, Cin, H, W), 13.0, math.log2(65504.0), g).clamp(-65503.0, 65503.0).contiguous(memory_format=CL)
    y = R.conv3x3_x2(x, img, Cout)
    assert bool(torch.isfinite(y).all())
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    y32 = F.conv2d(x.cpu(), w.cpu(), None, 1, 1).to(x.device)
    scale = F.conv2d(x.abs().double(), w.abs().double(), None, 1, 1)
    e3, e32 = float(((y.double() - ref).abs() / scale).max()), float(((y32.double() - ref).abs() / scale).max())
    r3 = float((y.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    r32 = float((y32.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"CONV_X2_CEILING max {e3:.3e} (f32 {e32:.3e}) rms {r3:.3e} (f32 {r32:.3e})")
    assert e3 <= max(2.5 * e32, 2.0 ** -21), (e3, e32)
    assert r3 <= 1.5 * r32 + 1e-9, (r3, r32)
    x = torch.randn(B, Cin, H, W, device="cuda", generator=g).contiguous(memory_format=CL)
    for bb, c, i, j in ((0, 0, 0, 0), (1, 47, 20, 44), (1, 17, 15, 32)):    # a corner, the last element, a tile boundary in both directions
        x[bb, c, i, j] = 1.0
        clean = R.conv3x3_x2(x, img, Cout)
        x[bb, c, i, j] = 1.0e5
        y = R.conv3x3_x2(x, img, Cout)
        x[bb, c, i, j] = 1.0
        hit = torch.zeros(B, 1, H, W, dtype=torch.bool, device="cuda")
        hit[bb, 0, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = True
        hit = hit.expand_as(y)
        assert not bool(torch.isfinite(y[hit]).any()), (bb, c, i, j)
        assert torch.equal(y[~hit], clean[~hit]), (bb, c, i, j)


def _attn_ref(qkv, scale):
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    B, H, T, _ = q.shape
    ref = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale, dim=-1) @ v.double()
    o32 = F.scaled_dot_product_attention(q, k, v, scale=scale)
    return ref.transpose(1, 2).reshape(B, T, H * D), o32.transpose(1, 2).reshape(B, T, H * D)


def test_attention_fp16x2_ceiling(R):
    """vd3d_attention_x3 in fp16x2 scales q, k, v by 2^4 before their split, so its ceiling is 65 504 / 16 = 4 094 (include/vd3d.h).  (1, 77, 3): |v| up to 4 000
    meets the fp16x2 bar of test_attention_x3_is_float32_faithful; one v = 5 000 in head 1 makes that output column of head 1 non-finite for every query, one
    k = 5 000 in head 1 all of head 1; heads 0 and 2 stay bit-identical."""
    B, T, H = 1, 77, 3
    g = torch.Generator(device="cuda").manual_seed(34)
    qkv = torch.randn(B, T, 3, H, D, device="cuda", generator=g)
    qkv[:, :, 2] = (torch.rand(B, T, H, D, device="cuda", generator=g) * 2 - 1) * 4000.0
    qkv[0, 5, 2, 1, 7], qkv[0, 76, 2, 2, 63] = 4000.0, -4000.0
    scale = D ** -0.5
    run = lambda t: R.attention_x3(t.view(B, T, 3 * H * D), H, scale, mode="fp16x2")   # noqa: E731
    out = run(qkv)
    assert bool(torch.isfinite(out).all())
    ref, o32 = _attn_ref(qkv, scale)
    e3, e32 = float((out.double() - ref).abs().max()), float((o32.double() - ref).abs().max())
    r3 = float((out.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    r32 = float((o32.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"ATTN_X2_CEILING max {e3:.3e} (f32 {e32:.3e}) rms {r3:.3e} (f32 {r32:.3e})")
    assert e3 <= max(3.0 * e32, 1e-6 * float(ref.abs().max())), (e3, e32)
    assert r3 <= 2.0 * r32 + 1e-8, (r3, r32)
    out = out.view(B, T, H, D)
    for which, t, d in ((2, 40, 9), (1, 70, 33)):     # a value, a key (in the masked last KV tile)
        bad = qkv.clone()
        bad[0, t, which, 1, d] = 5000.0
        o = run(bad).view(B, T, H, D)
        if which == 2:
            assert not bool(torch.isfinite(o[0, :, 1, d]).any())
        else:
            assert not bool(torch.isfinite(o[0, :, 1]).any())
        assert torch.equal(o[:, :, 0], out[:, :, 0]) and torch.equal(o[:, :, 2], out[:, :, 2])


# ---------------------------------------------------------------------------------------------------------------- bf16x3 / f32: no range limit
# Truncation splits and float32 accumulation commute with a power of two while nothing under- or overflows: |x|, |w| in [2^-6, 2^6] and s = +-60 keep the
# smallest third term (2^-6 2^-60 2^-16 ...) near 2^-90 and the largest sum far below 2^127.  (Behaviour at the float32 subnormal floor is not stated.)
SCALES = [-60, 60]


@pytest.mark.parametrize("s", SCALES)
def test_gemm_bf16x3_is_exactly_scale_invariant(R, s):
    M, K, N = 300, 256, 96
    g = torch.Generator(device="cuda").manual_seed(41)
    x, w, b = _pow2_uniform((M, K), -6, 6, g), _pow2_uniform((N, K), -6, 6, g), _pow2_uniform((N,), -6, 6, g)
    f = 2.0 ** s
    y = R.linear_x3(x, R.gemm_x3_pack(w), N, b)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert torch.equal(R.linear_x3(x * f, R.gemm_x3_pack(w), N, b * f), y * f)            # the activations carry the scale
    assert torch.equal(R.linear_x3(x, R.gemm_x3_pack(w * f), N, b * f), y * f)            # the packed weights carry it


@pytest.mark.parametrize("s", SCALES)
def test_conv_x3_is_exactly_scale_invariant(R, s):
    B, H, W, Cin, Cout = 1, 11, 37, 32, 128
    g = torch.Generator(device="cuda").manual_seed(42)
    x = _pow2_uniform((B, Cin, H, W), -6, 6, g).contiguous(memory_format=CL)
    w = _pow2_uniform((Cout, Cin, 3, 3), -6, 6, g)
    f = 2.0 ** s
    y = R.conv3x3_x3(x, R.conv3x3_x3_pack(w), Cout)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert torch.equal(R.conv3x3_x3(x * f, R.conv3x3_x3_pack(w), Cout), y * f)
    assert torch.equal(R.conv3x3_x3(x, R.conv3x3_x3_pack(w * f), Cout), y * f)


@pytest.mark.parametrize("kernel", ["f32", "bf16x3"])
@pytest.mark.parametrize("s", SCALES)
def test_attention_values_are_exactly_scale_invariant(R, kernel, s):
    B, T, H = 2, 77, 3
    g = torch.Generator(device="cuda").manual_seed(43)
    qkv = torch.randn(B, T, 3, H, D, device="cuda", generator=g)
    qkv[:, :, 2] = _pow2_uniform((B, T, H, D), -6, 6, g)
    run = (lambda t: R.attention_f32(t.view(B, T, -1), H, 0.125)) if kernel == "f32" else (lambda t: R.attention_x3(t.view(B, T, -1), H, 0.125, mode="bf16x3"))
    out = run(qkv)
    scaled = qkv.clone()
    scaled[:, :, 2] *= 2.0 ** s
    assert bool(torch.isfinite(out).all()) and torch.equal(run(scaled), out * 2.0 ** s)


# ---------------------------------------------------------------------------------------------------------------- online softmax: known answers
KERNELS = ["f32", "bf16x3", "fp16x2"]


def _attn(R, kernel, qkv, H):
    B, T = qkv.shape[:2]
    flat = qkv.reshape(B, T, -1).contiguous()
    out = R.attention_f32(flat, H, 0.125) if kernel == "f32" else R.attention_x3(flat, H, 0.125, mode=kernel)
    return out.view(B, T, H, D)


def _pointed(T, H, g, kernel):
    """The (iii) pattern of test_attention_*_known_answers: q, k, v = 0.01 randn, then every query is 64 e_5, so a key c e_5 has the logit 64 c / 8 = 8 c and every
    other key a logit near 0.  In fp16x2 the values are rounded to 11 significant bits, which that arithmetic carries exactly (f32 and bf16x3 carry all 24)."""
    qkv = torch.randn(1, T, 3, H, D, device="cuda", generator=g) * 0.01
    if kernel == "fp16x2":
        qkv[:, :, 2] = qkv[:, :, 2].half().float()
    e = torch.zeros(D, device="cuda")
    e[5] = 1.0
    qkv[0, :, 0] = e * 64.0
    return qkv, e


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("T,key", [(200, 197), (65, 64), (257, 256)])
def test_attention_dominant_key_in_the_last_masked_tile(R, kernel, T, key):
    """(a) the running maximum arrives in the LAST KV tile, which is partly masked: 512 above everything before it, so the state of every earlier tile is
    rescaled by alpha = exp2(-738) = 0 exactly and the output is that key's value.  T = 200: key 197 of 192 .. 199; T = 65 and 257: the key is the ONLY valid
    row of its tile (257 also has a second 256-query workgroup, of one query)."""
    g = torch.Generator(device="cuda").manual_seed(T)
    qkv, e = _pointed(T, 2, g, kernel)
    qkv[0, key, 1] = e * 64.0
    out = _attn(R, kernel, qkv, 2)
    assert torch.allclose(out, qkv[:, key:key + 1, 2].expand(1, T, 2, D), rtol=0, atol=1e-30)


@pytest.mark.parametrize("kernel", KERNELS)
def test_attention_staircase_rescales_by_zero_in_every_tile(R, kernel):
    """(b) T = 256: key 64 i + 5 beats everything before it by 512 (i = 0 .. 3), so every tile brings a new maximum and rescales by an exact zero: the output
    is the value of key 197.  (c) the inverse: the maximum in tile 0, every later step 512 lower: p underflows to 0 exactly, the output is the value of key 5."""
    T, H = 256, 2
    g = torch.Generator(device="cuda").manual_seed(7)
    for steps, winner in (((1, 2, 3, 4), 197), ((4, 3, 2, 1), 5)):
        qkv, e = _pointed(T, H, g, kernel)
        for i, c in enumerate(steps):
            qkv[0, 64 * i + 5, 1] = e * (64.0 * c)          # logit 512 c
        out = _attn(R, kernel, qkv, H)
        assert torch.allclose(out, qkv[:, winner:winner + 1, 2].expand(1, T, H, D), rtol=0, atol=1e-30), steps


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("T", [64, 128, 256])
def test_attention_constant_very_negative_logits_give_the_exact_mean(R, kernel, T):
    """(d) all keys identical and q . k * scale = -30 000 for every pair: the softmax is uniform, and with integer values and T a power of two the mean is
    exact.  A kernel that substitutes a finite "minus infinity" for the masked or initial maximum (-1e4, -30 000, ...) fails here."""
    H = 2
    g = torch.Generator(device="cuda").manual_seed(T + 1)
    qkv = torch.zeros(1, T, 3, H, D, device="cuda")
    qkv[0, :, 0, :, 9] = -480.0
    qkv[0, :, 1, :, 9] = 500.0                                  # -480 * 500 / 8 = -30 000; both exact in bf16 and in fp16 (times 2^4: 8 000 < 65 504)
    vi = torch.randint(-8, 9, (1, T, H, D), device="cuda", generator=g).float()
    qkv[:, :, 2] = vi
    out = _attn(R, kernel, qkv, H)
    assert torch.equal(out, vi.mean(dim=1, keepdim=True).expand(1, T, H, D))


@pytest.mark.parametrize("kernel", ["f32", "bf16x3"])
def test_attention_nan_and_inf_stay_where_they_belong(R, kernel):
    """(e) include/vd3d.h: NaN / Inf inputs give NaN.  A NaN (or an Inf: its logits are +-Inf, and Inf - Inf is NaN) in one query row makes exactly that
    query's output of that head NaN; a NaN in one key makes exactly that (batch, head) slab NaN; everything else is bit-identical to the clean run.
    (An Inf in a KEY is not asserted: a logit of -Inf is a legitimate probability 0.)"""
    B, T, H = 2, 77, 3
    g = torch.Generator(device="cuda").manual_seed(51)
    qkv = torch.randn(B, T, 3, H, D, device="cuda", generator=g)
    clean = _attn(R, kernel, qkv, H)
    assert bool(torch.isfinite(clean).all())
    for val in (float("nan"), float("inf"), float("-inf")):
        bad = qkv.clone()
        bad[1, 70, 0, 2, 13] = val                                  # a query of the masked last tile's rows, batch 1, head 2
        out = _attn(R, kernel, bad, H)
        hit = torch.zeros(B, T, H, dtype=torch.bool, device="cuda")
        hit[1, 70, 2] = True
        assert bool(torch.isnan(out[hit]).all()), val
        assert torch.equal(out[~hit], clean[~hit]), val
    for t in (3, 70):                                               # a key of the first tile, one of the masked last tile
        bad = qkv.clone()
        bad[0, t, 1, 1, 40] = float("nan")
        out = _attn(R, kernel, bad, H)
        hit = torch.zeros(B, T, H, dtype=torch.bool, device="cuda")
        hit[0, :, 1] = True
        assert bool(torch.isnan(out[hit]).all()), t
        assert torch.equal(out[~hit], clean[~hit]), t


# ---------------------------------------------------------------------------------------------------------------- a second device
def _second_device_ops():
    def gemm(mode):
        def op(r, dev):
            g = torch.Generator().manual_seed(61)
            x, w, b = torch.randn(300, 256, generator=g), torch.randn(96, 256, generator=g) * 0.05, torch.randn(96, generator=g)
            return r.linear_x3(x.to(dev), r.gemm_x3_pack(w.to(dev), mode), 96, b.to(dev), mode=mode)
        return op

    def conv_x2(r, dev):
        g = torch.Generator().manual_seed(62)
        x, w = torch.randn(1, 32, 20, 40, generator=g), torch.randn(128, 32, 3, 3, generator=g) * 0.1
        return r.conv3x3_x2(x.to(dev).contiguous(memory_format=CL), r.conv3x3_x2_pack(w.to(dev)), 128)

    def attn(kernel):
        def op(r, dev):
            g = torch.Generator().manual_seed(63)
            qkv = torch.randn(2, 77, 3 * 3 * D, generator=g).to(dev)
            return r.attention_f32(qkv, 3, 0.125) if kernel == "f32" else r.attention_x3(qkv, 3, 0.125, mode=kernel)
        return op
    return {"linear_x3-bf16x3": gemm("bf16x3"), "linear_x3-fp16x2": gemm("fp16x2"), "conv3x3_x2": conv_x2,
            "attention_x3-bf16x3": attn("bf16x3"), "attention_x3-fp16x2": attn("fp16x2"), "attention_f32": attn("f32")}


@pytest.mark.parametrize("name", sorted(_second_device_ops()))
def test_on_a_second_device(name):
    """The > 64 KB dynamic-LDS opt-in is a per-device function attribute (csrc/vd3d_kernels.h vd_lds_optin) and every C entry point makes its context's device
    current: one call through Renderer(0), then one through Renderer(1), equal bits.  The pattern of test_conv3x3_x3_on_a_second_device."""
    if torch.cuda.device_count() < 2:
        pytest.skip("only one GPU visible")
    from visiondepth3d_amd.render_3d import Renderer
    op = _second_device_ops()[name]
    outs = []
    for d in (0, 1):
        r = Renderer(d)
        try:
            with torch.cuda.device(d):
                outs.append(op(r, f"cuda:{d}").cpu())
        finally:
            r.close()
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
