"""Exact-arithmetic expectations for the fp16 up-scale convolutions (vd3d_conv.hip, vd3d_conv_rdb.hip): data, reference and epilogues.  No tests in here.

The kernels take fp16 operands and accumulate in float32.  With small INTEGER operands (x in [-3, 3], w in [-2, 2]) every product and every partial sum is
an integer below 2^24 (|acc| <= 9 * C_in * 6: 3 456 at 64 channels, 10 368 at 192), so the float32 accumulator is exact in ANY summation order and the
expected result needs no convolution library: a float64 sum converted exactly to float32, then the epilogue's float32 operations one at a time in numpy,
then one round-to-nearest-even to fp16 -- compared on bits.  Power-of-two scalings (``SCALES``) keep all of that exact and move the results to the edges
of the fp16 range.

tests/test_upscale_exact_host.py checks this file on the CPU (the reference against ATen's float64 convolution, the exactness preconditions of every data
set, the epilogue against the module graph's float32 evaluation, the launch policy); tests/test_hip_upscale_exact.py uses it on the GPU."""
import numpy as np
import torch

# name -> (exponent of x, exponent of w): operands are integer * 2^e, still exact in fp16; the accumulator is integer * 2^(ex + ew)
SCALES = {
    "unit": (0, 0),
    "subnormal-out": (-12, -12),    # acc = n * 2^-24, |n| < 1024: every non-zero output is an fp16 subnormal, exactly representable
    "subnormal-in": (-24, 0),       # the same outputs from fp16-SUBNORMAL inputs
    "overflow": (6, 4),             # acc = n * 2^10: |n| >= 64 leaves the fp16 range and must come out as +-inf, the rest exactly
}
X_RANGE, W_RANGE, HEAD_X_RANGE = (-3, 3), (-2, 2), (0, 3)
# every (C_in, x range) x SCALES combination the GPU tests draw from (the host test checks the exactness preconditions of each)
DATASETS = [(3, HEAD_X_RANGE), (64, X_RANGE), (96, X_RANGE), (128, X_RANGE), (160, X_RANGE), (192, X_RANGE)]


def acc_bound(cin, x_range=X_RANGE, w_range=W_RANGE):
    """Largest |integer accumulator| 9 taps x C_in channels can reach."""
    return 9 * cin * max(abs(x_range[0]), abs(x_range[1])) * max(abs(w_range[0]), abs(w_range[1]))


def int_data(H, W, cin, cout, seed, x_range=X_RANGE, scale="unit", device=None):
    """(x, w): x fp16 [H, W, cin] (NHWC without the batch; on ``device`` if given), w fp16 [cout, cin, 3, 3] on the host; integers from a seeded host
    generator, dense (asymmetric in every index, so a swapped tap, channel or fragment lane shows), times the power of two of ``scale``."""
    gen = torch.Generator().manual_seed(seed)
    ex, ew = SCALES[scale]
    xi = torch.randint(x_range[0], x_range[1] + 1, (H, W, cin), generator=gen, dtype=torch.int8)
    wi = torch.randint(W_RANGE[0], W_RANGE[1] + 1, (cout, cin, 3, 3), generator=gen, dtype=torch.int8)
    if device is not None:
        xi = xi.to(device)
    return (xi.float() * 2.0 ** ex).half(), (wi.float() * 2.0 ** ew).half()


def nchw(x_hwc):
    """[H, W, C] -> the [1, C, H, W] channels_last view of the same memory (what the Renderer methods take)."""
    return x_hwc.permute(2, 0, 1)[None]


def hwc(t_nchw):
    """[1, C, H, W] (channels_last or a channel slice of it) -> contiguous [H, W, C]."""
    return t_nchw[0].permute(1, 2, 0).contiguous()


def bits(t):
    """fp16 tensor -> its bit patterns (numpy int16, on the host)."""
    return t.contiguous().cpu().numpy().view(np.int16)


def ref_acc64(x, w, up2=False):
    """The accumulator of a 3x3 / stride 1 / zero padding 1 convolution in float64, as nine shifted matmuls (no convolution is called): x [H, W, C_in],
    w [C_out, C_in, 3, 3] -> [H, W, C_out] (with ``up2``: x is up-sampled nearest x2 first, [2H, 2W, C_out]).  Runs on x's device."""
    x = x.double()
    w = w.double().to(x.device)
    if up2:
        x = x.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
    H, W, C = (int(s) for s in x.shape)
    xp = torch.zeros((H + 2, W + 2, C), dtype=torch.float64, device=x.device)
    xp[1:H + 1, 1:W + 1] = x
    acc = torch.zeros((H * W, int(w.shape[0])), dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            acc += xp[kh:kh + H, kw:kw + W].reshape(H * W, C) @ w[:, :, kh, kw].t()
    return acc.view(H, W, -1)


def _acc32(acc):
    if isinstance(acc, torch.Tensor):          # narrowed where it lives (a third of the bytes to move), checked the same way
        a32 = acc.float()
        assert torch.equal(a32.double(), acc), "the accumulator is not exact in float32: the data breaks the precondition"
        return a32.cpu().numpy()
    a64 = np.asarray(acc)
    a32 = a64.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a64), "the accumulator is not exact in float32: the data breaks the precondition"
    return a32


def _leaky(v, slope):
    return np.where(v >= 0, v, v * slope)      # v >= 0 ? v : v * slope  (NaN takes the product, like the kernels' comparison)


def _f16(v):
    assert v.dtype == np.float32
    with np.errstate(over="ignore"):
        return v.astype(np.float16)            # one round-to-nearest-even; beyond 65 504 (+ half an ULP): +-inf


def expect_c64(acc, bias, slope=None):
    """Epilogue of k_conv3x3_c64 / k_conv3x3_c64_s: acc [H, W, 64] float64 (exact), bias float32 [64], slope float32 [64] or None -> fp16 [H, W, 64]."""
    v = _acc32(acc)
    v = v + np.asarray(bias, dtype=np.float32)
    if slope is not None:
        v = _leaky(v, np.asarray(slope, dtype=np.float32))
    return _f16(v)


def expect_head(acc, bias, slope=None):
    """Epilogue of k_conv3x3_head: the same two float32 operations and one fp16 rounding."""
    return expect_c64(acc, bias, slope)


def expect_dense(acc, bias, slope=1.0, r1=None, alpha=1.0, r2=None, beta=1.0):
    """Epilogue of k_conv3x3_dense_f16: slope, alpha, beta scalars; r1, r2 fp16 [H, W, C_out] or None.  Every line is one float32 operation."""
    v = _acc32(acc)
    v = v + np.asarray(bias, dtype=np.float32)
    v = _leaky(v, np.float32(slope))
    if r1 is not None:
        v = v * np.float32(alpha)
        v = v + np.asarray(r1).astype(np.float32)
    if r2 is not None:
        v = v * np.float32(beta)
        v = v + np.asarray(r2).astype(np.float32)
    return _f16(v)


# The launch policy of vd_launch_conv3x3_c64_f16 (vd3d_conv.hip), restated.  When the policy there changes, the regime assertions of
# tests/test_hip_upscale_exact.py and tests/test_upscale_exact_host.py fail, and the shapes of the c64 cases must be chosen again from the new policy.
C64_TW, C64_TH_S, C64_TH, C64_SWITCH = 32, 8, 16, 4096


def c64_slots(n_cu):
    s = 3 * n_cu
    return s - s % 8


def c64_regime(H, W, n_cu):
    """(regime, ntiles, per, rounds): "one-round" -- the 32 x 8 kernel, every workgroup one tile; "persistent" -- the 32 x 8 kernel, 3 * n_cu (rounded down
    to 8) workgroups walk ``per`` tiles per XCD band in ``rounds`` rounds; "tile16" -- the 32 x 16 kernel, one tile per workgroup (per 0, rounds 1)."""
    ntx = -(-W // C64_TW)
    nt8 = ntx * -(-H // C64_TH_S)
    slots = c64_slots(n_cu)
    if nt8 <= C64_SWITCH and slots >= 8:
        per = -(-nt8 // 8)
        if nt8 <= slots:
            return "one-round", nt8, per, 1
        return "persistent", nt8, per, -(-per // (slots // 8))
    return "tile16", ntx * -(-H // C64_TH), 0, 1
