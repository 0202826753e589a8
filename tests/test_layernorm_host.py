"""CPU tests (no GPU) of the restatements that tests/test_hip_layernorm.py holds vd3d_add_layernorm (csrc/vd3d_netops.hip, float32 and bf16) to, bit for bit,
and of the cases both files share.

The restatements are NumPy float32, one NumPy operation per float32 operation of the kernel and in its order (the library is built with -ffp-contract=off;
float32 division and sqrtf are correctly rounded): lane l of the row's wave adds (v[2j] + v[2j+1]) over j ascending, its elements at float2 / dword index
l + 64 j; the 64 lane sums go through the xor butterfly (offsets 32, 16, .. 1); mean = sum / (float)cols; the centred squares d * d are added per lane over its
2 NJ elements in order and go through the same butterfly; rstd = 1 / sqrtf(sq / n + eps); (v - mean) * rstd * g + b left to right.  bf16: the sum x + y is
rounded to nearest even (f2bf) and the statistics are those of the ROUNDED sum; the result is rounded once.

Against F.layer_norm in float64 on the same (rounded) operands, per element, with u = 2^-24, NJ = cols / 128, out the float64 result, d = v - mean:
  the mean    a lane's sum is 2 NJ additions deep, the butterfly 6, the division 1: |dmean| <= (2 NJ + 7) u mean|v| =: D;  it shifts every d by as much,
  d           one rounding: u |d|,
  rstd        d * d carries 2 u (d's rounding twice) + 1 u, the sum of squares 2 NJ + 6 roundings, / n, + eps: (2 NJ + 11) u of sq / n + eps (all terms
              positive); the root halves it and rounds, the reciprocal rounds: (NJ + 7.5) u; the shifted mean adds D^2 to the variance: D^2 / (2 (var + eps)),
  the result  * rstd, * g and + b round once each.
  |err| <= |g| rstd D + |out - b| ((NJ + 7.5) u + D^2 / (2 (var + eps)) + 3 u) + u |out|        [+ 2^-8 |out| for the bf16 result's rounding]
(first order; the float64 reference's own rounding, 2^-40 of the same scales, is added).  bf16 carries 8 significand bits, so one rounding to nearest is
off by up to 2^-8 of the value (the counterpart of u = 2^-24 for float32's 24 bits): no correctly rounded bf16 result can hold 2^-9, and the restatement
measures 0.99 x the 2^-8 form.  Mutants of the restatement must fall outside the bound."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
EPS = 1e-6
COLS = (384, 768, 1024)
CASES = ("unit", "low_variance", "constant", "common_offset", "massive", "wide_range", "cancelling", "outlier_gains")
MUTANTS = ("eps_outside", "unbiased", "one_pass", "gamma_layout", "stats_unrounded")
_XOR = [np.arange(64) ^ off for off in (32, 16, 8, 4, 2, 1)]


def bf2f(h):
    """bf16 bits (uint16) -> float32."""
    return (np.asarray(h).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f2bf(f):
    """The kernel's f2bf: round to nearest even on the bits, uint32 arithmetic (it wraps like the device's)."""
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def _wave_sum(v):
    """wave_sum_f on [rows, 64]: the xor butterfly; every lane ends with the same sum (each step adds the same two numbers in both lanes)."""
    for idx in _XOR:
        v = v + v[:, idx]
    return v[:, :1]


def _normalise(s, gamma, beta, eps, mut):
    """The statistics and the result of one wave per row on the float32 values s [rows, cols]; gamma, beta float32 [cols].  Returns float32 [rows, cols]."""
    rows, cols = s.shape
    NJ = cols // 128
    assert cols == NJ * 128
    V = s.reshape(rows, NJ, 64, 2)                       # the element of lane l, step j, half k sits at column 2 (l + 64 j) + k
    n, eps = np.float32(cols), np.float32(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros((rows, 64), np.float32)
        for j in range(NJ):
            acc = acc + (V[:, j, :, 0] + V[:, j, :, 1])
        mean = _wave_sum(acc) / n
        sq = np.zeros((rows, 64), np.float32)
        for j in range(NJ):
            for k in range(2):
                if mut == "one_pass":
                    sq = sq + V[:, j, :, k] * V[:, j, :, k]
                else:
                    d = V[:, j, :, k] - mean
                    sq = sq + d * d
        tot = _wave_sum(sq)
        if mut == "one_pass":
            var = tot / n - mean * mean
        elif mut == "unbiased":
            var = tot / (n - np.float32(1.0))
        else:
            var = tot / n
        rstd = np.float32(1.0) / (np.sqrt(var) + eps) if mut == "eps_outside" else np.float32(1.0) / np.sqrt(var + eps)
        if mut == "gamma_layout":                        # each lane takes ITS 2 NJ consecutive gains, not the ones at its columns
            G, B = (a.reshape(64, NJ, 2).transpose(1, 0, 2)[None] for a in (gamma, beta))
        else:
            G, B = gamma.reshape(1, NJ, 64, 2), beta.reshape(1, NJ, 64, 2)
        out = (V - mean[:, :, None, None]) * rstd[:, :, None, None] * G + B
    return out.reshape(rows, cols).astype(np.float32)


def ln_restated_f32(x, y, gamma, beta, eps, mut=None):
    """k_add_layernorm_f32: float32 [rows, cols] -> (out_sum or None, out_norm)."""
    s = x if y is None else x + y
    return (None if y is None else s), _normalise(s, gamma, beta, eps, mut)


def ln_restated_bf16(x, y, gamma, beta, eps, mut=None):
    """k_add_layernorm: bf16 bits (uint16) [rows, cols] -> (out_sum bits or None, out_norm bits)."""
    if y is None:
        osum, v = None, bf2f(x)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            raw = bf2f(x) + bf2f(y)
        osum = f2bf(raw)
        v = raw if mut == "stats_unrounded" else bf2f(osum)
    return osum, f2bf(_normalise(v, bf2f(gamma), bf2f(beta), eps, mut))


def to_bf16(a):
    """float32 -> bf16 bits, round to nearest even (finite values: the kernel's rule is ATen's)."""
    return f2bf(np.asarray(a, np.float32))


# ---------------------------------------------------------------------------------------------------------------------------- the cases
_CACHE = {}


def case(name, cols, rows=6):
    """(x, y or None, gamma, beta) in float32.  The bf16 tests round each to bf16 first."""
    key = (name, cols, rows)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(CASES.index(name) * 10007 + cols + rows)
    f = np.float32
    gamma, beta = (1 + 0.1 * rng.standard_normal(cols)).astype(f), (0.1 * rng.standard_normal(cols)).astype(f)
    x, y = (2 * rng.standard_normal((rows, cols))).astype(f), rng.standard_normal((rows, cols)).astype(f)
    if name == "low_variance":                           # the variance is about eps
        x, y = (1e-3 * rng.standard_normal((rows, cols))).astype(f), None
    elif name == "constant":                             # the float64 answer is beta
        x, y = np.repeat(np.resize(np.array([0.0, 1.0, -3.7, 1000.3, 1e-3, -65504.0], f), rows)[:, None], cols, 1), None
    elif name == "common_offset":
        x, y = (1000 + rng.uniform(-1, 1, (rows, cols))).astype(f), None
    elif name == "massive":                              # DINOv2's massive channels: three at +-300 among unit values
        x = rng.standard_normal((rows, cols)).astype(f)
        x[:, [7, cols // 2 + 1, cols - 2]] = np.array([300.0, -300.0, 300.0], f) * rng.uniform(0.9, 1.1, (rows, 3)).astype(f)
        y = (0.1 * y).astype(f)
    elif name == "wide_range":
        x, y = (rng.choice([-1.0, 1.0], (rows, cols)) * 2.0 ** rng.uniform(-20, 10, (rows, cols))).astype(f), None
    elif name == "cancelling":                           # x + y is about 1e-3 of x
        x = (3 * rng.standard_normal((rows, cols))).astype(f)
        y = (-x * (1 + 1e-3 * rng.standard_normal((rows, cols)))).astype(f)
    elif name == "outlier_gains":                        # tests/outlier_weights.py: gains of 6 and 0.02
        idx = rng.permutation(cols)
        gamma[idx[:4]] *= f(6.0)
        gamma[idx[4:8]] *= f(0.02)
    _CACHE[key] = (x, y, gamma, beta)
    return _CACHE[key]


def as_bf16(c):
    return tuple(None if a is None else to_bf16(a) for a in c)


# ---------------------------------------------------------------------------------------------------------------------------- reference and bound
def reference(s, gamma, beta, eps=EPS):
    """F.layer_norm in float64 on float32 / widened operands."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
    return torch.nn.functional.layer_norm(t(s), (s.shape[1],), t(gamma), t(beta), eps).numpy()


def bound(s, gamma, beta, ref, bf16_out, eps=EPS):
    """The per-element bound of the module docstring, [rows, cols]."""
    s, g, b = np.asarray(s, np.float64), np.asarray(gamma, np.float64)[None], np.asarray(beta, np.float64)[None]
    NJ = s.shape[1] // 128
    var = s.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    D = (2 * NJ + 7) * U * np.abs(s).mean(1, keepdims=True)
    f32 = np.abs(g) * rstd * D + np.abs(ref - b) * ((NJ + 7.5) * U + D * D / (2 * (var + eps)) + 3 * U) + U * np.abs(ref)
    f32 = f32 + 2.0 ** -40 * (np.abs(g) * rstd * np.abs(s).max(1, keepdims=True) + np.abs(ref) + 1e-30)
    return f32 + 2.0 ** -8 * (np.abs(ref) + f32) if bf16_out else f32


def run_case(name, cols, dtype, mut=None, with_y=True, rows=6):
    """-> (result as float64, float64 reference, bound, out_sum as float32 or None, the float32 operand s)."""
    x, y, gamma, beta = case(name, cols, rows)
    if not with_y:
        y = None
    if dtype == "f32":
        osum, out = ln_restated_f32(x, y, gamma, beta, EPS, mut)
        s, g, b = (x if y is None else x + y), gamma, beta
        outf = out
    else:
        xb, yb, gb, bb = as_bf16((x, y, gamma, beta))
        ob, outb = ln_restated_bf16(xb, yb, gb, bb, EPS, mut)
        osum, g, b, outf = (None if ob is None else bf2f(ob)), bf2f(gb), bf2f(bb), bf2f(outb)
        s = bf2f(xb) if yb is None else bf2f(f2bf(bf2f(xb) + bf2f(yb)))
    ref = reference(s, g, b)
    return outf.astype(np.float64), ref, bound(s, g, b, ref, dtype == "bf16"), osum, s


# ---------------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("name", CASES)
def test_restatement_is_within_the_derived_bound_of_float64_layer_norm(name, cols, dtype, record_property):
    for with_y in (True, False):
        got, ref, bnd, osum, s = run_case(name, cols, dtype, with_y=with_y)
        ratio = float((np.abs(got - ref) / bnd).max())
        x, y, gamma, beta = case(name, cols)
        if dtype == "f32":
            yard = torch.nn.functional.layer_norm(torch.from_numpy(s), (cols,), torch.from_numpy(gamma), torch.from_numpy(beta), EPS).numpy()
            e32 = float(np.abs(yard.astype(np.float64) - ref).max())
        else:
            e32 = float("nan")
        print(f"LN_HOST {name} cols {cols} {dtype} y{int(with_y and y is not None)}: {ratio:.3f} x the bound, max err {float(np.abs(got - ref).max()):.3e} (ATen f32 cpu {e32:.3e})")
        record_property(f"ratio_y{int(with_y)}", ratio)
        assert ratio <= 1.0, (name, cols, dtype, ratio)
        if osum is not None:                              # the sum is ATen's: float32 add, or its bf16 add (rounded once, to nearest even)
            tx, ty = torch.from_numpy(x), torch.from_numpy(y)
            want = (tx + ty) if dtype == "f32" else (tx.to(torch.bfloat16) + ty.to(torch.bfloat16)).float()
            assert np.array_equal(osum.view(np.uint32), want.numpy().view(np.uint32))
    if name == "constant":                                # the last run (y=None): constant rows, whose float64 answer is beta itself
        b = case(name, cols)[3]
        assert np.array_equal(ref, np.broadcast_to((bf2f(to_bf16(b)) if dtype == "bf16" else b).astype(np.float64)[None], ref.shape))


def test_to_bf16_is_atens_rounding():
    a = np.random.default_rng(5).standard_normal(4096).astype(np.float32) * np.float32(3)
    assert np.array_equal(bf2f(to_bf16(a)), torch.from_numpy(a).to(torch.bfloat16).float().numpy())


# the named cases of each mutant: (case, cols, dtype)
MUTANT_CASES = {"eps_outside": [("low_variance", 384, "f32"), ("low_variance", 1024, "bf16")],
                "unbiased": [("unit", 1024, "f32"), ("massive", 384, "f32"), ("unit", 384, "bf16")],
                "one_pass": [("common_offset", 1024, "f32"), ("common_offset", 768, "f32"), ("common_offset", 384, "f32")],
                "gamma_layout": [("outlier_gains", 384, "f32"), ("outlier_gains", 1024, "bf16"), ("unit", 768, "f32")],
                "stats_unrounded": [("unit", 384, "bf16"), ("outlier_gains", 768, "bf16"), ("massive", 1024, "bf16")]}


@pytest.mark.parametrize("mut", MUTANTS)
def test_each_mutant_falls_outside_the_bound(mut, record_property):
    """eps outside the root, the unbiased variance, one-pass E[x^2] - mean^2, lane-major gamma / beta, statistics of the unrounded bf16 sum: each is outside
    the derived bound on every case named for it, where the restatement itself is inside."""
    assert set(MUTANT_CASES) == set(MUTANTS)
    for name, cols, dtype in MUTANT_CASES[mut]:
        got, ref, bnd, _, _ = run_case(name, cols, dtype, mut)
        ok, ref0, bnd0, _, _ = run_case(name, cols, dtype)
        with np.errstate(invalid="ignore"):
            d = np.abs(got - ref) / bnd
        r, r0 = float(np.where(np.isnan(d), np.inf, d).max()), float((np.abs(ok - ref0) / bnd0).max())
        print(f"LN_MUTANT {mut} {name} cols {cols} {dtype}: {r:.3e} x the bound (restatement {r0:.3f} x)")
        record_property(f"{mut}_{name}_{cols}_{dtype}", r)
        assert r0 <= 1.0 < r, (mut, name, cols, dtype, r, r0)
