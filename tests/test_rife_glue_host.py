"""CPU tests (no GPU) of the restatements that tests/test_hip_rife_glue.py holds the three float32 glue kernels of the interpolation network to, bit for bit
(csrc/vd3d_conv_ifn.hip: k_rife_warp_pack, k_rife_update, k_rife_blend), and of the input families both files share.

The restatements are NumPy float32, one NumPy operation per float32 operation of the kernel, in the kernel's order (the library is built with
-ffp-contract=off, so the device performs exactly these roundings).  Here they are proved against the module's own operations in FLOAT64 -- F.pad to
multiples of 32, rife.backwarp (grid_sample, border, align_corners=True), F.interpolate(align_corners=False), cat, sigmoid -- within a bound DERIVED from the
operation count (below), beside the same chain in float32 on the CPU as a yardstick.  Mutants of the restatement (one deliberate flaw each) must fall outside
that bound on a named case: the inputs discriminate.

The bounds, with u = 2^-24 (the relative error of one float32 rounding), pixels in [0, 1], four weights that sum to 1:
  warp     the fraction f - floorf(f) is exact for f >= 0 and off by <= u / 2 for f < 0; the sample moves by <= u / 2 per axis and the value by as much
           (neighbouring pixels differ by <= 1): u.  A weight is three roundings (1 - a, 1 - b, their product), the tap product a fourth, and the first
           term passes three additions: (4 + 3) u of a sum of terms that is <= 1.                                                       WARP = 8 u
  pack     s = 1: the warp.  s > 1: the halvings are exact, each of the four values passes two additions of sums <= 1: + 2 u.           PACK = 10 u
           mask channel: 2 u |mean| (s > 1), else exact; flow channels: 2 u mean|flow| / s (s > 1; 1 / s is a power of two), else exact.
  update   (d + 0.5) / s - 0.5 and both weights are exact (multiples of 1 / 8 below 2^15); a term is hx * p, the inner sum, hy * (.), the outer sum:
           4 u up(|t|); * s is exact; the add into the state is one rounding of the result.                        UPDATE = 4 u s up(|t|) + u |result|
  blend    two warps weighted m and 1 - m: 8 u; m is the float64 sigmoid rounded once, |v0 - v1| <= 1: u; 1 - m: u; the two products: u of
           v0 m + v1 (1 - m) <= 1; the sum: u.                                                                                          BLEND = 12 u
The float64 chain's own rounding is covered by 2^-40 (relative to the value's scale)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
SLACK64 = 2.0 ** -40
SIZES = [(1, 1), (32, 64), (33, 65), (70, 100)]
BATCH = 3
KINDS = ("random", "integer", "quarter", "minus_2^-30", "on_0", "on_last", "inside_first", "outside_first", "inside_last", "outside_last", "padded_strip",
         "plus_1e30", "minus_1e30")
MUTANTS = ("clamp_image", "edge_pad", "trunc", "no_flow_scale", "no_update_scale", "align_corners", "mask_swapped")


def pad32(n):
    return (n + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------------------------------- the restatements
def _axis(p, f, n, dt, mut):
    """rf_axis: the clamp of f to +-65536 (fmaxf / fminf drop a NaN: it becomes -65536), floorf, the integer add, fraction 0 outside [0, n - 1) and for NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        fc = np.fmin(np.fmax(f, dt(-65536.0)), dt(65536.0))
        fi = np.trunc(fc) if mut == "trunc" else np.floor(fc)
        i = p + fi.astype(np.int64)
        a = np.where((i < 0) | (i >= n - 1) | np.isnan(f), dt(0.0), f - fi).astype(dt)
    i0 = np.clip(i, 0, n - 1)
    return i0, np.minimum(i0 + 1, n - 1), a


def _pixel11(x6, state, dt, mut):
    """rf_pixel11 at every pixel of the padded frame: [N, Hp, Wp, 11] = warped frame 0, warped frame 1, mask, flow."""
    N, _, h, w = x6.shape
    Hp, Wp = pad32(h), pad32(w)
    X = np.pad(x6.astype(dt), ((0, 0), (0, 0), (0, Hp - h), (0, Wp - w)), mode="edge" if mut == "edge_pad" else "constant")   # rf_px: outside h x w reads 0
    if state is None:
        fl, mk = np.zeros((N, Hp, Wp, 4), dt), np.zeros((N, Hp, Wp), dt)
    else:
        assert state.shape == (N, Hp, Wp, 8)
        fl, mk = state[..., :4].astype(dt), state[..., 4].astype(dt)
    ys, xs, nn = np.arange(Hp)[None, :, None], np.arange(Wp)[None, None, :], np.arange(N)[:, None, None]
    nx, ny = (w, h) if mut == "clamp_image" else (Wp, Hp)
    v = np.empty((N, Hp, Wp, 11), dt)
    one = dt(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in (0, 3):
            k = 0 if c0 == 0 else 2
            xa, xb, ax = _axis(xs, fl[..., k], nx, dt, mut)
            ya, yb, ay = _axis(ys, fl[..., k + 1], ny, dt, mut)
            w00, w01, w10, w11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay
            for c in range(c0, c0 + 3):
                P = X[:, c]
                v[..., c] = P[nn, ya, xa] * w00 + P[nn, ya, xb] * w01 + P[nn, yb, xa] * w10 + P[nn, yb, xb] * w11
    v[..., 6] = mk
    v[..., 7:] = fl
    return v


def warp_pack_restated(x6, state, s, dt=np.float32, mut=None):
    """k_rife_warp_pack: x6 [N, 6, h, w], state [N, Hp, Wp, 8] or None -> [N, Hp / s, Wp / s, 16]."""
    v = _pixel11(x6, state, dt, mut)
    if s > 1:
        c, hf = s // 2 - 1, dt(0.5)
        with np.errstate(invalid="ignore", over="ignore"):
            v = hf * (hf * v[:, c::s, c::s] + hf * v[:, c::s, c + 1::s]) + hf * (hf * v[:, c + 1::s, c::s] + hf * v[:, c + 1::s, c + 1::s])
    out = np.zeros(v.shape[:3] + (16,), dt)
    out[..., :7] = v[..., :7]
    with np.errstate(invalid="ignore", over="ignore"):
        out[..., 7:11] = v[..., 7:] if mut == "no_flow_scale" else v[..., 7:] * (dt(1.0) / dt(s))
    return out


def update_restated(t, state, s, first, dt=np.float32, mut=None):
    """k_rife_update: t [N, Hp / s, Wp / s, C >= 5], state [N, Hp, Wp, 8] -> the new state."""
    N, Hp, Wp, _ = state.shape
    rs = dt(1.0) / dt(s)

    def axis(n_out, n_in):
        d = np.arange(n_out).astype(dt)
        sf = d * (dt(n_in - 1) / dt(max(n_out - 1, 1))) if mut == "align_corners" else np.maximum((d + dt(0.5)) * rs - dt(0.5), dt(0.0))
        a = np.minimum(sf.astype(np.int64), n_in - 1)
        lo = (sf - a.astype(dt)).astype(dt)
        return a, np.minimum(a + 1, n_in - 1), lo, (dt(1.0) - lo).astype(dt)
    ya, yb, ly, hy = axis(Hp, Hp // s)
    xa, xb, lx, hx = axis(Wp, Wp // s)
    T = t[..., :5].astype(dt)
    ly, hy, lx, hx = ly[None, :, None, None], hy[None, :, None, None], lx[None, None, :, None], hx[None, None, :, None]
    u = hy * (hx * T[:, ya][:, :, xa] + lx * T[:, ya][:, :, xb]) + ly * (hx * T[:, yb][:, :, xa] + lx * T[:, yb][:, :, xb])
    if mut != "no_update_scale":
        u[..., :4] = u[..., :4] * dt(s)
    out = np.zeros((N, Hp, Wp, 8), dt)
    out[..., :5] = u if first else state[..., :5].astype(dt) + u
    return out


def sigmoid64(x):
    """The float64 sigmoid."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def blend_restated(x6, state, m=None, dt=np.float32, mut=None):
    """k_rife_blend with the sigmoid value m [N, Hp, Wp] given (default: the float64 sigmoid of the mask rounded once): -> [N, 3, h, w]."""
    N, _, h, w = x6.shape
    if m is None:
        m = sigmoid64(state[..., 4])
    m = np.asarray(m).astype(dt)[:, :h, :w]
    v = _pixel11(x6, state, dt, mut)[:, :h, :w]
    if mut == "mask_swapped":
        m = dt(1.0) - m
    out = np.empty((N, 3, h, w), dt)
    for c in range(3):
        out[:, c] = v[..., c] * m + v[..., 3 + c] * (dt(1.0) - m)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- the input families
def make_state(flow, mask):
    """[N, 4, Hp, Wp] flow and [N, Hp, Wp] mask -> the NHWC state [N, Hp, Wp, 8] (channels 5 .. 7 zero)."""
    st = np.zeros(mask.shape + (8,), np.float32)
    st[..., :4] = np.transpose(flow, (0, 2, 3, 1))
    st[..., 4] = mask
    return st


def _plant(rng, kinds, h, w, quarter_only):
    """Flows of the planted kinds, [N, 4, Hp, Wp] float32.  Channels 0, 2 move along x (extent Wp, image w), channels 1, 3 along y."""
    N, _, Hp, Wp = kinds.shape
    flow = np.zeros(kinds.shape, np.float32)
    for ch in range(4):
        n_pad, n_img = (Wp, w) if ch % 2 == 0 else (Hp, h)
        p = (np.arange(Wp)[None, None, :] if ch % 2 == 0 else np.arange(Hp)[None, :, None]) + np.zeros((N, Hp, Wp))
        k = kinds[:, ch]
        quarter = rng.integers(-160, 161, size=k.shape) / 4.0
        strip = n_img - 1 + rng.random(k.shape) * (n_pad - n_img)            # a position in [w - 1, Wp - 1]: the padded strip and its seam
        if quarter_only:
            strip = np.round(strip * 4.0) / 4.0
        val = [quarter if quarter_only else (rng.random(k.shape) * 2 - 1) * 40.0, rng.integers(-40, 41, size=k.shape).astype(np.float64), quarter,
               np.full(k.shape, 0.0 if quarter_only else -2.0 ** -30), -p, n_pad - 1 - p, 1 - p, -1 - p, n_pad - 2 - p, n_pad - p, strip - p,
               np.full(k.shape, 70000.25 if quarter_only else 1e30), np.full(k.shape, -70000.25 if quarter_only else -1e30)]
        for i, v in enumerate(val):
            flow[:, ch] = np.where(k == i, v.astype(np.float32), flow[:, ch])
    return flow


def _kinds(rng, h, w):
    Hp, Wp = pad32(h), pad32(w)
    kinds = rng.integers(0, len(KINDS), size=(BATCH, 4, Hp, Wp))
    strip = KINDS.index("padded_strip")
    if Wp == w:
        kinds[:, 0::2][kinds[:, 0::2] == strip] = 0          # no padded strip along x at this size
    if Hp == h:
        kinds[:, 1::2][kinds[:, 1::2] == strip] = 0
    return kinds


_CACHE = {}


def family(h, w):
    """The general family of one size: x6 [3, 6, h, w] in [0, 1], flow [3, 4, Hp, Wp] of the planted kinds, kinds, a mask in [0, 1] and one in +-4."""
    if ("g", h, w) not in _CACHE:
        rng = np.random.default_rng(1000 * h + w)
        kinds = _kinds(rng, h, w)
        Hp, Wp = pad32(h), pad32(w)
        _CACHE["g", h, w] = dict(x6=rng.random((BATCH, 6, h, w)).astype(np.float32), kinds=kinds, flow=_plant(rng, kinds, h, w, False),
                                 mask=rng.random((BATCH, Hp, Wp)).astype(np.float32), mask4=((rng.random((BATCH, Hp, Wp)) * 2 - 1) * 4).astype(np.float32))
    return _CACHE["g", h, w]


def exact_family(h, w):
    """Pixels k / 16, flows that are multiples of 1 / 4 (+-70000.25 in place of +-1e30), masks from {0, +104, -104} (m exactly 0.5, 1, 0 under any correct expf): every float32
    operation of the three kernels is exact."""
    if ("e", h, w) not in _CACHE:
        rng = np.random.default_rng(7000 * h + w)
        kinds = _kinds(rng, h, w)
        Hp, Wp = pad32(h), pad32(w)
        _CACHE["e", h, w] = dict(x6=(rng.integers(0, 16, size=(BATCH, 6, h, w)) / 16.0).astype(np.float32), kinds=kinds, flow=_plant(rng, kinds, h, w, True),
                                 mask=np.array([0.0, 104.0, -104.0], np.float32)[rng.integers(0, 3, size=(BATCH, Hp, Wp))])
    return _CACHE["e", h, w]


def nonfinite_family(h, w):
    """The general family with three tenths of the flows replaced by NaN, +Inf and -Inf.  No module reference: the contract is the kernel comment's."""
    if ("n", h, w) not in _CACHE:
        g = family(h, w)
        rng = np.random.default_rng(9000 * h + w)
        r = rng.random(g["flow"].shape)
        flow = g["flow"].copy()
        flow[r < 0.1] = np.nan
        flow[(r >= 0.1) & (r < 0.2)] = np.inf
        flow[(r >= 0.2) & (r < 0.3)] = -np.inf
        _CACHE["n", h, w] = dict(x6=g["x6"], flow=flow, mask=g["mask"])
    return _CACHE["n", h, w]


def update_inputs(h, w, s, pitch=8, exact=False):
    """t [3, Hp / s, Wp / s, pitch] (1e30 in channels >= 5) and the five state channels [3, Hp, Wp, 5]: values in [0, 1], or small integers."""
    Hp, Wp = pad32(h), pad32(w)
    rng = np.random.default_rng(31 * h + w + 7 * s)
    t = np.full((BATCH, Hp // s, Wp // s, pitch), 1e30, np.float32)
    if exact:
        t[..., :5] = rng.integers(-8, 9, size=t.shape[:3] + (5,))
        st = rng.integers(-8, 9, size=(BATCH, Hp, Wp, 5)).astype(np.float32)
    else:
        t[..., :5] = rng.random(t.shape[:3] + (5,))
        st = rng.random((BATCH, Hp, Wp, 5)).astype(np.float32)
    state = np.full((BATCH, Hp, Wp, 8), 9.0, np.float32)
    state[..., :5] = st
    return t, state


# ---------------------------------------------------------------------------------------------------------------------------- the module's own chain
def _pad(x6, dtype):
    h, w = x6.shape[2:]
    return F.pad(torch.from_numpy(x6).to(dtype), (0, (-w) % 32, 0, (-h) % 32))


def pack_module(x6, flow, mask, s, dtype):
    """RifeNet.forward's block input: pad, backwarp both frames, cat with the mask, F.interpolate(1 / s) of it and of the flow (* 1 / s): [N, 11, Hp / s, Wp / s]."""
    from visiondepth3d_amd.rife import backwarp
    x = _pad(x6, dtype)
    fl, mk = torch.from_numpy(flow).to(dtype), torch.from_numpy(mask).to(dtype)[:, None]
    cat = torch.cat((backwarp(x[:, :3], fl[:, :2]), backwarp(x[:, 3:], fl[:, 2:4]), mk), 1)
    kw = dict(scale_factor=1.0 / s, mode="bilinear", align_corners=False, recompute_scale_factor=False)
    return torch.cat((F.interpolate(cat, **kw), F.interpolate(fl, **kw) * (1.0 / s)), 1)


def update_module(t, state, s, first, dtype):
    tt = torch.from_numpy(t[..., :5]).permute(0, 3, 1, 2).to(dtype)
    up = F.interpolate(tt, scale_factor=float(s), mode="bilinear", align_corners=False, recompute_scale_factor=False)
    up = torch.cat((up[:, :4] * float(s), up[:, 4:]), 1)
    return up if first else torch.from_numpy(state[..., :5]).permute(0, 3, 1, 2).to(dtype) + up


def blend_module(x6, flow, mask, dtype):
    from visiondepth3d_amd.rife import backwarp
    h, w = x6.shape[2:]
    x = _pad(x6, dtype)
    fl, mk = torch.from_numpy(flow).to(dtype), torch.sigmoid(torch.from_numpy(mask).to(dtype)[:, None])
    return (backwarp(x[:, :3], fl[:, :2]) * mk + backwarp(x[:, 3:], fl[:, 2:4]) * (1.0 - mk))[:, :, :h, :w]


def _down_abs(a, s):
    """F.interpolate(1 / s) of |a| in float64: the scale of a down-scaled value's rounding error."""
    return F.interpolate(torch.from_numpy(np.abs(a)).double(), scale_factor=1.0 / s, mode="bilinear", align_corners=False, recompute_scale_factor=False).numpy()


def pack_bound(flow, mask, s):
    """The derived per-element bound of warp_pack_restated against the float64 chain, [N, 11, Hp / s, Wp / s]."""
    N, _, Hp, Wp = flow.shape
    b = np.empty((N, 11, Hp // s, Wp // s))
    b[:, :6] = (8 + 2 * (s > 1)) * U + SLACK64
    b[:, 6:7] = (2 * U * (s > 1) + SLACK64) * _down_abs(mask[:, None], s) + SLACK64
    b[:, 7:] = (2 * U * (s > 1) + SLACK64) * _down_abs(flow, s) / s + SLACK64
    return b


def update_bound(t, ref, s):
    up = update_module(np.abs(t), None, s, True, torch.float64).numpy()        # s up(|t|) on the flow channels, up(|t|) on the mask
    return 4 * U * up + U * np.abs(ref) + SLACK64


BLEND_BOUND = 12 * U + SLACK64


def bars(tag, got, ref, yard, scale=None):
    """The project's usual bars against float64, beside the float32 yardstick: max <= max(2.5 x, 2^-21), RMS <= 1.5 x + 1e-9."""
    sc = 1.0 if scale is None else scale
    d, d32 = (np.asarray(got, np.float64) - ref) / sc, (np.asarray(yard, np.float64) - ref) / sc
    e, e32, r, r32 = float(np.abs(d).max()), float(np.abs(d32).max()), float(np.sqrt((d * d).mean())), float(np.sqrt((d32 * d32).mean()))
    print(f"RIFE_GLUE_F64 {tag} max {e:.3e} (f32 cpu {e32:.3e}) rms {r:.3e} (f32 cpu {r32:.3e})")
    assert e <= max(2.5 * e32, 2.0 ** -21), (tag, e, e32)
    assert r <= 1.5 * r32 + 1e-9, (tag, r, r32)
    return e, e32


def _nchw(a):
    return np.transpose(a, (0, 3, 1, 2))


def pack_ratio(g, s, with_state, mut=None):
    flow, mask = (g["flow"], g["mask"]) if with_state else (np.zeros_like(g["flow"]), np.zeros_like(g["mask"]))
    got = _nchw(warp_pack_restated(g["x6"], make_state(flow, mask) if with_state else None, s, mut=mut))
    ref = pack_module(g["x6"], flow, mask, s, torch.float64).numpy()
    return got, ref, float((np.abs(got[:, :11].astype(np.float64) - ref) / pack_bound(flow, mask, s)).max())


# ---------------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("h,w", SIZES)
def test_every_size_holds_every_kind_of_flow(h, w):
    """Per axis: every kind is planted (the padded strip only where the size has one), and it lands where its name says."""
    Hp, Wp = pad32(h), pad32(w)
    for fam in (family(h, w), exact_family(h, w)):
        kinds, flow = fam["kinds"], fam["flow"].astype(np.float64)
        for ch in range(4):
            n_pad, n_img = (Wp, w) if ch % 2 == 0 else (Hp, h)
            p = (np.arange(Wp)[None, None, :] if ch % 2 == 0 else np.arange(Hp)[None, :, None]) + np.zeros((BATCH, Hp, Wp))
            land = p + flow[:, ch]
            for i, name in enumerate(KINDS):
                sel = kinds[:, ch] == i
                if name == "padded_strip" and n_pad == n_img:
                    assert not sel.any()
                    continue
                assert int(sel.sum()) >= 8, (name, ch, int(sel.sum()))
                want = {"on_0": 0, "on_last": n_pad - 1, "inside_first": 1, "outside_first": -1, "inside_last": n_pad - 2, "outside_last": n_pad}.get(name)
                if want is not None:
                    assert bool((land[sel] == want).all()), name
                if name == "padded_strip":
                    assert bool(((land[sel] >= n_img - 1) & (land[sel] <= n_pad - 1)).all()) and bool((land[sel] > n_img).any())
                if name in ("integer", "quarter"):
                    assert bool((flow[:, ch][sel] * 4 == np.round(flow[:, ch][sel] * 4)).all())
                    assert bool((flow[:, ch][sel] < 0).any()) and bool((flow[:, ch][sel] > 0).any())
            assert bool((np.abs(flow[:, ch][kinds[:, ch] == KINDS.index("plus_1e30")]) > 65536).all())
        if fam is not exact_family(h, w):
            q = flow[kinds == KINDS.index("quarter")]
            assert bool(((q < 0) & (q != np.floor(q))).any())                  # a negative non-integer: floorf differs from truncation
            assert bool((flow[kinds == KINDS.index("minus_2^-30")] == -2.0 ** -30).all())
    nf = nonfinite_family(h, w)["flow"]
    assert min(int(np.isnan(nf).sum()), int(np.isposinf(nf).sum()), int(np.isneginf(nf).sum())) >= 100


@pytest.mark.parametrize("with_state", [True, False])
@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("h,w", SIZES)
def test_warp_pack_restated_is_within_the_derived_bound_of_the_float64_module(h, w, s, with_state, record_property):
    g = family(h, w)
    got, ref, ratio = pack_ratio(g, s, with_state)
    assert bool((got[:, 11:] == 0).all())
    flow, mask = (g["flow"], g["mask"]) if with_state else (np.zeros_like(g["flow"]), np.zeros_like(g["mask"]))
    yard = pack_module(g["x6"], flow, mask, s, torch.float32).numpy()
    sc = np.ones_like(ref)
    sc[:, 7:] = np.maximum(1.0, _down_abs(flow, s) / s)                         # the flow channels on the image channels' scale
    e, e32 = bars(f"pack {h}x{w} s{s} state{int(with_state)} bound-ratio {ratio:.3f}", got[:, :11], ref, yard, sc)
    record_property("pack", dict(ratio=ratio, e=e, e32=e32))
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("h,w", SIZES)
def test_update_restated_is_within_the_derived_bound_of_the_float64_module(h, w, s, first, record_property):
    t, state = update_inputs(h, w, s)
    got = update_restated(t, state, s, first)
    assert bool((got[..., 5:] == 0).all())
    ref = update_module(t, state, s, first, torch.float64).numpy()
    ratio = float((np.abs(_nchw(got)[:, :5].astype(np.float64) - ref) / update_bound(t, ref, s)).max())
    e, e32 = bars(f"update {h}x{w} s{s} first{int(first)} bound-ratio {ratio:.3f}", _nchw(got)[:, :5], ref, update_module(t, state, s, first, torch.float32).numpy())
    record_property("update", dict(ratio=ratio, e=e, e32=e32))
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("h,w", SIZES)
def test_blend_restated_is_within_the_derived_bound_of_the_float64_module(h, w, record_property):
    g = family(h, w)
    got = blend_restated(g["x6"], make_state(g["flow"], g["mask4"]))
    ref = blend_module(g["x6"], g["flow"], g["mask4"], torch.float64).numpy()
    ratio = float(np.abs(got.astype(np.float64) - ref).max() / BLEND_BOUND)
    e, e32 = bars(f"blend {h}x{w} bound-ratio {ratio:.3f}", got, ref, blend_module(g["x6"], g["flow"], g["mask4"], torch.float32).numpy())
    record_property("blend", dict(ratio=ratio, e=e, e32=e32))
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("h,w", SIZES)
def test_exact_family_float32_equals_float64_bit_for_bit(h, w):
    """On the exact family every float32 operation of the restatements is exact: the float64 evaluation of the same formulas gives the same numbers, and
    they equal the float64 module chain as well (its grid arithmetic moves a sample by ~1e-14, a value by as much)."""
    g = exact_family(h, w)
    st = make_state(g["flow"], g["mask"])
    m = sigmoid64(g["mask"]).astype(np.float32)
    assert set(np.unique(m)) == {0.0, 0.5, 1.0}
    for s in (1, 2, 4):
        for state in (st, None):
            a, b = warp_pack_restated(g["x6"], state, s), warp_pack_restated(g["x6"], state, s, dt=np.float64)
            assert np.array_equal(a.astype(np.float64), b)
        ref = pack_module(g["x6"], g["flow"], g["mask"], s, torch.float64).numpy()
        got = _nchw(warp_pack_restated(g["x6"], st, s))[:, :11].astype(np.float64)
        assert float(np.abs(got[:, :7] - ref[:, :7]).max()) <= SLACK64 * 128
        for first in (False, True):
            t, state = update_inputs(h, w, s, exact=True)
            state[..., :4] = st[..., :4]
            a, b = update_restated(t, state, s, first), update_restated(t, state, s, first, dt=np.float64)
            assert np.array_equal(a.astype(np.float64), b)
            assert np.array_equal(_nchw(a)[:, :5].astype(np.float64), update_module(t, state, s, first, torch.float64).numpy())
    a, b = blend_restated(g["x6"], st, m), blend_restated(g["x6"], st, m, dt=np.float64)
    assert np.array_equal(a.astype(np.float64), b)
    assert float(np.abs(b - blend_module(g["x6"], g["flow"], g["mask"], torch.float64).numpy()).max()) <= SLACK64 * 128


# the named case of each mutant: (kernel, h, w, s)
MUTANT_CASES = {"clamp_image": [("pack", 33, 65, 1), ("blend", 70, 100, 1)], "edge_pad": [("pack", 33, 65, 1), ("pack", 1, 1, 4), ("blend", 70, 100, 1)],
                "trunc": [("pack", 32, 64, 1), ("blend", 32, 64, 1)], "no_flow_scale": [("pack", 32, 64, 2), ("pack", 33, 65, 4)],
                "no_update_scale": [("update", 32, 64, 2), ("update", 33, 65, 4)], "align_corners": [("update", 32, 64, 2), ("update", 1, 1, 4)],
                "mask_swapped": [("blend", 32, 64, 1), ("blend", 33, 65, 1)]}


def mutant_ratio(mut, kernel, h, w, s):
    g = family(h, w)
    if kernel == "pack":
        return pack_ratio(g, s, True, mut)[2]
    if kernel == "blend":
        got = blend_restated(g["x6"], make_state(g["flow"], g["mask4"]), mut=mut)
        return float(np.abs(got.astype(np.float64) - blend_module(g["x6"], g["flow"], g["mask4"], torch.float64).numpy()).max() / BLEND_BOUND)
    t, state = update_inputs(h, w, s)
    ref = update_module(t, state, s, False, torch.float64).numpy()
    return float((np.abs(_nchw(update_restated(t, state, s, False, mut=mut))[:, :5].astype(np.float64) - ref) / update_bound(t, ref, s)).max())


@pytest.mark.parametrize("mut", MUTANTS)
def test_each_mutant_falls_outside_the_bound(mut, record_property):
    """One deliberate flaw each -- the clamp to w - 1 / h - 1, edge-repeating padding, truncation for floorf, flow / s dropped, * s dropped, align_corners=True
    geometry, mask and 1 - mask swapped: outside the derived bound on every named case, while the restatement itself is inside on the same inputs."""
    assert set(MUTANT_CASES) == set(MUTANTS)
    for kernel, h, w, s in MUTANT_CASES[mut]:
        r, r0 = mutant_ratio(mut, kernel, h, w, s), mutant_ratio(None, kernel, h, w, s)
        print(f"RIFE_GLUE_MUTANT {mut} {kernel} {h}x{w} s{s}: {r:.3e} x the bound (restatement {r0:.3f} x)")
        record_property(f"{mut}_{kernel}_{h}x{w}_s{s}", r)
        assert r0 <= 1.0 < r, (mut, kernel, h, w, s, r, r0)


@pytest.mark.parametrize("h,w", [(1, 1), (33, 65)])
def test_nonfinite_flows_read_the_border_pixel(h, w):
    """The kernel comment's contract, on the restatement: a NaN or -Inf flow reads the left / top border, +Inf the right / bottom one (of the PADDED frame:
    zero where the frame is padded), and every image channel is finite."""
    Hp, Wp = pad32(h), pad32(w)
    g = family(h, w)
    X = np.pad(g["x6"], ((0, 0), (0, 0), (0, Hp - h), (0, Wp - w)))
    for bad, col in ((np.nan, 0), (-np.inf, 0), (np.inf, Wp - 1)):
        flow = np.zeros((BATCH, 4, Hp, Wp), np.float32)
        flow[:, 0::2] = bad                                                    # x non-finite, y zero: column `col` of the same row
        v = warp_pack_restated(g["x6"], make_state(flow, g["mask"]), 1)
        assert np.array_equal(_nchw(v)[:, :6], np.broadcast_to(X[:, :, :, col:col + 1], X.shape))
        flow = np.zeros((BATCH, 4, Hp, Wp), np.float32)
        flow[:, 1::2] = bad
        row = 0 if col == 0 else Hp - 1
        out = blend_restated(g["x6"], make_state(flow, g["mask4"]))
        m = sigmoid64(g["mask4"]).astype(np.float32)[:, None, :h, :w]
        Xr = np.broadcast_to(X[:, :, row:row + 1, :], X.shape)[:, :, :h, :w]
        assert np.array_equal(out, Xr[:, :3] * m + Xr[:, 3:] * (np.float32(1) - m))
    nf = nonfinite_family(h, w)
    st = make_state(nf["flow"], nf["mask"])
    for s in (1, 2, 4):
        assert bool(np.isfinite(warp_pack_restated(nf["x6"], st, s)[..., :7]).all())
    assert bool(np.isfinite(blend_restated(nf["x6"], st)).all())
