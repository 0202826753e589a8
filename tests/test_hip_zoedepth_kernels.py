"""GPU tests (-m gpu) of the four kernels of csrc/vd3d_zoedepth.hip alone, through the C entry points (Renderer's thin wrappers): the padded front end and the
un-padding post-process against their torch statements within derived bounds (zoedepth_cases.front_end_bound / bicubic_bound state the derivations), the attractor
step bit for bit against its NumPy float32 statement, and the log-binomial tail against the float64 statement under the project's bar for composed float32 kernels
(tests/test_hip_depth_pro_head_poly.py): error <= max(2.5 x the float32 CPU module's error against the same float64, 2^-21), relative to the magnitude scale."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import zoedepth_cases as cases   # noqa: E402

HALF = (0.5, 0.5, 0.5)


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def table():
    from visiondepth3d_amd import zoedepth
    return zoedepth.rescale_table()


# ---------------------------------------------------------------------------------------------------------------- front end
# (H, W, target): the smallest legal frame (pad 4 on a side of 5), two odd frames, a frame whose padded height IS the target height (that axis is the identity:
# 20 + 2 * 9 = 38), an up-scaled one; the outputs span one to several hundred workgroups
@pytest.mark.parametrize("H,W,target", [(5, 5, (32, 32)), (37, 53, (64, 96)), (270, 481, (96, 160)), (20, 30, (38, 64)), (24, 32, (96, 128))])
def test_preprocess_is_the_processor(R, table, H, W, target):
    from visiondepth3d_amd import zoedepth
    fr = cases.frames(2, H, W, 100 + H + W)
    ph, pw = zoedepth.pad_amounts(H, W)
    proc = dict(zoedepth.PROCESSOR)
    ref = zoedepth.preprocess_statement(fr, proc, target=target)
    got = R.zoedepth_preprocess(fr.cuda(), (ph, pw), target, HALF, HALF, table.cuda())
    assert got.shape == ref.shape == (2, 3, *target) and got.is_contiguous(memory_format=torch.channels_last)
    lim = cases.front_end_bound(H + 2 * ph, W + 2 * pw)
    d = float((got.cpu() - ref).abs().max())
    print("ZOE_PREPROCESS", dict(H=H, W=W, pad=(ph, pw), target=target, max_diff=d, bound=lim, exact=float((got.cpu() == ref).float().mean())))
    assert d <= lim
    assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0


def test_preprocess_spreads_a_nan_of_the_table_to_the_pixels_that_tap_it(R, table):
    """A NaN entry of the byte table reaches exactly the output pixels whose four taps (zero weights included) read that byte, as in ATen."""
    from visiondepth3d_amd import zoedepth
    fr = cases.frames(1, 37, 53, 3)
    fr[0, 10, 20] = 201
    tab = table.clone()
    tab[201] = float("nan")
    ph, pw = zoedepth.pad_amounts(37, 53)
    ref = zoedepth.preprocess_statement(fr, dict(zoedepth.PROCESSOR), table=tab, target=(64, 96))
    got = R.zoedepth_preprocess(fr.cuda(), (ph, pw), (64, 96), HALF, HALF, tab.cuda()).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and 0 < int(torch.isnan(got).sum()) < got.numel()


# ---------------------------------------------------------------------------------------------------------------- post-process
def _pred(B, th, tw, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:th, 0:tw]
    return torch.from_numpy((0.5 + 9.0 * ((y * 3 + x * 5) % (th + tw)) / (th + tw) + rng.uniform(0, 0.5, (B, th, tw))).astype(np.float32))


@pytest.mark.parametrize("H,W", [(45, 61), (135, 241), (17, 23)])
@pytest.mark.parametrize("th,tw", [(24, 32), (48, 64)])
def test_post_process_is_the_processors(R, th, tw, H, W):
    """Against post_process_depth_estimation restated in torch on the CPU (zoedepth.post_statement IS that restatement: asserted), B = 2; 17 x 23 is smaller than
    either prediction.  Bound: zoedepth_cases.bicubic_bound with the local magnitude and range."""
    from visiondepth3d_amd import zoedepth
    pred = _pred(2, th, tw, th + H)
    ref = torch.stack(cases.post_process_in_torch(pred, [(H, W)] * 2))
    assert torch.equal(zoedepth.post_statement(pred, H, W), ref)
    ph, pw = zoedepth.pad_amounts(H, W)
    got = R.zoedepth_post(pred.cuda(), H, W, (ph, pw)).cpu()
    assert got.shape == ref.shape == (2, H, W)
    A, D = cases.bicubic_local(pred, H, W, ph, pw)
    lim = cases.bicubic_bound(A, th, tw, D)
    d = (got - ref).abs().double()
    print("ZOE_POST", dict(pred=(th, tw), out=(H, W), pad=(ph, pw), max_diff=float(d.max()), max_ratio_to_bound=float((d / lim).max()),
                           exact=float((got == ref).float().mean())))
    assert bool((d <= lim).all())


def test_post_process_spreads_nan_exactly_as_aten(R):
    from visiondepth3d_amd import zoedepth
    pred = _pred(1, 24, 32, 5)
    pred[0, 12, 12] = float("nan")
    ref = zoedepth.post_statement(pred, 45, 61)
    got = R.zoedepth_post(pred.cuda(), 45, 61, zoedepth.pad_amounts(45, 61)).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and 1 < int(torch.isnan(got).sum()) < got.numel()
    assert bool(torch.isfinite(got[~torch.isnan(got)]).all())


# ---------------------------------------------------------------------------------------------------------------- the attractor step
# (h, w, hp, wp): odd sizes, equal input and output size, a 1 x 1 previous map, and a map of several workgroups
GEOMETRIES = [(7, 11, 4, 6), (9, 13, 9, 13), (5, 7, 1, 1), (24, 40, 12, 20)]


@pytest.mark.parametrize("kind", ["mean", "sum"])
@pytest.mark.parametrize("nb", [20, 64])
@pytest.mark.parametrize("nA", [1, 4, 16])
def test_attractor_is_its_numpy_statement_bit_for_bit(R, nA, nb, kind):
    rng = np.random.Generator(np.random.PCG64(nA * 100 + nb))
    for h, w, hp, wp in GEOMETRIES:
        att = rng.uniform(0.0, 3.0, (2, h, w, nA)).astype(np.float32)
        prev = rng.uniform(0.0, 3.0, (2, hp, wp, nb)).astype(np.float32)
        att[0, 0, 0, 0] = prev[0, 0, 0, 0]   # dx == 0 on one element
        ref = cases.attractor_numpy(att, prev, kind)
        got = R.zoedepth_attractor(torch.from_numpy(att).cuda(), torch.from_numpy(prev).cuda(), kind).cpu().numpy()
        assert got.shape == ref.shape == (2, h, w, nb)
        assert np.array_equal(got, ref), (h, w, hp, wp, float(np.abs(got - ref).max()))


# ---------------------------------------------------------------------------------------------------------------- the log-binomial tail
def _composed(d, dtype, device="cpu"):
    """The kernel's operands from the planted module: w1 split into its ``last`` columns, the relative-depth column and the embedding columns; the module's table."""
    from transformers.models.zoedepth.modeling_zoedepth import log_binom
    clb, cl = d["clb"], d["cl"]
    w1 = clb.mlp[0].weight.detach()[:, :, 0, 0]
    lbt = clb.log_binomial_transform
    c = lambda t: t.detach().to(device, dtype).contiguous()   # noqa: E731
    return dict(w1_last=c(w1[:, :32]), wrel=c(w1[:, 32]) if cl > 32 else None, w1_e=c(w1[:, cl:]), b1=c(clb.mlp[0].bias), w2=c(clb.mlp[2].weight[:, :, 0, 0]),
                b2=c(clb.mlp[2].bias), table=log_binom(lbt.k_minus_1, lbt.k_idx).reshape(-1).to(device))


@pytest.mark.parametrize("with_rel", [False, True], ids=["no-rel", "rel"])
@pytest.mark.parametrize("nb", [20, 64])
@pytest.mark.parametrize("H,W,hc,wc", [(24, 40, 12, 20), (9, 13, 5, 7)])
def test_bins_tail_against_the_float64_statement(R, H, W, hc, wc, nb, with_rel):
    from visiondepth3d_amd import zoedepth
    d = cases.planted_tail(2, H, W, hc, wc, nb, with_rel, seed=H + nb)
    lo, hi = d["min_temp"], d["max_temp"]
    # the float64 statement (the composed form) and what it alone shows of the planted branches
    w = _composed(d, torch.float64)
    c64 = lambda t: None if t is None else t.double()   # noqa: E731
    P64 = torch.einsum("ce,behw->bchw", w["w1_e"], d["e"].double())
    st = zoedepth.bins_statement(c64(d["last"]), c64(d["rel"]), w["wrel"], P64, c64(d["bins"]), w["w1_last"], w["b1"], w["w2"], w["b2"], w["table"], lo, hi)
    hid = torch.einsum("ck,bkhw->bchw", w["w1_last"], d["last"].double()) + zoedepth._up(P64, (H, W)) + w["b1"].view(1, -1, 1, 1)
    if with_rel:
        hid = hid + w["wrel"].view(1, -1, 1, 1) * d["rel"].double().unsqueeze(1)
    arg = torch.einsum("mc,bchw->bmhw", w["w2"], torch.nn.functional.gelu(hid)) + w["b2"].view(1, -1, 1, 1)
    o = torch.nn.functional.softplus(arg) + 1e-4
    p, temp = o[:, 0] / (o[:, 0] + o[:, 1]), (hi - lo) * (o[:, 2] / (o[:, 2] + o[:, 3])) + lo
    shown = dict(temp_low=int((temp < 2 * lo).sum()), temp_high=int((temp > hi / 2).sum()), p_low=int((p < 1e-4).sum()), q_low=int(((1 - p) < 1e-4).sum()),
                 softplus_linear=int((arg > 20).sum()), range_over_mean=float((st.max() - st.min()) / st.mean()))
    assert min(shown["temp_low"], shown["temp_high"], shown["p_low"], shown["q_low"], shown["softplus_linear"]) > 0 and shown["range_over_mean"] >= 0.1, shown
    # the stock module in float64 is the same function, in float32 it is the yardstick
    ref64, scale = cases.tail_in_module(d, torch.float64)
    assert float(((st - ref64).abs() / scale).max()) <= 1e-12
    ref32, _ = cases.tail_in_module(d, torch.float32)
    # the kernel: float32 operands, P = W1_e . e as the route forms it (a float32 1 x 1 convolution)
    g = _composed(d, torch.float32, "cuda")
    nhwc = lambda t: t.cuda().permute(0, 2, 3, 1).contiguous()   # noqa: E731
    P = torch.nn.functional.conv2d(d["e"].cuda(), g["w1_e"][:, :, None, None])
    got = R.zoedepth_bins(nhwc(d["last"]), d["rel"].cuda() if with_rel else None, g["wrel"], nhwc(P), nhwc(d["bins"]), g["w1_last"], g["b1"], g["w2"], g["b2"],
                          g["table"], lo, hi).cpu().double()
    assert got.shape == st.shape == (2, H, W) and bool(torch.isfinite(got).all())

    def err(v):
        return float(((v - st).abs() / scale).max()), float(((v - st) / scale).pow(2).mean().sqrt())
    (e, rms), (e32, rms32) = err(got), err(ref32.double())
    print("ZOE_BINS_ERR", dict(fine=(H, W), coarse=(hc, wc), nb=nb, rel=with_rel, max=e, yardstick_max=e32, rms=rms, yardstick_rms=rms32, **shown))
    assert e <= max(2.5 * e32, 2.0 ** -21), (e, e32)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(R, table):
    """A pad that is not smaller than its side, bin and attractor counts outside what is built, misaligned and overlapping buffers: VD3D_E_UNSUPPORTED with the
    message; the outputs keep their NaNs."""
    from visiondepth3d_amd import _abi
    L, ctx = R._L, R._ctx

    def ptr(t, off=0):
        return C.c_void_p(t.data_ptr() + off)

    def refused(rc, word):
        assert rc == _abi.E_UNSUPPORTED and word in L.vd3d_last_error().decode(), (rc, L.vd3d_last_error())
    out = torch.full((4096,), float("nan"), device="cuda")
    fr = torch.zeros(1, 5, 5, 3, dtype=torch.uint8, device="cuda")
    tab = table.cuda()
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    z = (C.c_float * 3)(0.5, 0.0, 0.5)
    refused(L.vd3d_zoedepth_preprocess_u8(ctx, ptr(fr), ptr(tab), 1, 5, 5, 5, 4, 16, 16, m, m, ptr(out)), "smaller than its side")
    refused(L.vd3d_zoedepth_preprocess_u8(ctx, ptr(fr), ptr(tab), 1, 5, 5, 4, 5, 16, 16, m, m, ptr(out)), "smaller than its side")
    refused(L.vd3d_zoedepth_preprocess_u8(ctx, ptr(fr), ptr(tab), 1, 5, 5, 4, 4, 0, 16, m, m, ptr(out)), "empty shape")
    refused(L.vd3d_zoedepth_preprocess_u8(ctx, ptr(fr), ptr(tab), 1, 5, 5, 4, 4, 16, 16, m, z, ptr(out)), "std[1]")
    refused(L.vd3d_zoedepth_preprocess_u8(ctx, ptr(fr), ptr(tab), 1, 5, 5, 4, 4, 16, 16, m, m, ptr(out, 2)), "4-byte aligned")
    pred = torch.zeros(1, 8, 8, device="cuda")
    refused(L.vd3d_zoedepth_post_f32(ctx, ptr(pred), 1, 8, 8, 0, 8, 1, 1, ptr(out)), "empty shape")
    refused(L.vd3d_zoedepth_post_f32(ctx, ptr(pred), 1, 8, 8, 8, 8, -1, 1, ptr(out)), "negative pad")
    refused(L.vd3d_zoedepth_post_f32(ctx, ptr(pred), 1, 8, 8, 4, 4, 1, 1, ptr(pred, 16)), "overlaps")
    att, prev = torch.zeros(1, 4, 4, 16, device="cuda"), torch.zeros(1, 2, 2, 64, device="cuda")
    refused(L.vd3d_zoedepth_attractor_f32(ctx, ptr(att), ptr(prev), 1, 4, 4, 2, 2, 17, 20, 1, ptr(out)), "17 attractors")
    refused(L.vd3d_zoedepth_attractor_f32(ctx, ptr(att), ptr(prev), 1, 4, 4, 2, 2, 4, 22, 1, ptr(out)), "22 bins")
    refused(L.vd3d_zoedepth_attractor_f32(ctx, ptr(att), ptr(prev), 1, 4, 4, 2, 2, 4, 260, 1, ptr(out)), "260 bins")
    refused(L.vd3d_zoedepth_attractor_f32(ctx, ptr(att), ptr(prev), 1, 4, 4, 2, 2, 4, 20, 1, ptr(out, 4)), "16-byte aligned")
    refused(L.vd3d_zoedepth_attractor_f32(ctx, ptr(att), ptr(prev), 1, 2, 2, 2, 2, 4, 64, 1, ptr(prev)), "overlaps")
    last, P, bins = torch.zeros(1, 4, 4, 32, device="cuda"), torch.zeros(1, 2, 2, 24, device="cuda"), torch.zeros(1, 2, 2, 20, device="cuda")
    wt = torch.zeros(4096, device="cuda")
    args = lambda Ch, nb, o, lo=0.0212, hi=50.0: (ctx, ptr(last), None, None, ptr(P), ptr(bins), ptr(wt), ptr(wt), ptr(wt), ptr(wt), ptr(wt), lo, hi, 1, 4, 4, 2, 2, Ch, nb, o)   # noqa: E731
    refused(L.vd3d_zoedepth_bins_f32(*args(132, 20, ptr(out))), "132 hidden channels")
    refused(L.vd3d_zoedepth_bins_f32(*args(22, 20, ptr(out))), "22 hidden channels")
    refused(L.vd3d_zoedepth_bins_f32(*args(24, 18, ptr(out))), "18 bins")
    refused(L.vd3d_zoedepth_bins_f32(*args(24, 20, ptr(out), lo=0.0)), "temperatures")
    refused(L.vd3d_zoedepth_bins_f32(*args(24, 20, ptr(out, 2))), "4-byte aligned")
    refused(L.vd3d_zoedepth_bins_f32(*args(24, 20, ptr(last))), "overlaps")
    assert L.vd3d_zoedepth_bins_f32(ctx, ptr(last), ptr(wt), None, ptr(P), ptr(bins), ptr(wt), ptr(wt), ptr(wt), ptr(wt), ptr(wt), 0.0212, 50.0, 1, 4, 4, 2, 2, 24, 20,
                                    ptr(out)) == _abi.E_INVALID   # the plane without its weight column
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and float(pred.abs().max()) == 0.0 and float(prev.abs().max()) == 0.0 and float(last.abs().max()) == 0.0
