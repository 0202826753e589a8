"""GPU tests (-m gpu) of DepthPipe(gemm="fp16x2", conv="fp16x2") with and without self_contained=True: the depth leg on the library's own fp16x2 kernels
(vd3d_gemm_x3 / vd3d_attention_x3 in mode fp16x2, vd3d_conv3x3_s1_x2, vd3d_conv3x3_s2_x2) with no vendor-library call.

The set-up of tests/test_hip_self_contained.py: depth-anything-v2-small with synthetic weights at a 9 x 17 patch grid (maps 36 x 68, 18 x 34, 9 x 17 and 5 x 9).
No vendor-library operator is dispatched; conv_routes names every convolution module that runs, none as "library"; the library selection did not run; the
prediction is float32-faithful against the stock module in float64 on the CPU (bars of tests/test_hip_depth_f64.py, which the fp16x2 mode is already held to);
the uint8 plane meets the stock float32 GPU graph's; forwards repeat bit for bit and a frame's prediction does not depend on its batch; the flop count equals
that of gemm="fp16x2", conv=None.  One case under the trained-like weights of tests/outlier_weights.py, where the reassemble projections see the massive
channels directly in this mode.  Without self_contained the size rule (CONV_X2_MIN_TILES tiles per frame) keeps the small maps on the library.

MEASURED on an MI355X (profiles/r18_fp16x2_self_contained.md), as E / E_yardstick and RMS / RMS_yardstick against the bars 2.5 and 1.71: synthetic weights
seed 0 1.04 and 0.95, seed 1 0.98 and 0.95; outlier weights 0.68 and 0.72.  uint8 plane 99.995 - 100 % identical to the stock float32 GPU graph's, no byte off by
more than 1; raw prediction within 1.9e-6 of the range."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
pytest.importorskip("transformers")
F = torch.nn.functional

from test_hip_self_contained import BANNED, FH, FW, NAME, SIZE, _frames   # noqa: E402

K, K_RMS = 2.5, 1.71     # tests/test_hip_depth_f64.py


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _pipe(R, seed, **kw):
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    kw.setdefault("conv", "fp16x2")
    return DepthPipe(NAME, device="cuda", dtype=torch.float32, seed=seed, renderer=R, processor=dict(PROCESSORS["da"], size=SIZE), gemm="fp16x2", **kw)


_CACHE = {}


def _leg(R, seed):
    """Per seed, once: the self-contained fp16x2 pipe, its prediction for the two frames, and the stock module's on the same pixel values -- float64 on the CPU
    (the truth), float32 on the CPU (the yardstick), float32 on the GPU.  Shared by the tests below; they do not modify it."""
    if seed not in _CACHE:
        from transformers import DepthAnythingForDepthEstimation
        from visiondepth3d_amd.depth import build_config, synthetic_weights_
        import torch.cuda.tunable as tn
        flags = (torch.backends.cudnn.benchmark, tn.is_enabled())
        pipe = _pipe(R, seed, self_contained=True)
        flags = (flags, (torch.backends.cudnn.benchmark, tn.is_enabled()))
        frames = _frames(2)
        assert pipe.resize_target(FH, FW) == SIZE
        pred = pipe.infer_bgr_u8(frames, raw=True)
        x = R.depth_preprocess(frames, SIZE[0], SIZE[1], pipe.proc["mean"], pipe.proc["std"]).contiguous()   # NCHW copy of what the pipe's network saw
        stock = DepthAnythingForDepthEstimation(build_config(NAME)).eval()
        synthetic_weights_(stock, seed)
        with torch.no_grad():
            p32 = stock(pixel_values=x.cpu()).predicted_depth
            p32g = stock.cuda()(pixel_values=x).predicted_depth
            p64 = stock.cpu().double()(pixel_values=x.cpu().double()).predicted_depth
        _CACHE[seed] = dict(flags=flags, pipe=pipe, frames=frames, pred=pred, p64=p64, p32=p32, p32g=p32g)
    return _CACHE[seed]


def _u8_stats(pred, exp):
    from visiondepth3d_amd.depth import depth_to_u8
    d = (depth_to_u8(pred).to(torch.int16) - depth_to_u8(exp).to(torch.int16)).abs()
    return dict(exact=float((d == 0).float().mean()), max=int(d.max()), pred_err_of_range=float((pred - exp).abs().max()) / float(exp.max() - exp.min()))


def test_fp16x2_self_contained_forward_dispatches_no_vendor_library_operator(R):
    """The second forward under a TorchDispatchMode: no convolution, matrix product or attention operator of ATen.  conv_routes names the patch embedding, the
    four projections, the two transposed convolutions, the stride-2 convolution, the four fusion projections and all 20 three-by-three convolutions, every one
    as "fp16x2", none as "library".  The library selection did not run and the process-wide switches are as the constructor found them."""
    from torch.utils._python_dispatch import TorchDispatchMode
    leg = _leg(R, 0)
    pipe = leg["pipe"]
    seen = []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with Log():
        pred = pipe.infer_bgr_u8(leg["frames"], raw=True)
    assert len(seen) > 20, seen
    bad = sorted({s for s in seen if BANNED.match(s)})
    assert not bad, bad
    assert torch.equal(pred, leg["pred"])
    routes = pipe.conv_routes
    assert routes and all(v[0] == "fp16x2" for v in routes.values()), routes
    mods = dict(pipe.model.named_modules())
    convs = [n for n, m in mods.items() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)) and "layers.0.residual_layer1" not in n and n != "head.conv3"]
    assert sorted(routes) == sorted(convs), sorted(set(routes) ^ set(convs))    # every convolution module that runs (head.conv3 is inside vd3d_dpt_head_tail_f32)
    k3 = [n for n in convs if isinstance(mods[n], torch.nn.Conv2d) and mods[n].kernel_size == (3, 3) and mods[n].stride == (1, 1)]
    assert len(k3) == 20 and all(routes[n] == ("fp16x2", "self-contained") for n in k3)
    for n, what in (("backbone.embeddings.patch_embeddings.projection", "vd3d_patchify_f32"), ("neck.reassemble_stage.layers.0.projection", "vd3d_gemm_x3"),
                    ("neck.reassemble_stage.layers.3.projection", "vd3d_gemm_x3"), ("neck.reassemble_stage.layers.0.resize", "vd3d_depth_to_space_bias_nhwc_f32"),
                    ("neck.reassemble_stage.layers.1.resize", "vd3d_depth_to_space_bias_nhwc_f32"), ("neck.reassemble_stage.layers.3.resize", "vd3d_conv3x3_s2_x2"),
                    ("neck.fusion_stage.layers.0.projection", "vd3d_gemm_x3"), ("neck.fusion_stage.layers.3.projection", "vd3d_gemm_x3")):
        assert routes[n][0] == "fp16x2" and routes[n][1].startswith("self-contained") and what in routes[n][1], (n, routes[n])
    assert pipe.tuned_gemm is False and pipe.miopen_find is False
    assert leg["flags"][0] == leg["flags"][1]


@pytest.mark.parametrize("seed", [0, 1])
def test_fp16x2_self_contained_is_float32_faithful_against_float64(R, seed):
    """E = max |pred - pred64| / range(pred64) <= 2.5 x the stock float32 CPU module's, RMS <= 1.71 x its (the bars of tests/test_hip_depth_f64.py)."""
    leg = _leg(R, seed)
    p64 = leg["p64"]
    rng = float(p64.max() - p64.min())

    def err(p):
        d = p.detach().double().cpu() - p64
        return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng
    (E, rms), (E32, rms32) = err(leg["pred"]), err(leg["p32"])
    print("SELF_CONTAINED_X2_F64", dict(seed=seed, E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32))
    assert tuple(leg["pred"].shape) == tuple(p64.shape) == (2,) + SIZE and bool(torch.isfinite(leg["pred"]).all())
    assert E <= K * E32, (E, E32)
    assert rms <= K_RMS * rms32, (rms, rms32)


@pytest.mark.parametrize("seed", [0, 1])
def test_fp16x2_self_contained_u8_plane_meets_the_stock_float32_graph(R, seed):
    """depth_to_u8 of the raw prediction against that of the stock float32 graph on the GPU: no byte off by more than 1, >= 99.5 % identical, the raw
    prediction within 1e-4 of the range (the bars test_depth_leg_bf16x3_meets_the_float32_legs_bar_1080p[fp16x2] holds the mode to)."""
    leg = _leg(R, seed)
    st = _u8_stats(leg["pred"], leg["p32g"])
    print("SELF_CONTAINED_X2_U8", seed, st)
    assert st["max"] <= 1 and st["exact"] >= 0.995, st
    assert st["pred_err_of_range"] < 1e-4, st


def test_fp16x2_self_contained_repeats_and_does_not_depend_on_the_batch(R):
    leg = _leg(R, 0)
    pipe = leg["pipe"]
    assert torch.equal(pipe.infer_bgr_u8(leg["frames"], raw=True), leg["pred"])
    f3 = _frames(3)
    one, three = pipe.infer_bgr_u8(f3[:1], raw=True), pipe.infer_bgr_u8(f3, raw=True)
    assert torch.equal(one[0], three[0])
    assert torch.equal(three[:2], leg["pred"])


def test_fp16x2_self_contained_counts_the_library_modes_flops(R):
    leg = _leg(R, 0)
    lib_pipe = _pipe(R, 0, conv=None)
    assert lib_pipe.self_contained is False and lib_pipe.conv is None
    a, b = leg["pipe"].flops_per_frame(FH, FW), lib_pipe.flops_per_frame(FH, FW)
    assert a == b and a > 0, (a, b)


def test_fp16x2_self_contained_under_outlier_weights(R):
    """tests/outlier_weights.py, seed 0, 210 x 378 (the set-up of tests/test_hip_depth_f64.py): massive residual channels reach the reassemble projections'
    fp16x2 GEMMs directly.  The prediction is finite and meets the same float64 bars."""
    import outlier_weights as ow
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    H, W = 210, 378
    pred64, pred32 = ow.reference_predictions(0)
    frames = torch.from_numpy(ow.clip_frames()).cuda()
    pipe = DepthPipe(NAME, device="cuda", dtype=torch.float32, model=ow.stock_model(0, torch.float32), processor=dict(PROCESSORS["da"], size=(H, W)), renderer=R,
                     gemm="fp16x2", conv="fp16x2", self_contained=True)
    pred = pipe.infer_bgr_u8(frames, raw=True)
    assert tuple(pred.shape) == tuple(pred64.shape) and bool(torch.isfinite(pred).all())
    assert all(v[0] == "fp16x2" for v in pipe.conv_routes.values()), pipe.conv_routes
    E, rms = ow.errors_of_range(pred, pred64)
    E32, rms32 = ow.errors_of_range(pred32, pred64)
    print("SELF_CONTAINED_X2_OUTLIER", dict(E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32))
    assert E <= K * E32, (E, E32)
    assert rms <= K_RMS * rms32, (rms, rms32)


def test_conv_fp16x2_without_self_contained_keeps_small_maps_on_the_library(R):
    """conv="fp16x2" alone: the large maps take vd3d_conv3x3_s1_x2, the maps below CONV_X2_MIN_TILES tiles per frame stay library calls and say so; the rule
    reads the map only, so one frame and three frames route alike; the u8 bar holds."""
    from visiondepth3d_amd.depth import CONV_X2_MIN_TILES
    leg = _leg(R, 0)
    pipe = _pipe(R, 0)
    assert pipe.self_contained is False
    pred = pipe.infer_bgr_u8(leg["frames"], raw=True)
    routes = dict(pipe.conv_routes)
    own = [n for n, v in routes.items() if v[0] == "fp16x2"]
    lib = [n for n, v in routes.items() if v[0] == "library"]
    assert own and lib and len(own) + len(lib) == len(routes), routes
    assert all(routes[n][1].startswith("size rule") and f"< {CONV_X2_MIN_TILES}" in routes[n][1] for n in lib), routes
    assert "neck.convs.3" in lib, routes                                  # the 5 x 9 map: one tile
    pipe.infer_bgr_u8(_frames(3)[:1], raw=True)
    assert dict(pipe.conv_routes) == routes                               # the batch size is not read
    st = _u8_stats(pred, leg["p32g"])
    print("CONV_X2_U8", st)
    assert st["max"] <= 1 and st["exact"] >= 0.995, st
    assert st["pred_err_of_range"] < 1e-4, st
