"""GPU tests (-m gpu) of DPT-Hybrid ("MiDaS 3.0", Intel/dpt-hybrid-midas) in DepthPipe: the published configuration at full size with synthetic weights, 384 x 384
(the hybrid embeddings take the configured image size only), two synthetic frames; both pairs of the split modes, with and without self_contained=True.

The yardstick is tests/test_hip_self_contained_dpt.py's: the prediction against the stock module in float64 on the CPU, held to the stock float32 CPU module's own
error against that float64 (maximum error <= 2.5 x, RMS <= 1.71 x); the uint8 plane against the float32 graph on the GPU (no byte off by more than one level,
>= 99.5 % identical).  Under the keyword: no vendor-library operator is dispatched -- none of test_hip_self_contained.BANNED, and no ATen group norm, batch norm
(what WeightStandardizedConv2d runs on every forward) or max-pool either -- conv_routes names every convolution and normalisation that runs, forwards repeat bit for
bit and a frame does not depend on its batch.  The references (_stock: the full-size module in float32 and float64 on the CPU, about 17 s) and the four
pipes are built once and shared; no test modifies them.

No test here can pass on a flat plane: with seed 7 the float64 truth of both frames has >= 128 distinct uint8 levels and under 75 % of its pixels at the ReLU
floor (stock float32 graph on the CPU: 0.4 - 1 % at the floor, >= 251 levels; seed 5, which the DPT-Large tests use, leaves 98 % of this model's plane at zero)."""
import json
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_hip_self_contained import BANNED   # noqa: E402

NAME, SEED, FH, FW = "dpt-hybrid-midas", 7, 252, 476
PAIRS = ("bf16x3", "fp16x2")
PREFIX = "dpt.embeddings.backbone.bit."
# on top of BANNED: what the BiT prefix's module graph dispatches
BANNED_PREFIX = re.compile(r"^aten\.(native_group_norm|group_norm|native_batch_norm|_native_batch_norm_legit|batch_norm|miopen_batch_norm|cudnn_batch_norm|max_pool2d)")


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _frames(n):
    from visiondepth3d_amd import synth
    return torch.from_numpy(np.stack([synth.synth_frame(i, FH, FW)[0] for i in range(n)])).cuda()


def _pipe(R, pair, **kw):
    from visiondepth3d_amd.depth import DepthPipe
    return DepthPipe(NAME, device="cuda", dtype=torch.float32, seed=SEED, renderer=R, gemm=pair, conv=pair, **kw)


def _not_flat(p64):
    from visiondepth3d_amd.depth import depth_to_u8
    st = [(int(torch.unique(depth_to_u8(p64[i:i + 1].float())).numel()), float((p64[i] == 0).double().mean())) for i in range(p64.shape[0])]
    assert all(lv >= 128 and fl < 0.75 for lv, fl in st), st
    return st


_STOCK, _LEGS = {}, {}


def _stock(R):
    """Once: the stock module's predictions for the two frames on the pixel values the pipe's network sees -- float64 on the CPU (the truth), float32 on the CPU (the
    yardstick) and float32 on the GPU.  Shared; not modified."""
    if not _STOCK:
        from transformers import DPTForDepthEstimation
        from visiondepth3d_amd.depth import PROCESSORS, build_config, synthetic_weights_
        frames = _frames(2)
        proc = PROCESSORS["dpt"]
        x = R.depth_preprocess(frames, 384, 384, proc["mean"], proc["std"]).contiguous()
        stock = DPTForDepthEstimation(build_config(NAME)).eval()
        synthetic_weights_(stock, SEED)
        with torch.no_grad():
            p32 = stock(pixel_values=x.cpu()).predicted_depth
            stock.cuda()
            p32g = stock(pixel_values=x).predicted_depth
            stock.cpu().double()
            p64 = stock(pixel_values=x.cpu().double()).predicted_depth
        _STOCK.update(frames=frames, x=x, p64=p64, p32=p32, p32g=p32g, flat=_not_flat(p64))
    return _STOCK


def _leg(R, pair, sc):
    if (pair, sc) not in _LEGS:
        st = _stock(R)
        pipe = _pipe(R, pair, self_contained=sc)
        assert pipe.resize_target(FH, FW) == (384, 384) and pipe.dpt_hybrid and pipe.dpt_vit and pipe.self_contained is sc and pipe.arch == "generic"
        _LEGS[pair, sc] = dict(st, pipe=pipe, pred=pipe.infer_bgr_u8(st["frames"], raw=True))
    return _LEGS[pair, sc]


def _dispatch_log(fn):
    from torch.utils._python_dispatch import TorchDispatchMode
    seen = []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    with Log():
        out = fn()
    return seen, out


def _u8_stats(a, b):
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return dict(exact=float((d == 0).float().mean()), max=int(d.max()))


@pytest.mark.parametrize("sc", [False, True], ids=["library-prefix", "self-contained"])
@pytest.mark.parametrize("pair", PAIRS)
def test_dpt_hybrid_is_float32_faithful_against_float64(R, pair, sc):
    """E = max |pred - pred64| / range(pred64) <= 2.5 x the stock float32 CPU module's, RMS <= 1.71 x its (the bars of tests/test_hip_self_contained_dpt.py)."""
    leg = _leg(R, pair, sc)
    p64 = leg["p64"]
    rng = float(p64.max() - p64.min())

    def err(p):
        d = p.detach().double().cpu() - p64
        return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng
    (E, rms), (E32, rms32) = err(leg["pred"]), err(leg["p32"])
    print("DPT_HYBRID_F64", dict(pair=pair, self_contained=sc, E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32,
                                 levels_floor=leg["flat"]))
    assert tuple(leg["pred"].shape) == tuple(p64.shape) == (2, 384, 384) and bool(torch.isfinite(leg["pred"]).all())
    assert E <= 2.5 * E32, (E, E32)
    assert rms <= 1.71 * rms32, (rms, rms32)


@pytest.mark.parametrize("pair", PAIRS)
def test_dpt_hybrid_self_contained_dispatches_no_vendor_operator_and_names_every_route(R, pair):
    """conv_routes under the keyword: the 52 convolutions and 52 normalisations of the BiT prefix and its pool; the embedding projection; hooks 2 / 3's projections
    and hook 3's stride-2 convolution (hooks 0 / 1 are identities here: DPT-Large's two transposed convolutions and two of its four projections do not exist in
    this model); the four fusion projections; all 20 three-by-three stride-1 convolutions of neck, fusion stage and head that run."""
    leg = _leg(R, pair, True)
    pipe = leg["pipe"]
    assert pipe.tuned_gemm is False and pipe.miopen_find is False
    seen, pred = _dispatch_log(lambda: pipe.infer_bgr_u8(leg["frames"], raw=True))
    assert len(seen) > 20, seen
    bad = sorted({s for s in seen if BANNED.match(s) or BANNED_PREFIX.match(s)})
    assert not bad, bad
    assert torch.equal(pred, leg["pred"])
    routes = pipe.conv_routes
    assert routes and all(v[0] == pair for v in routes.values()), routes
    mods = dict(pipe.model.named_modules())
    convs = [n for n, m in mods.items() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)) and "layers.0.residual_layer1" not in n and n != "head.head.4"]
    norms = [n for n, m in mods.items() if isinstance(m, torch.nn.GroupNorm)]
    assert len(convs) == 52 + 28 and len(norms) == 52 and all(n.startswith(PREFIX) for n in norms)
    assert sorted(routes) == sorted(convs + norms + [PREFIX + "embedder.pooler"]), sorted(set(routes) ^ set(convs + norms))
    s1 = "vd3d_conv3x3_" + R.TILE_CONVS[pair, 1]
    for n, what in ([(PREFIX + "embedder.convolution", "vd3d_im2col_nhwc_f32 + vd3d_gemm_x3"), (PREFIX + "embedder.norm", "vd3d_groupnorm_nhwc_f32"),
                     (PREFIX + "embedder.pooler", "vd3d_maxpool3x3_s2_nhwc_f32"),
                     (PREFIX + "encoder.stages.0.layers.0.downsample.conv", "vd3d_gemm_x3 over the pixel rows"),
                     (PREFIX + "encoder.stages.0.layers.0.conv2", s1), (PREFIX + "encoder.stages.2.layers.8.conv2", s1),
                     (PREFIX + "encoder.stages.1.layers.0.conv2", "vd3d_im2col_nhwc_f32"), (PREFIX + "encoder.stages.2.layers.0.conv2", "vd3d_im2col_nhwc_f32"),
                     (PREFIX + "encoder.stages.1.layers.0.downsample.conv", "vd3d_im2col_nhwc_f32"), (PREFIX + "encoder.stages.2.layers.0.downsample.conv", "vd3d_im2col_nhwc_f32"),
                     (PREFIX + "encoder.stages.2.layers.8.norm3", "vd3d_groupnorm_nhwc_f32 + shortcut + ReLU"),
                     ("dpt.embeddings.projection", "vd3d_gemm_x3 over the pixel rows"),
                     ("neck.reassemble_stage.layers.3.resize", "vd3d_conv3x3_" + R.TILE_CONVS[pair, 2])]
                    + [(f"neck.reassemble_stage.layers.{i}.projection", "vd3d_gemm_x3") for i in (2, 3)]
                    + [(f"neck.fusion_stage.layers.{i}.projection", "vd3d_gemm_x3") for i in range(4)]):
        assert routes[n][0] == pair and what in routes[n][1], (n, routes[n])
    k3 = [n for n in convs if not n.startswith(PREFIX) and mods[n].kernel_size == (3, 3) and mods[n].stride == (1, 1)]
    assert len(k3) == 20 and all(routes[n] == (pair, "self-contained") for n in k3)
    assert sum("vd3d_im2col_nhwc_f32" in v[1] for v in routes.values()) == 5


@pytest.mark.parametrize("pair", PAIRS)
def test_dpt_hybrid_self_contained_repeats_and_does_not_depend_on_the_batch(R, pair):
    leg = _leg(R, pair, True)
    pipe = leg["pipe"]
    assert torch.equal(pipe.infer_bgr_u8(leg["frames"], raw=True), leg["pred"])
    f3 = _frames(3)
    one, three = pipe.infer_bgr_u8(f3[:1], raw=True), pipe.infer_bgr_u8(f3, raw=True)
    assert torch.equal(one[0], three[0])
    assert torch.equal(three[:2], leg["pred"])


@pytest.mark.parametrize("pair", PAIRS)
def test_dpt_hybrid_without_the_keyword_names_the_library_prefix(R, pair):
    """Without self_contained the BiT prefix stays the module graph on the float32 library, and conv_routes says so by module name; the embedding projection is on
    vd3d_gemm_x3 all the same.  The flop count is the same with and without the keyword."""
    leg = _leg(R, pair, False)
    pipe = leg["pipe"]
    routes = pipe.conv_routes
    mods = dict(pipe.model.named_modules())
    prefix = [n for n, m in mods.items() if n.startswith(PREFIX) and isinstance(m, (torch.nn.Conv2d, torch.nn.GroupNorm))]
    assert len(prefix) == 104 and all(routes[n][0] == "library" and "BiT prefix" in routes[n][1] for n in prefix)
    assert routes["dpt.embeddings.projection"] == (pair, "vd3d_gemm_x3 over the pixel rows")
    a, b = _leg(R, pair, True)["pipe"].flops_per_frame(FH, FW), pipe.flops_per_frame(FH, FW)
    assert a == b and a > 0, (a, b)


def test_dpt_hybrid_f32_with_renderer_is_the_stock_graph(R):
    """gemm="f32" with a renderer leaves DPT-Hybrid's module graph as transformers builds it -- no forward replaced, no method patched, the parameters the stock
    model's bit for bit -- and the prediction is the stock model's on the same input to 1e-5 of its range (tests/test_hip_dpt.py's statement for DPT-Large: the
    float32 library kernels do not repeat bit for bit from one model instance to the next)."""
    from transformers import DPTForDepthEstimation
    from visiondepth3d_amd.depth import DepthPipe, build_config, synthetic_weights_
    st = _stock(R)
    pipe = DepthPipe(NAME, device="cuda", dtype=torch.float32, renderer=R, seed=SEED)
    assert pipe.arch == "generic" and pipe.dpt_vit is False and pipe.dpt_hybrid is False and pipe.conv_routes == {}
    assert all("forward" not in m.__dict__ for m in pipe.model.modules())
    assert "_resize_pos_embed" not in pipe.model.dpt.embeddings.__dict__
    stock = DPTForDepthEstimation(build_config(NAME)).eval()
    synthetic_weights_(stock, SEED)
    stock = stock.cuda().float().to(memory_format=torch.channels_last)
    ps, ss = dict(pipe.model.named_parameters()), dict(stock.named_parameters())
    assert ps.keys() == ss.keys() and all(torch.equal(ps[k], ss[k]) for k in ps)
    x = st["x"].contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        got = pipe.model(pixel_values=x).predicted_depth
        exp = stock(pixel_values=x).predicted_depth
    err = float((got - exp).abs().max()) / float(exp.max() - exp.min())
    print("DPT_HYBRID_F32_VS_STOCK", dict(pred_max_err_of_range=err, bit_equal=bool(torch.equal(got, exp))))
    assert err < 1e-5, err
    assert pipe.flops_per_frame(FH, FW) > 0


@pytest.mark.parametrize("sc", [False, True], ids=["library-prefix", "self-contained"])
@pytest.mark.parametrize("pair", PAIRS)
def test_dpt_hybrid_depth_frames_u8_meets_the_float32_pipe(R, pair, sc):
    """depth_frames_u8 (front end, network, hand-off to the frame size) against the float32 pipe's planes: >= 99.5 % of the bytes identical and none off by more
    than one level -- what tests/test_hip_dpt.py requires of DPT-Large in the split modes."""
    from visiondepth3d_amd.depth import DepthPipe
    leg = _leg(R, pair, sc)
    if "u8_f32" not in _STOCK:
        _STOCK["u8_f32"] = DepthPipe(NAME, device="cuda", dtype=torch.float32, renderer=R, seed=SEED).depth_frames_u8(leg["frames"])
    got = leg["pipe"].depth_frames_u8(leg["frames"])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, FH, FW) and int(torch.unique(got).numel()) >= 128
    st = _u8_stats(got, _STOCK["u8_f32"])
    print("DPT_HYBRID_U8", dict(pair=pair, self_contained=sc, **st))
    assert st["exact"] >= 0.995 and st["max"] <= 1, st


def test_from_pretrained_hybrid_folder_reaches_the_self_contained_mode(R, tmp_path):
    """A local DPT-Hybrid checkpoint folder through from_pretrained: a small hybrid in the published geometry (hidden 384, one bottleneck per stage, 64 x 64 input:
    BiT maps 16^2, 8^2 and 4^2, a 4 x 4 patch grid -- GroupNorm over 16 pixels, stride-2 im2col on 16 -> 8 and 8 -> 4) routes to the same rewrite, under the
    keyword too, and computes the stock graph's prediction to the split modes' 1e-4 of its range."""
    import transformers
    from visiondepth3d_amd.depth import DepthPipe, synthetic_weights_
    cfg = transformers.DPTConfig(is_hybrid=True, hidden_size=384, num_hidden_layers=4, num_attention_heads=6, intermediate_size=1536, image_size=64, patch_size=16,
                                 backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[256, 512, 128, 128], neck_ignore_stages=[0, 1], reassemble_factors=[1, 1, 1, 0.5],
                                 fusion_hidden_size=64, readout_type="project", backbone_featmap_shape=[1, 1024, 4, 4],
                                 backbone_config=dict(model_type="bit", layer_type="bottleneck", depths=[1, 1, 1], out_features=["stage1", "stage2", "stage3"],
                                                      global_padding="same", embedding_dynamic_padding=True, num_groups=32))
    model = transformers.DPTForDepthEstimation(cfg).eval()
    synthetic_weights_(model, 7)
    model.save_pretrained(str(tmp_path))
    (tmp_path / "preprocessor_config.json").write_text(json.dumps(dict(size={"height": 64, "width": 64}, keep_aspect_ratio=False, ensure_multiple_of=1,
                                                                       image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5], resample=3)))
    from visiondepth3d_amd import synth
    small = torch.from_numpy(np.stack([synth.synth_frame(i, 96, 128)[0] for i in range(2)])).cuda()   # (252 x 476 -> 64 x 64 is past the front end's tap budget)
    x = R.depth_preprocess(small, 64, 64, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    with torch.no_grad():
        exp = model.double()(pixel_values=x.cpu().double()).predicted_depth
    assert float(exp.max() - exp.min()) > 0 and float((exp == 0).double().mean()) < 0.75
    for kw in (dict(gemm="bf16x3"), dict(gemm="fp16x2", conv="fp16x2", self_contained=True)):
        pipe = DepthPipe.from_pretrained(str(tmp_path), renderer=R, **kw)
        assert pipe.dpt_hybrid and pipe.resize_target(FH, FW) == (64, 64)
        with torch.no_grad():
            got = pipe.model(pixel_values=x).predicted_depth
        assert float((got.cpu().double() - exp).abs().max()) <= 1e-4 * float(exp.max() - exp.min()), (kw, float((got.cpu().double() - exp).abs().max()))
        if kw.get("self_contained"):
            assert all(v[0] == "fp16x2" for v in pipe.conv_routes.values()) and PREFIX + "encoder.stages.2.layers.0.norm3" in pipe.conv_routes
