"""GPU tests (-m gpu) of DepthPipe(self_contained=True) on a metric Depth-Anything model (depth_estimation_type="metric": the head ends in Sigmoid() * max_depth,
which vd3d_dpt_head_tail_act_f32 evaluates): depth-anything-v2-small's configuration made metric with max_depth 20, synthetic weights, the 9 x 17 patch grid and
the frames of tests/test_hip_self_contained.py, both pairs of the mode.

No vendor-library operator is dispatched; the prediction is float32-faithful against the stock module in float64 on the CPU (the stock float32 CPU module is the
yardstick; bars of tests/test_hip_depth_f64.py); the uint8 plane meets the stock float32 GPU graph's; forwards repeat bit for bit and a frame does not depend on
its batch; without the keyword the model routes as a relative one does and its head stays the module graph.  Under these weights the planes span about 1 to 18.5
of the 20 m: the sigmoid does not saturate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_hip_self_contained import BANNED, FH, FW, NAME, SIZE, _frames   # noqa: E402

PAIRS = ("bf16x3", "fp16x2")
MAX_DEPTH = 20


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _metric_model(seed):
    from transformers import DepthAnythingForDepthEstimation
    from visiondepth3d_amd.depth import build_config, synthetic_weights_
    cfg = build_config(NAME)
    cfg.depth_estimation_type, cfg.max_depth = "metric", MAX_DEPTH
    m = DepthAnythingForDepthEstimation(cfg).eval()
    assert isinstance(m.head.activation2, torch.nn.Sigmoid) and m.head.max_depth == MAX_DEPTH
    synthetic_weights_(m, seed)
    return m


def _pipe(R, seed, pair, **kw):
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    return DepthPipe(NAME + "-metric", device="cuda", dtype=torch.float32, renderer=R, model=_metric_model(seed), processor=dict(PROCESSORS["da"], size=SIZE),
                     gemm=pair, conv=pair, **kw)


_STOCK, _LEGS = {}, {}


def _stock(R, seed):
    """Per seed, once: the stock module's prediction for the two frames on the pipe's own pixel values -- float64 on the CPU (the truth), float32 on the CPU (the
    yardstick), float32 on the GPU.  Shared; not modified."""
    if seed not in _STOCK:
        from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD
        frames = _frames(2)
        x = R.depth_preprocess(frames, SIZE[0], SIZE[1], IMAGENET_MEAN, IMAGENET_STD).contiguous()
        stock = _metric_model(seed)
        with torch.no_grad():
            p32 = stock(pixel_values=x.cpu()).predicted_depth
            p32g = stock.cuda()(pixel_values=x).predicted_depth
            p64 = stock.cpu().double()(pixel_values=x.cpu().double()).predicted_depth
        _STOCK[seed] = dict(frames=frames, p64=p64, p32=p32, p32g=p32g)
    return _STOCK[seed]


def _leg(R, seed, pair):
    if (seed, pair) not in _LEGS:
        pipe = _pipe(R, seed, pair, self_contained=True)
        st = _stock(R, seed)
        assert pipe.resize_target(FH, FW) == SIZE
        _LEGS[seed, pair] = dict(st, pipe=pipe, pred=pipe.infer_bgr_u8(st["frames"], raw=True))
    return _LEGS[seed, pair]


@pytest.mark.parametrize("pair", PAIRS)
def test_metric_model_constructs_and_dispatches_no_vendor_library_operator(R, pair):
    """The constructor takes the Sigmoid head (it raised NotImplementedError before vd3d_dpt_head_tail_act_f32 existed); conv_routes names every convolution module
    that runs but head.conv3, which is inside the tail kernel, none as "library"; the second forward dispatches no ATen convolution, product or attention."""
    from torch.utils._python_dispatch import TorchDispatchMode
    leg = _leg(R, 0, pair)
    pipe = leg["pipe"]
    assert pipe.self_contained and pipe.tuned_gemm is False and pipe.miopen_find is False
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
    assert not any("sigmoid" in s for s in seen), [s for s in seen if "sigmoid" in s]   # the activation ran inside the tail kernel
    assert torch.equal(pred, leg["pred"])
    routes = pipe.conv_routes
    assert routes and all(v[0] == pair for v in routes.values()), routes
    mods = dict(pipe.model.named_modules())
    convs = [n for n, m in mods.items() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)) and "layers.0.residual_layer1" not in n and n != "head.conv3"]
    assert sorted(routes) == sorted(convs) and "head.conv3" not in routes, sorted(set(routes) ^ set(convs))


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("pair", PAIRS)
def test_metric_self_contained_is_float32_faithful_against_float64(R, pair, seed):
    """E = max |pred - pred64| / range(pred64) <= 2.5 x the stock float32 CPU module's, RMS <= 1.71 x its (the bars of tests/test_hip_depth_f64.py)."""
    from visiondepth3d_amd.depth import depth_to_u8
    leg = _leg(R, seed, pair)
    p64 = leg["p64"]
    rng = float(p64.max() - p64.min())
    levels = [int(torch.unique(depth_to_u8(p64[i:i + 1].float())).numel()) for i in range(p64.shape[0])]
    assert min(levels) >= 128 and 0.5 < float(p64.min()) and float(p64.max()) < MAX_DEPTH - 0.5, (levels, float(p64.min()), float(p64.max()))   # no flat, no saturated plane

    def err(p):
        d = p.detach().double().cpu() - p64
        return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng
    (E, rms), (E32, rms32) = err(leg["pred"]), err(leg["p32"])
    print("METRIC_SELF_CONTAINED_F64", dict(pair=pair, seed=seed, E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32,
                                            lo=float(p64.min()), hi=float(p64.max()), levels=levels))
    assert tuple(leg["pred"].shape) == tuple(p64.shape) == (2,) + SIZE and bool(torch.isfinite(leg["pred"]).all())
    assert E <= 2.5 * E32, (E, E32)
    assert rms <= 1.71 * rms32, (rms, rms32)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("pair", PAIRS)
def test_metric_self_contained_u8_plane_meets_the_stock_float32_graph(R, pair, seed):
    """depth_to_u8 of the raw prediction against that of the stock float32 graph on the GPU: no byte off by more than 1, >= 99.5 % identical."""
    from visiondepth3d_amd.depth import depth_to_u8
    leg = _leg(R, seed, pair)
    pred, exp = leg["pred"], leg["p32g"]
    d = (depth_to_u8(pred).to(torch.int16) - depth_to_u8(exp).to(torch.int16)).abs()
    st = dict(exact=float((d == 0).float().mean()), max=int(d.max()), pred_err_of_range=float((pred - exp).abs().max()) / float(exp.max() - exp.min()))
    print("METRIC_SELF_CONTAINED_U8", pair, seed, st)
    assert st["max"] <= 1 and st["exact"] >= 0.995, st


@pytest.mark.parametrize("pair", PAIRS)
def test_metric_self_contained_repeats_and_does_not_depend_on_the_batch(R, pair):
    leg = _leg(R, 0, pair)
    pipe = leg["pipe"]
    assert torch.equal(pipe.infer_bgr_u8(leg["frames"], raw=True), leg["pred"])
    f3 = _frames(3)
    one, three = pipe.infer_bgr_u8(f3[:1], raw=True), pipe.infer_bgr_u8(f3, raw=True)
    assert torch.equal(one[0], three[0])
    assert torch.equal(three[:2], leg["pred"])


@pytest.mark.parametrize("pair", PAIRS)
def test_without_the_keyword_a_metric_model_routes_as_it_always_did(R, pair, monkeypatch):
    """No keyword: conv_routes is what the relative model of the same shape gets in the same mode (the 3 x 3 stride-1 convolutions, by the size rule), head.conv3 is
    not in it and runs as the module it is, followed by the module graph's Sigmoid; the tail kernel is not called.  The prediction is the stock graph's."""
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    st = _stock(R, 0)
    pipe = _pipe(R, 0, pair)
    assert pipe.self_contained is False
    calls = dict(tail=0, conv3=0, sigmoid=0)
    orig = R.dpt_head_tail
    monkeypatch.setattr(R, "dpt_head_tail", lambda *a, **k: (calls.__setitem__("tail", calls["tail"] + 1), orig(*a, **k))[1])
    hooks = [pipe.model.head.conv3.register_forward_hook(lambda *_: calls.__setitem__("conv3", calls["conv3"] + 1)),
             pipe.model.head.activation2.register_forward_hook(lambda *_: calls.__setitem__("sigmoid", calls["sigmoid"] + 1))]
    pred = pipe.infer_bgr_u8(st["frames"], raw=True)
    for h in hooks:
        h.remove()
    assert calls == dict(tail=0, conv3=1, sigmoid=1), calls
    relative = DepthPipe(NAME, device="cuda", dtype=torch.float32, seed=0, renderer=R, processor=dict(PROCESSORS["da"], size=SIZE), gemm=pair, conv=pair)
    relative.infer_bgr_u8(st["frames"], raw=True)
    # neck and fusion stage: the relative model's routes; the head: the relative model's two 3 x 3 convolutions are routed in front of its tail kernel, the metric
    # head is the module graph from conv1 to the Sigmoid and so appears in no route
    assert pipe.conv_routes == {k: v for k, v in relative.conv_routes.items() if not k.startswith("head.")}
    assert not any(k.startswith("head.") for k in pipe.conv_routes) and {"head.conv1", "head.conv2"} <= set(relative.conv_routes)
    assert any(v[0] == "library" for v in pipe.conv_routes.values())           # at this size the split modes leave maps to the library: not the keyword's routes
    exp = st["p32g"]
    assert float((pred - exp).abs().max()) <= 1e-4 * float(exp.max() - exp.min())


def test_another_head_activation_is_refused_on_the_gpu_too(R):
    m = _metric_model(0)
    m.head.activation2 = torch.nn.Tanh()
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    with pytest.raises(NotImplementedError, match="ReLU.*Sigmoid"):
        DepthPipe("tanh-head", device="cuda", dtype=torch.float32, renderer=R, model=m, processor=dict(PROCESSORS["da"], size=SIZE), gemm="bf16x3", conv="bf16x3",
                  self_contained=True)
