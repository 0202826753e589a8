"""GPU tests (-m gpu) of DepthPipe(encoders=m, decoder=m) for DepthPro on the two synthetic geometries of depth_pro_cases: the neck, the fusion stage, the head and
the field-of-view convolutions on own kernels (depth_pro.DecoderRoutes) behind the routed encoders -- no vendor-library call between pixel_values and
predicted_depth / field_of_view.

The yardsticks are those of tests/test_hip_depth_pro_encoders.py: predicted_depth and field_of_view against the stock module in float64 on the CPU, held to the
stock float32 CPU module's own error against that float64 (maximum error <= 2.5 x, RMS <= 1.71 x); the uint8 plane against the stock path on the CPU (>= 99.5 %
identical, no byte off by more than one level).  With no library call left, the OUTPUTS are held bit for bit over two forwards and for a frame alone against the same
frame in a batch.  Each route switch at "0" (depth_pro.DECODER_SWITCHES) gives a pipe that meets the same bars.  The stock references are computed once per process
and not modified."""
import re

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import depth_pro_cases as cases   # noqa: E402

FH, FW = 135, 241
MODES = ["bf16x3", "fp16x2"]
BANNED = re.compile(r"^aten\.(convolution|_convolution|miopen_|cudnn_|mm\b|addmm|bmm|baddbmm|linear|matmul|_scaled_dot_product_|_flash_attention_forward|_efficient_attention_forward)")
_STOCK, _PIPES, _TRUE = {}, {}, {}


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()
    _PIPES.clear()
    _TRUE.clear()


def _u8_stats(a, b):
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return dict(exact=float((d == 0).float().mean()), max=int(d.max()))


def _stock(R):
    """Once: the stock module on the pixel values the pipe's network sees -- float64 on the CPU (the truth) and float32 on the CPU (the yardstick) -- and the stock
    path's final planes (processor in torch, float32 module, post-process in torch, all on the CPU)."""
    if not _STOCK:
        from visiondepth3d_amd.depth import depth_to_u8
        fr = cases.frames(2, FH, FW, 11)
        model = cases.build(cases.mini_config())
        x = R.depthpro_preprocess(fr.cuda(), 256, (0.5,) * 3, (0.5,) * 3)
        with torch.no_grad():
            o32 = model(pixel_values=x.cpu())
            o64 = cases.build(cases.mini_config()).double()(pixel_values=x.cpu().double())
            full = model(pixel_values=cases.processor_in_torch(fr, 256))
        inv = torch.stack(cases.post_process_in_torch(full.predicted_depth, full.field_of_view, [(FH, FW)] * 2))
        levels = [int(torch.unique(depth_to_u8(inv[i:i + 1])).numel()) for i in range(2)]
        assert min(levels) >= 100, levels   # no test here can pass on a flat plane
        _STOCK.update(frames=fr, x=x, o32=o32, o64=o64, inv=inv, u8=depth_to_u8(inv), levels=levels)
    return _STOCK


def _pipe(R, mode):
    if mode not in _PIPES:
        from visiondepth3d_amd.depth import DepthPipe
        _PIPES[mode] = DepthPipe("mini-depth-pro", model=cases.build(cases.mini_config()), processor=cases.mini_processor(), renderer=R, encoders=mode, decoder=mode)
    p = _PIPES[mode]
    assert p.encoders == mode and p.decoder == mode and p.arch == "depth_pro" and p.gemm == "f32" and not p.self_contained
    return p


def _bars(st, out, B, tag):
    """predicted_depth and field_of_view against float64, each beside the stock float32 CPU module's own error: 2.5 x maximum, 1.71 x RMS."""
    res = {}
    for key in ("predicted_depth", "field_of_view"):
        t64 = getattr(st["o64"], key)[:B]
        rng = float(t64.max() - t64.min()) if t64.numel() > 1 and float(t64.max() - t64.min()) > 0 else float(t64.abs().max())

        def err(p):
            d = p.detach().double().cpu() - t64
            return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng
        (E, rms), (E32, rms32) = err(getattr(out, key)), err(getattr(st["o32"], key)[:B])
        res[key] = dict(E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32)
    print("DEPTH_PRO_DECODER_F64", dict(tag, B=B, **res))
    assert tuple(out.predicted_depth.shape) == (B, 256, 256) and bool(torch.isfinite(out.predicted_depth).all()) and tuple(out.field_of_view.shape) == (B,)
    for key, r in res.items():
        assert r["E"] <= 2.5 * r["E_yardstick"], (key, r)
        assert r["rms"] <= 1.71 * r["rms_yardstick"], (key, r)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_mini_outputs_are_float32_faithful_against_float64(R, mode, B):
    st, pipe = _stock(R), _pipe(R, mode)
    with torch.no_grad():
        out = pipe.model(pixel_values=st["x"][:B])
    _bars(st, out, B, dict(mode=mode))


@pytest.mark.parametrize("mode", MODES)
def test_mini_uint8_product_against_the_stock_path(R, mode):
    st, pipe = _stock(R), _pipe(R, mode)
    got = pipe.depth_frames_u8(st["frames"].cuda())
    s = _u8_stats(got.cpu(), st["u8"])
    print("DEPTH_PRO_DECODER_U8", dict(s, mode=mode, levels=st["levels"]))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, FH, FW) and pipe.front_end_route == "kernel"
    assert s["exact"] >= 0.995 and s["max"] <= 1, s


def _decoder_modules(model):
    return sorted(n for n, m in model.named_modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Linear))
                  and n.startswith(("depth_pro.neck.", "fusion_stage.", "head.", "fov_model.conv", "fov_model.head.")))


@pytest.mark.parametrize("mode", MODES)
def test_no_library_operator_is_dispatched_and_every_module_has_a_route(R, mode):
    """A forward under a TorchDispatchMode: no convolution, matrix-product or attention operator of ATen between pixel_values and the two outputs.
    decoder_routes names every Conv2d / ConvTranspose2d of the decoder, each with a kernel of this project, the two new ones in their default form."""
    from torch.utils._python_dispatch import TorchDispatchMode
    st, pipe = _stock(R), _pipe(R, mode)
    with torch.no_grad():
        warm = pipe.model(pixel_values=st["x"])       # (position embeddings are interpolated once per input size)
    seen = []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    pipe.decoder_routes.clear()
    with torch.no_grad(), Log():
        out = pipe.model(pixel_values=st["x"])
    assert len(seen) > 20, seen
    bad = sorted({s for s in seen if BANNED.match(s)})
    assert not bad, bad
    assert torch.equal(out.predicted_depth, warm.predicted_depth) and torch.equal(out.field_of_view, warm.field_of_view)
    routes = pipe.decoder_routes
    assert sorted(routes) == _decoder_modules(pipe.model), sorted(set(routes) ^ set(_decoder_modules(pipe.model)))
    for name, route in routes.items():
        assert route.startswith(("vd3d_", "not run")) and "library" not in route, (name, route)
    assert [n for n, r in routes.items() if r.startswith("not run")] == ["fusion_stage.intermediate.0.residual_layer1.convolution1",
                                                                       "fusion_stage.intermediate.0.residual_layer1.convolution2"]
    from visiondepth3d_amd import depth_pro
    epi = {n: r for n, r in routes.items() if "residual_layer" in n and not r.startswith("not run")}
    assert len(epi) == 18 and routes["head.layers.0"].startswith("vd3d_conv3x3_")
    for n, r in dict(epi, **{"head.layers.0": routes["head.layers.0"]}).items():
        arg_set = re.search(r"\((relu_in\+bias\+relu|bias\+r1\+r2|bias\+r1|bias)\)", r)
        if r.startswith("vd3d_conv3x3_epi"):
            assert arg_set and (mode, arg_set.group(1)) in depth_pro.DECODER_EPI_ROUTED, (n, r)
        else:
            assert "not routed" in r, (n, r)
    want = "vd3d_depthpro_head" if mode in depth_pro.DECODER_HEAD_POLY_ROUTED else "vd3d_dpt_head_tail_f32"
    assert routes["head.layers.4"] == want, routes["head.layers.4"]
    assert routes["fov_model.conv"] == "vd3d_im2col_nhwc_f32 + vd3d_gemm_x3"          # 64 -> 32 channels: the stride-2 tile convolution builds multiples of 128


@pytest.mark.parametrize("mode", MODES)
def test_outputs_repeat_and_do_not_depend_on_the_batch(R, mode):
    st, pipe = _stock(R), _pipe(R, mode)
    with torch.no_grad():
        a, b, one = pipe.model(pixel_values=st["x"]), pipe.model(pixel_values=st["x"]), pipe.model(pixel_values=st["x"][:1])
    for key in ("predicted_depth", "field_of_view"):
        ta, tb, t1 = getattr(a, key), getattr(b, key), getattr(one, key)
        assert bool(torch.isfinite(ta).all()) and float(ta.abs().max()) > 0, key
        assert torch.equal(ta, tb), key
        assert torch.equal(ta[:1], t1), key


@pytest.mark.parametrize("switch", ["VD3D_DEPTHPRO_RES_EPI", "VD3D_DEPTHPRO_HEAD_POLY"])
@pytest.mark.parametrize("value", ["0", "1"])
@pytest.mark.parametrize("mode", MODES)
def test_each_route_switch_gives_a_pipe_inside_the_same_bars(R, mode, switch, value, monkeypatch):
    """"0": the residual units on bias-free convolution + vd3d_nhwc_bias_act_f32 (the same BITS as the fused epilogue) | the head on GEMM + depth-to-space + tile
    convolution + vd3d_dpt_head_tail_f32; "1": every built form.  decoder_routes says which form ran."""
    st, pipe = _stock(R), _pipe(R, mode)
    for name in ("VD3D_DEPTHPRO_RES_EPI", "VD3D_DEPTHPRO_HEAD_POLY"):
        monkeypatch.delenv(name, raising=False)
    with torch.no_grad():
        base = pipe.model(pixel_values=st["x"])
    monkeypatch.setenv(switch, value)
    with torch.no_grad():
        out = pipe.model(pixel_values=st["x"])
    routes = dict(pipe.decoder_routes)
    _bars(st, out, 2, dict(mode=mode, switch=f"{switch}={value}"))
    unit = routes["fusion_stage.final.residual_layer2.convolution2"]
    if switch == "VD3D_DEPTHPRO_RES_EPI":
        assert unit == ("vd3d_conv3x3_epi (bias+r1)" if value == "1" else f"vd3d_conv3x3_{R.TILE_CONVS[mode, 1]} + vd3d_nhwc_bias_act_f32 (VD3D_DEPTHPRO_RES_EPI=0)"), unit
        assert torch.equal(out.predicted_depth, base.predicted_depth) and torch.equal(out.field_of_view, base.field_of_view)   # the epilogue's contract
    else:
        assert routes["head.layers.4"] == ("vd3d_depthpro_head" if value == "1" else "vd3d_dpt_head_tail_f32"), routes["head.layers.4"]
        assert ("VD3D_DEPTHPRO_HEAD_POLY=0" in routes["head.layers.2"]) == (value == "0")
    assert all(r.startswith(("vd3d_", "not run")) for r in routes.values()), routes


@pytest.mark.parametrize("mode", MODES)
def test_the_forward_makes_no_host_synchronisation(R, mode):
    st, pipe = _stock(R), _pipe(R, mode)
    fr = st["frames"].cuda()
    pipe.infer_bgr_u8(fr)          # (one warm call: lazy initialisation may synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = pipe.infer_bgr_u8(fr)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("mode", MODES)
def test_a_model_without_the_field_of_view_branch_routes(R, mode):
    from visiondepth3d_amd.depth import DepthPipe
    m = cases.build(cases.mini_config(use_fov_model=False))
    fr = cases.frames(1, 64, 80, 13)
    with torch.no_grad():
        o = m(pixel_values=cases.processor_in_torch(fr, 256))
    exp = cases.post_process_in_torch(o.predicted_depth, None, [(64, 80)])[0]
    pipe = DepthPipe("mini-nofov", model=cases.build(cases.mini_config(use_fov_model=False)), processor=cases.mini_processor(), renderer=R, encoders=mode, decoder=mode)
    got = pipe.infer_bgr_u8(fr.cuda())[0].cpu()
    assert pipe.decoder == mode and not any(n.startswith("fov_model") for n in pipe.decoder_routes)
    assert float(((got - exp).abs() / exp).max()) <= 1e-4, float(((got - exp).abs() / exp).max())


def _true_grid(R):
    """Once: the stock graph on the GPU at the published 24 x 24 grid (1536 x 1536, fusion width 64: tile seams on 768 x 768 maps), one frame, and its uint8 plane."""
    if not _TRUE:
        from visiondepth3d_amd import depth_pro
        from visiondepth3d_amd.depth import PROCESSORS, DepthPipe, depth_to_u8
        fr = cases.frames(1, 270, 481, 21).cuda()
        pipe = DepthPipe("true-grid", model=cases.build(cases.true_grid_config(), fov_gain=40.0), processor=dict(PROCESSORS["depth_pro"]), renderer=R)
        xs = depth_pro.preprocess_statement(fr, (1536, 1536), (0.5,) * 3, (0.5,) * 3)
        with torch.no_grad():
            o = pipe.model(pixel_values=xs)
        exp = depth_to_u8(depth_pro.post_statement(o.predicted_depth, o.field_of_view, 270, 481))
        assert int(torch.unique(exp).numel()) >= 100
        _TRUE.update(frames=fr, u8=exp)
        del pipe
    return _TRUE


@pytest.mark.parametrize("mode", MODES)
def test_true_grid_one_frame_against_the_stock_graph_on_the_gpu(R, mode):
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    tg = _true_grid(R)
    pipe = DepthPipe("true-grid", model=cases.build(cases.true_grid_config(), fov_gain=40.0), processor=dict(PROCESSORS["depth_pro"]), renderer=R, encoders=mode,
                     decoder=mode)
    got = pipe.depth_frames_u8(tg["frames"])
    s = _u8_stats(got, tg["u8"])
    print("DEPTH_PRO_DECODER_TRUE_GRID", dict(s, mode=mode, levels=int(torch.unique(tg["u8"]).numel())))
    assert all(r.startswith(("vd3d_", "not run")) for r in pipe.decoder_routes.values()) and len(pipe.decoder_routes) == len(_decoder_modules(pipe.model))
    assert s["exact"] >= 0.995 and s["max"] <= 1, s
