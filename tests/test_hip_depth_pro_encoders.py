"""GPU tests (-m gpu) of DepthPipe(encoders="bf16x3" | "fp16x2") for DepthPro on the two synthetic geometries of depth_pro_cases: the patch pyramid, the three
Dinov2Model encoders and every patch merge on own kernels, the neck / fusion stage / head / field-of-view convolutions the stock module graph behind them.

The yardsticks are those of tests/test_hip_depth_pro.py: predicted_depth against the stock module in float64 on the CPU, held to the stock float32 CPU module's
own error against that float64 (maximum error <= 2.5 x, RMS <= 1.71 x: the bars of tests/test_hip_self_contained_dpt.py); the uint8 plane against the stock path on
the CPU (>= 99.5 % identical, no byte off by more than one level).  The tensors the own kernels hand to the library decoder are additionally held bit for bit:
over two forwards, and for a frame alone against the same frame in a batch.  The stock references are computed once per process and not modified."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import depth_pro_cases as cases   # noqa: E402

FH, FW = 135, 241
MODES = ["bf16x3", "fp16x2"]
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
        _PIPES[mode] = DepthPipe("mini-depth-pro", model=cases.build(cases.mini_config()), processor=cases.mini_processor(), renderer=R, encoders=mode)
    p = _PIPES[mode]
    assert p.encoders == mode and p.arch == "depth_pro" and p.gemm == "f32" and not p.self_contained
    return p


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_mini_depth_is_float32_faithful_against_float64(R, mode, B):
    """predicted_depth on the pixel values of the front end kernel: E = max |pred - pred64| / range(pred64) <= 2.5 x the stock float32 CPU module's, RMS <= 1.71 x
    its.  The ratios are printed (DEPTH_PRO_ENCODERS_F64) and recorded in profiles/r28_depth_pro_encoders.md."""
    st, pipe = _stock(R), _pipe(R, mode)
    with torch.no_grad():
        out = pipe.model(pixel_values=st["x"][:B])
    assert pipe.encoders_resize == {"image": "pyramid", "fov": "pyramid"}   # 256 / 4 is the encoders' image size: neither resized for itself
    p64 = st["o64"].predicted_depth[:B]
    rng = float(p64.max() - p64.min())

    def err(p):
        d = p.detach().double().cpu() - p64
        return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng
    (E, rms), (E32, rms32) = err(out.predicted_depth), err(st["o32"].predicted_depth[:B])
    print("DEPTH_PRO_ENCODERS_F64", dict(mode=mode, B=B, E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32, levels=st["levels"]))
    assert tuple(out.predicted_depth.shape) == (B, 256, 256) and bool(torch.isfinite(out.predicted_depth).all())
    assert E <= 2.5 * E32, (E, E32)
    assert rms <= 1.71 * rms32, (rms, rms32)


@pytest.mark.parametrize("mode", MODES)
def test_mini_uint8_product_against_the_stock_path(R, mode):
    """depth_frames_u8 of two frames whose fields of view differ, against the stock path on the CPU: >= 99.5 % of the bytes identical, none off by more than one."""
    st, pipe = _stock(R), _pipe(R, mode)
    got = pipe.depth_frames_u8(st["frames"].cuda())
    s = _u8_stats(got.cpu(), st["u8"])
    print("DEPTH_PRO_ENCODERS_U8", dict(s, mode=mode, levels=st["levels"]))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, FH, FW)
    assert pipe.front_end_route == "kernel"
    assert s["exact"] >= 0.995 and s["max"] <= 1, s


def _own_features(pipe, x):
    """The tensors the own kernels hand over in one forward: the list DepthProNeck receives and the field-of-view encoder's features."""
    got = {}
    h1 = pipe.model.depth_pro.neck.register_forward_pre_hook(lambda mod, args: got.__setitem__("neck", [t.clone() for t in args[0]]))
    h2 = pipe.model.fov_model.fov_encoder.register_forward_hook(lambda mod, args, out: got.__setitem__("fov", out.clone()))
    try:
        with torch.no_grad():
            pipe.model(pixel_values=x)
    finally:
        h1.remove()
        h2.remove()
    return got["neck"] + [got["fov"]]


@pytest.mark.parametrize("mode", MODES)
def test_own_kernel_features_repeat_and_do_not_depend_on_the_batch(R, mode):
    """What reaches DepthProNeck (image features, three pyramid levels, two hooks) and the field-of-view features: equal bit for bit over two forwards, and frame
    0's tensors in a two-frame batch equal its tensors alone -- no library call chooses them.  (The prediction behind the library decoder is not held to this.)"""
    st, pipe = _stock(R), _pipe(R, mode)
    a, b, one = _own_features(pipe, st["x"]), _own_features(pipe, st["x"]), _own_features(pipe, st["x"][:1])
    assert [tuple(t.shape) for t in a] == [(2, 384, 4, 4), (2, 384, 4, 4), (2, 384, 8, 8), (2, 384, 16, 16), (2, 384, 16, 16), (2, 384, 16, 16), (2, 32, 4, 4)]
    for i, (ta, tb, t1) in enumerate(zip(a, b, one)):
        assert bool(torch.isfinite(ta).all()) and float(ta.abs().max()) > 0, i
        assert torch.equal(ta, tb), i
        assert torch.equal(ta[:1], t1), i


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
    assert o.field_of_view is None
    exp = cases.post_process_in_torch(o.predicted_depth, None, [(64, 80)])[0]
    pipe = DepthPipe("mini-nofov", model=cases.build(cases.mini_config(use_fov_model=False)), processor=cases.mini_processor(), renderer=R, encoders=mode)
    got = pipe.infer_bgr_u8(fr.cuda())[0].cpu()
    assert pipe.encoders == mode and pipe.encoders_resize == {"image": "pyramid"}
    assert float(((got - exp).abs() / exp).max()) <= 1e-4, float(((got - exp).abs() / exp).max())


def _true_grid(R):
    """Once: the stock graph on the GPU at the published 24 x 24 grid (1536 x 1536, 37 sequences of 577 tokens), one frame, and its uint8 plane."""
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
    """T = 577, 37 sequences, merges of 24 / 48 / 96 (every resize the identity): the uint8 bar against the stock graph on the GPU."""
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    tg = _true_grid(R)
    pipe = DepthPipe("true-grid", model=cases.build(cases.true_grid_config(), fov_gain=40.0), processor=dict(PROCESSORS["depth_pro"]), renderer=R, encoders=mode)
    got = pipe.depth_frames_u8(tg["frames"])
    s = _u8_stats(got, tg["u8"])
    print("DEPTH_PRO_ENCODERS_TRUE_GRID", dict(s, mode=mode, levels=int(torch.unique(tg["u8"]).numel())))
    assert pipe.encoders_resize == {"image": "pyramid", "fov": "pyramid"}
    assert s["exact"] >= 0.995 and s["max"] <= 1, s
