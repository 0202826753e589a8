"""GPU tests (-m gpu) of ZoeDepth end to end through DepthPipe(model=..., renderer=R): tiny multi-head and single-head models, the front end, the metric head and
the post-process on the four kernels of csrc/vd3d_zoedepth.hip, held to the float64 CPU run of the stock modules behind the torch statements under the project's
bar for float32 paths: error <= max(2.5 x the float32 CPU run's error against the same float64, 2^-21), relative to the magnitude of the prediction."""
import contextlib
import copy

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import zoedepth_cases as cases   # noqa: E402


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


_MODELS, _REFS = {}, {}


@contextlib.contextmanager
def _deterministic_library():
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = was


def _model(which):
    """"nyu" / "kitti": the multi-head model with the vote forced by the classifier's last bias (a vote near a tie could fall differently in two float32 runs);
    "single": the single-head model."""
    if which not in _MODELS:
        m = cases.tiny_model(which != "single", seed=11)
        if which != "single":
            cases.force_domain(m, ("nyu", "kitti").index(which))
        _MODELS[which] = m
    return _MODELS[which]


def _reference(which, B, H, W):
    """(float64 reference at the frame size, float32 CPU run, frames): the stock modules behind preprocess_statement and the restated post-process; computed once."""
    key = (which, B, H, W)
    if key not in _REFS:
        from visiondepth3d_amd import zoedepth
        m = _model(which)
        fr = cases.frames(B, H, W, 31 + H)
        x = zoedepth.preprocess_statement(fr, cases.TINY_PROCESSOR)
        with torch.no_grad():
            p64 = copy.deepcopy(m).double()(pixel_values=x.double()).predicted_depth
            p32 = m(pixel_values=x).predicted_depth
        ref64 = torch.stack(cases.post_process_in_torch(p64, [(H, W)] * B))
        ref32 = torch.stack(cases.post_process_in_torch(p32, [(H, W)] * B))
        _REFS[key] = (ref64, ref32, fr)
    return _REFS[key]


def _pipe(R, which):
    from visiondepth3d_amd.depth import DepthPipe
    return DepthPipe("zoe-tiny", model=copy.deepcopy(_model(which)), processor=cases.TINY_PROCESSOR, renderer=R)


def _check(pipe, which, B, H, W, tag):
    from visiondepth3d_amd.depth import depth_to_u8
    ref64, ref32, fr = _reference(which, B, H, W)
    got = pipe.infer_bgr_u8(fr.cuda())
    assert pipe.front_end_route == "kernel" and got.shape == (B, H, W) and got.dtype == torch.float32
    scale = float(ref64.abs().max())
    e, e32 = float((got.cpu().double() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale
    rms, rms32 = float((got.cpu().double() - ref64).pow(2).mean().sqrt()) / scale, float((ref32.double() - ref64).pow(2).mean().sqrt()) / scale
    u_got, u_ref = depth_to_u8(got).cpu().int(), depth_to_u8(ref64.float()).int()
    off = int((u_got - u_ref).abs().max())
    print(tag, dict(model=which, B=B, frame=(H, W), max=e, yardstick_max=e32, rms=rms, yardstick_rms=rms32, range_over_mean=float((ref64.max() - ref64.min()) / ref64.mean()),
                    u8_max_off=off, u8_identical=float((u_got == u_ref).float().mean())))
    assert e <= max(2.5 * e32, 2.0 ** -21), (e, e32)
    assert off <= 1
    return got


@pytest.mark.parametrize("B,H,W", [(1, 45, 61), (3, 90, 160)])
@pytest.mark.parametrize("which", ["nyu", "kitti", "single"])
def test_pipe_is_the_stock_model_behind_the_statements(R, which, B, H, W):
    pipe = _pipe(R, which)
    assert pipe.arch == "zoedepth" and pipe.zoe_routes == {"metric_head": "kernels"}
    got = _check(pipe, which, B, H, W, "ZOE_E2E")
    if which == "single":
        assert pipe.zoe_domain is None
    else:   # the vote, on the device, equal to the stock module's
        assert isinstance(pipe.zoe_domain, torch.Tensor) and pipe.zoe_domain.is_cuda and pipe.zoe_domain.tolist() == [("nyu", "kitti").index(which)]
    # two forwards repeat bit for bit.  Under torch.backends.cudnn.deterministic: without it MIOpen runs the 1 x 1 convolutions of the single-head model's MLPs
    # (128 / 256 input channels) on a solver that sums in a run-dependent order -- with the STOCK head as well (measured: one ulp between warm forwards of
    # seed_bin_regressor.conv2, seed_projector.conv2, projectors.*.conv2, ... on equal inputs; none with the flag) -- which is the library's doing, not the route's
    fr = _reference(which, B, H, W)[2].cuda()
    with _deterministic_library():
        pipe.infer_bgr_u8(fr)   # (the solver search of the flag's first call)
        assert torch.equal(pipe.infer_bgr_u8(fr), pipe.infer_bgr_u8(fr))
    raw = pipe.infer_bgr_u8(fr, raw=True)
    assert tuple(raw.shape) == (B, 64, 96)


@pytest.mark.parametrize("which", ["kitti", "single"])
def test_the_switch_puts_the_stock_head_back(R, which, monkeypatch):
    monkeypatch.setenv("VD3D_ZOE_HEAD", "0")
    pipe = _pipe(R, which)
    assert pipe.zoe_routes == {"metric_head": "stock: VD3D_ZOE_HEAD=0"} and "forward" not in pipe.model.metric_head.__dict__
    _check(pipe, which, 3, 90, 160, "ZOE_E2E_STOCK_HEAD")
    assert pipe.zoe_domain is None


def test_bfloat16_keeps_the_stock_head(R):
    from visiondepth3d_amd.depth import DepthPipe
    pipe = DepthPipe("zoe-tiny", model=copy.deepcopy(_model("single")), processor=cases.TINY_PROCESSOR, renderer=R, dtype=torch.bfloat16)
    assert pipe.zoe_routes["metric_head"].startswith("stock") and "forward" not in pipe.model.metric_head.__dict__


@pytest.mark.parametrize("which", ["nyu", "single"])
def test_a_warm_head_forward_makes_no_host_synchronisation(R, which):
    """The routed metric head alone, on inputs already on the device: a warm forward under torch.cuda.set_sync_debug_mode("error") -- the multi-head model's
    ``.item()`` on the domain vote is gone."""
    pipe = _pipe(R, which)
    inp = cases.head_inputs(_model(which), 2, 64, 96, seed=3)
    dev = lambda t: t.cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.cuda()   # noqa: E731
    args = (dev(inp[0]), dev(inp[1]), [dev(f) for f in inp[2]], dev(inp[3]))
    with torch.no_grad(), _deterministic_library():   # (the flag: see the repeat check above)
        pipe.model.metric_head(*args)   # (the library's solver search for the new shapes)
        warm, _ = pipe.model.metric_head(*args)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again, _ = pipe.model.metric_head(*args)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(warm, again)


def test_statement_route_for_an_inference_size(R):
    """With an inference size the front end is the statement (ATen operators on the device) and the post-process still the kernel."""
    pipe = _pipe(R, "single")
    fr = cases.frames(1, 45, 61, 5).cuda()
    got = pipe.infer_bgr_u8(fr, inference_size=(80, 48), at_inference_size=True)
    assert pipe.front_end_route == "statement" and got.shape == (1, 48, 80) and bool(torch.isfinite(got).all())
    assert pipe.depth_frames_u8(fr).shape == (1, 45, 61)
