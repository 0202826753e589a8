"""GPU tests (-m gpu) of DepthPro (DepthProForDepthEstimation) in DepthPipe on the two synthetic geometries of depth_pro_cases: MINI (256 x 256, a 4 x 4 token grid:
the padding clamp and the non-identity merge resize) and TRUE-GRID (1536 x 1536, the published 24 x 24 grid, one frame).

What is built is the float32 mode: the front end and the post-process are own launches (vd3d_depthpro_preprocess_u8, vd3d_depthpro_post_f32), the network between
them is the stock module graph.  The split modes (gemm="bf16x3" / "fp16x2", with or without conv=) and self_contained=True refuse DepthPro by name; that refusal is
tested here.  The yardsticks are those of tests/test_hip_self_contained_dpt.py / tests/test_hip_dpt_hybrid.py: the model's outputs against the stock module in
float64 on the CPU (the depth map), held to the stock float32 CPU module's own error against that float64 (maximum error <= 2.5 x, RMS <= 1.71 x); the uint8 plane against the stock
path (no byte off by more than one level, >= 99.5 % identical).  No test here can pass on a flat plane: the float64 truth has >= 100 distinct uint8 levels per frame."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import depth_pro_cases as cases   # noqa: E402

FH, FW = 135, 241
_STOCK = {}


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _u8_stats(a, b):
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return dict(exact=float((d == 0).float().mean()), max=int(d.max()))


def _stock(R):
    """Once: the stock module on the pixel values the pipe's network sees -- float64 on the CPU (the truth) and float32 on the CPU (the yardstick) -- and the stock
    path's final planes (processor in torch, float32 module, post-process in torch, all on the CPU).  Shared; not modified."""
    if not _STOCK:
        from visiondepth3d_amd.depth import DepthPipe, depth_to_u8
        fr = cases.frames(2, FH, FW, 11)
        model = cases.build(cases.mini_config())
        x = R.depthpro_preprocess(fr.cuda(), 256, (0.5,) * 3, (0.5,) * 3)
        with torch.no_grad():
            o32 = model(pixel_values=x.cpu())
            o64 = cases.build(cases.mini_config()).double()(pixel_values=x.cpu().double())
            full = model(pixel_values=cases.processor_in_torch(fr, 256))
        inv = torch.stack(cases.post_process_in_torch(full.predicted_depth, full.field_of_view, [(FH, FW)] * 2))
        levels = [int(torch.unique(depth_to_u8(inv[i:i + 1])).numel()) for i in range(2)]
        assert min(levels) >= 100, levels
        pipe = DepthPipe("mini-depth-pro", model=cases.build(cases.mini_config()), processor=cases.mini_processor(), renderer=R)
        _STOCK.update(frames=fr, x=x, o32=o32, o64=o64, inv=inv, u8=depth_to_u8(inv), pipe=pipe, levels=levels)
    return _STOCK


def _f64_leg(R, B):
    st = _stock(R)
    pipe = st["pipe"]
    assert pipe.arch == "depth_pro" and pipe.gemm == "f32" and not pipe.self_contained
    with torch.no_grad():
        return st, pipe.model(pixel_values=st["x"][:B])


@pytest.mark.parametrize("B", [1, 2])
def test_mini_f32_depth_is_float32_faithful_against_float64(R, B):
    """predicted_depth on the pixel values of the front end kernel: E = max |pred - pred64| / range(pred64) <= 2.5 x the stock float32 CPU module's, RMS <= 1.71 x
    its (the bars of tests/test_hip_self_contained_dpt.py).  Measured: E ratio 0.72 - 0.93, RMS ratio 0.79.  In this mode the network is the stock module graph, so
    this is the yardstick a routed network will be held to, not a test of own arithmetic.  The field of view is not held to the same rule here: it is one number per
    frame, the yardstick is then a single draw of the CPU module's error, and the ratio of the library graph on the GPU to it moved between 1.55 and 2.59 from card
    to card -- a bar that no code of this project decides.  What the project does with the field of view is tested where it is deterministic: the post-process
    kernel against the processor (tests/test_hip_depth_pro_kernels.py, two frames with different fields of view) and the uint8 product below."""
    st, out = _f64_leg(R, B)
    p64 = st["o64"].predicted_depth[:B]
    rng = float(p64.max() - p64.min())

    def err(p):
        d = p.detach().double().cpu() - p64
        return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng
    (E, rms), (E32, rms32) = err(out.predicted_depth), err(st["o32"].predicted_depth[:B])
    print("DEPTH_PRO_F64", dict(B=B, E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32, levels=st["levels"]))
    assert tuple(out.predicted_depth.shape) == (B, 256, 256) and bool(torch.isfinite(out.predicted_depth).all())
    assert E <= 2.5 * E32, (E, E32)
    assert rms <= 1.71 * rms32, (rms, rms32)


def test_mini_uint8_product_against_the_stock_path(R):
    """depth_frames_u8 (front end kernel, network, post-process kernel, min-max hand-off) against the stock path on the CPU: >= 99.5 % of the bytes identical and
    none off by more than one level.  The two frames' fields of view differ (about 62 and 86 degrees), so a field of view applied to the wrong frame shows.
    infer_bgr_u8 itself: inverse depths inside the clamp, at the frame size; raw at the model's; ``front_end_route`` says which front end ran."""
    st = _stock(R)
    pipe = st["pipe"]
    got = pipe.depth_frames_u8(st["frames"].cuda())
    s = _u8_stats(got.cpu(), st["u8"])
    inv = pipe.infer_bgr_u8(st["frames"].cuda())
    rel = float(((inv.cpu() - st["inv"]).abs() / st["inv"]).max())
    print("DEPTH_PRO_U8", dict(s, levels=st["levels"], inverse_depth_max_rel=rel))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, FH, FW)
    assert s["exact"] >= 0.995 and s["max"] <= 1, s
    assert pipe.front_end_route == "kernel"
    assert tuple(inv.shape) == (2, FH, FW) and float(inv.min()) >= 0.99e-4 and float(inv.max()) <= 1.01e4
    assert tuple(pipe.infer_bgr_u8(st["frames"].cuda(), raw=True).shape) == (2, 256, 256)
    # the reference protocol at an inference size: the prediction comes back at that size
    res = pipe([st["frames"][0].numpy()[..., ::-1].copy()], inference_size=(96, 54))
    assert tuple(res[0]["predicted_depth"].shape) == (54, 96) and pipe.front_end_route == "statement"   # (an inference size: the front end as ATen operators)


def test_the_field_of_view_never_leaves_the_device(R):
    """No host synchronisation between the network and the post-process: the forward runs under torch.cuda.set_sync_debug_mode("error")."""
    st = _stock(R)
    fr = st["frames"].cuda()
    st["pipe"].infer_bgr_u8(fr)          # (first call: lazy initialisation may synchronise)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = st["pipe"].infer_bgr_u8(fr)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out).all())


def test_a_model_without_the_field_of_view_branch_runs_unscaled(R):
    from visiondepth3d_amd.depth import DepthPipe
    m = cases.build(cases.mini_config(use_fov_model=False))
    fr = cases.frames(1, 64, 80, 13)
    with torch.no_grad():
        o = m(pixel_values=cases.processor_in_torch(fr, 256))
    assert o.field_of_view is None
    exp = cases.post_process_in_torch(o.predicted_depth, None, [(64, 80)])[0]
    got = DepthPipe("mini-nofov", model=cases.build(cases.mini_config(use_fov_model=False)), processor=cases.mini_processor(), renderer=R).infer_bgr_u8(fr.cuda())[0].cpu()
    assert float(((got - exp).abs() / exp).max()) <= 1e-4, float(((got - exp).abs() / exp).max())


def test_split_modes_self_contained_tiles_and_pil_refuse_depth_pro_by_name(R):
    from visiondepth3d_amd.depth import DepthPipe
    m = cases.build(cases.mini_config())
    for kw in (dict(gemm="bf16x3"), dict(gemm="fp16x2"), dict(gemm="bf16x3", conv="bf16x3"), dict(gemm="fp16x2", conv="fp16x2")):
        with pytest.raises(NotImplementedError, match=r"gemm='(bf16x3|fp16x2)': 'mini' \(DepthProForDepthEstimation\).*not built"):
            DepthPipe("mini", model=m, processor=cases.mini_processor(), renderer=R, **kw)
    for pair in ("bf16x3", "fp16x2"):
        with pytest.raises(NotImplementedError, match=r"self_contained=True: 'mini' \(DepthProForDepthEstimation\).*not built"):
            DepthPipe("mini", model=m, processor=cases.mini_processor(), renderer=R, gemm=pair, conv=pair, self_contained=True)
    assert next(m.parameters()).device.type == "cpu"           # refused before the module was moved to a device
    with pytest.raises(NotImplementedError, match=r"front_end='pil': 'mini' \(DepthProForDepthEstimation\)"):
        DepthPipe("mini", model=m, processor=cases.mini_processor(), renderer=R, front_end="pil")
    with pytest.raises(NotImplementedError, match=r"tiled depth: 'mini-depth-pro' \(DepthProForDepthEstimation\)"):
        _stock(R)["pipe"].depth_frames_u8(_stock(R)["frames"].cuda(), tiled=True)


def test_true_grid_one_frame_against_the_stock_graph_on_the_gpu(R):
    """The published 24 x 24 grid at 1536 x 1536 (merges of 24 / 48 / 96, every resize the identity), one frame.  A GPU-to-GPU comparison: the pipe (front end kernel,
    stock graph, post-process kernel) against the processor and the post-process stated in torch ON THE GPU around the same module -- no float64 pass at this size.
    The pixel values are held to depth_pro_cases.bilinear_bound (A = 1, D = 2), the uint8 plane to the end-to-end bar (>= 99.5 % identical, one level at most)."""
    from visiondepth3d_amd import depth_pro
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe, depth_to_u8
    fr = cases.frames(1, 270, 481, 21).cuda()
    pipe = DepthPipe("true-grid", model=cases.build(cases.true_grid_config(), fov_gain=40.0), processor=dict(PROCESSORS["depth_pro"]), renderer=R)
    assert pipe.resize_target(270, 481) == (1536, 1536)
    x = R.depthpro_preprocess(fr, 1536, (0.5,) * 3, (0.5,) * 3)
    xs = depth_pro.preprocess_statement(fr, (1536, 1536), (0.5,) * 3, (0.5,) * 3)
    assert float((x - xs).abs().max()) <= cases.bilinear_bound(1.0, 2.0, 270, 481)
    with torch.no_grad():
        o = pipe.model(pixel_values=xs)
    assert tuple(o.predicted_depth.shape) == (1, 1536, 1536)
    exp = depth_to_u8(depth_pro.post_statement(o.predicted_depth, o.field_of_view, 270, 481))
    got = pipe.depth_frames_u8(fr)
    s = _u8_stats(got, exp)
    print("DEPTH_PRO_TRUE_GRID", dict(s, levels=int(torch.unique(exp).numel()), fov=o.field_of_view.tolist()))
    assert int(torch.unique(exp).numel()) >= 100
    assert s["exact"] >= 0.995 and s["max"] <= 1, s
