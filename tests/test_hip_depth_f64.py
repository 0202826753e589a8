"""GPU tests (-m gpu) of the depth leg against FLOAT64 under trained-like weights (tests/outlier_weights.py: massive residual channels, rows that are small
everywhere, nearly one-hot softmaxes, a prediction off the ReLU floor -- tests/test_outlier_weights_host.py asserts that the reference shows them).

    2 uint8 frames of 210 x 378 -> DepthPipe(model=<DA-V2-Small, outlier weights>, processor size (210, 378), gemm / conv mode) -> raw prediction

406 tokens: two 256-query attention workgroups, 22 valid rows in the last 64-row KV tile.  Reference: the STOCK Hugging Face module in float64 on the CPU
behind a float64 pre-process of the same frames.  Yardstick: the same in float32 on the CPU -- independent of the convolution solver a GPU box picks, the
reason tests/test_hip_gemm.py gives for its convolution yardstick.  Per mode

    E   = max |pred - pred64| / range(pred64)            RMS = sqrt(mean (pred - pred64)^2) / range(pred64)

and the bar is  E <= K x E_yardstick,  RMS <= K_RMS x RMS_yardstick.  K and K_RMS are what two stock float32 implementations of this graph differ by: 1.5 x
the largest ratio (stock float32 module on the GPU vs float64) / (stock float32 module on the CPU vs float64) over the three seeds, with the project's
kernel-level factors as floors (2.5 on the maximum, 1.5 on the RMS).  MEASURED below records the measurement (tools/probe_depth_f64.py on an MI355X,
profiles/r09_range_and_outliers.md): K = 2.5 (the floor), K_RMS = 1.71.  Measured against it on that box, as E / E_yardstick and RMS / RMS_yardstick over the
three seeds: f32 0.27 - 1.26 and 0.46 - 1.31; bf16x3 0.42 - 0.89 and 0.72 - 0.98 (the same with conv="bf16x3"); fp16x2 0.29 - 0.93 and 0.48 - 1.11.  The
yardstick itself moves a little with the CPU's thread count (seed 0: 1.16e-4 of the range with 16 threads, 1.28e-4 with 8)."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
pytest.importorskip("transformers")
F = torch.nn.functional

import outlier_weights as ow   # noqa: E402

H, W = 210, 378
MODES = {"f32": dict(gemm="f32"), "bf16x3": dict(gemm="bf16x3"), "bf16x3+conv": dict(gemm="bf16x3", conv="bf16x3"), "fp16x2": dict(gemm="fp16x2")}
# (stock float32 module on the GPU) / (stock float32 module on the CPU), both against float64, the largest over seeds 0 .. 2 -- measured on an MI355X with
# tools/probe_depth_f64.py: maximum 0.92 (0.92, 0.63, 0.72 per seed), RMS 1.14 (1.14, 0.74, 0.85).
MEASURED = dict(max_ratio=0.9164, rms_ratio=1.1397)
K = max(2.5, 1.5 * MEASURED["max_ratio"])         # 2.5: the floor holds
K_RMS = max(1.5, 1.5 * MEASURED["rms_ratio"])     # 1.71
# fp16x2 is held to the same bar: it meets it under these weights (measured 0.29 - 0.93 x on the maximum, 0.48 - 1.11 x on the RMS)
BARS = {mode: (K, K_RMS) for mode in MODES}


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _plane_stats(a, b):
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return dict(exact=float((d == 0).float().mean()), within1=float((d <= 1).float().mean()), max=int(d.max()), mean_abs=float(d.float().mean()))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mode", list(MODES))
def test_depth_leg_is_float32_faithful_against_float64(R, mode, seed, record_property):
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe, depth_to_u8
    pred64, pred32 = ow.reference_predictions(seed)
    frames = torch.from_numpy(ow.clip_frames()).cuda()
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, model=ow.stock_model(seed, torch.float32),
                     processor=dict(PROCESSORS["da"], size=(H, W)), renderer=R, **MODES[mode])
    assert pipe.resize_target(H, W) == (H, W)
    pred = pipe.infer_bgr_u8(frames, raw=True)
    assert tuple(pred.shape) == tuple(pred64.shape) and bool(torch.isfinite(pred).all())
    if MODES[mode].get("conv"):
        assert any(v[0] == "bf16x3" for v in pipe.conv_routes.values()), pipe.conv_routes     # some convolution really took the kernel at this size
    E, rms = ow.errors_of_range(pred, pred64)
    E32, rms32 = ow.errors_of_range(pred32, pred64)
    full64 = F.interpolate(pred64.unsqueeze(1), size=(H, W), mode="bicubic", align_corners=False).squeeze(1)
    st = _plane_stats(R.depth_handoff(pred, H, W).cpu(), depth_to_u8(full64))
    k, k_rms = BARS[mode]
    fig = dict(mode=mode, seed=seed, E=E, E_yardstick=E32, E_ratio=E / E32, rms=rms, rms_yardstick=rms32, rms_ratio=rms / rms32, k=k, k_rms=k_rms, u8=st)
    record_property("depth_f64", fig)
    print("DEPTH_F64", fig)
    assert E <= k * E32, fig
    assert rms <= k_rms * rms32, fig
