"""GPU tests (-m gpu) of DPT-Large in the split-operand modes (DepthPipe(gemm="bf16x3" | "fp16x2") on DPTForDepthEstimation with its plain ViT-L/16 encoder):
the reassemble stage's scatter kernel (vd3d_depth_to_space_bias_nhwc_f32), its transposed convolutions as split GEMM + scatter, the depth leg against the stock
float32 graph with the bar the DA modes meet (tests/test_hip_gemm.py), no silent fallback, the refusals, and gemm="f32" left as the stock graph."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
from test_hip_depth_e2e import _plane_stats, _record  # noqa: E402  (the uint8-plane statistics and the record of the DA depth-leg tests)

# synthetic weights, seed 5: the stock DPT-Large head's final ReLU leaves 8 % of a synthetic 1080p frame at zero (seed 0: 98 %, a flat plane that would
# compare equal whatever the backbone computed)
SEED = 5


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _frames(n, H=1080, W=1920):
    from visiondepth3d_amd import synth
    return torch.from_numpy(np.stack([synth.synth_frame(i, H, W)[0] for i in range(n)])).cuda()


def _stock_dpt_u8_planes(frames, seed=SEED):
    """The reference's statement for DPT-Large on torch float32: stock DPTForDepthEstimation, DPTImageProcessor's front end (384 x 384 without aspect keeping,
    antialiased bicubic, 1/255, mean = std = 0.5), the pipeline's bicubic post-process to the frame size, convert_depth_to_grayscale."""
    from transformers import DPTForDepthEstimation
    from visiondepth3d_amd.depth import PROCESSORS, build_config, depth_to_u8, synthetic_weights_
    model = DPTForDepthEstimation(build_config("dpt-large")).eval()
    synthetic_weights_(model, seed)
    model = model.cuda().float()
    B, H, W, _ = frames.shape
    x = frames.flip(-1).permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=(384, 384), mode="bicubic", antialias=True, align_corners=False)
    mean = torch.tensor(PROCESSORS["dpt"]["mean"], device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(PROCESSORS["dpt"]["std"], device="cuda").view(1, 3, 1, 1)
    with torch.no_grad():
        pred = model(pixel_values=((x / 255.0) - mean) / std).predicted_depth.float()
    full = F.interpolate(pred.unsqueeze(1), size=(H, W), mode="bicubic", align_corners=False).squeeze(1)
    return depth_to_u8(full), pred


@pytest.mark.parametrize("s,C", [(2, 256), (4, 256), (2, 512), (4, 512)])
def test_depth_to_space_bias_is_the_torch_reshape(R, s, C):
    """vd3d_depth_to_space_bias_nhwc_f32 is an exact copy plus one float32 add: bit for bit torch's view / permute / reshape + bias."""
    g = torch.Generator(device="cuda").manual_seed(s * 1000 + C)
    B, H, W = 3, 7, 5   # B * H * W odd
    y = torch.randn(B * H * W, s * s * C, device="cuda", generator=g)
    bias = torch.randn(C, device="cuda", generator=g)
    ref = y.view(B, H, W, s, s, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H * s, W * s)
    out = R.depth_to_space_bias(y, B, H, W, s, bias)
    assert out.shape == (B, C, H * s, W * s) and out.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(out, ref + bias.view(1, C, 1, 1))
    assert torch.equal(R.depth_to_space_bias(y, B, H, W, s), ref)


def test_depth_to_space_bias_refuses_shapes_it_does_not_build(R):
    from visiondepth3d_amd._lib import Vd3dError
    with pytest.raises(Vd3dError) as e:   # C not a multiple of 4
        R.depth_to_space_bias(torch.zeros(15, 4 * 6, device="cuda"), 1, 3, 5, 2, torch.zeros(6, device="cuda"))
    assert e.value.code == -4
    buf = torch.zeros(15 * 4 * 8 + 1, device="cuda")
    with pytest.raises(Vd3dError) as e:   # y not 16-byte aligned
        R.depth_to_space_bias(buf[1:].view(15, 32), 1, 3, 5, 2, torch.zeros(8, device="cuda"))
    assert e.value.code == -4


@pytest.mark.parametrize("mode", ["bf16x3", "fp16x2"])
@pytest.mark.parametrize("s,C", [(4, 256), (2, 512)])
def test_split_conv_transpose_is_float32_faithful(R, mode, s, C):
    """DPT-Large's reassemble transposed convolutions (hook 0: s = 4, C = 256; hook 1: s = 2, C = 512 on the 24 x 24 patch grid) as DepthPipe runs them --
    vd3d_gemm_x3 on the permuted weight, then the scatter + bias -- against float64 F.conv_transpose2d, beside PyTorch's float32 CPU transposed convolution on
    the same operands: maximum error <= 2.5 x, RMS <= 1.5 x the float32 one's (the bar of test_conv3x3_x2_is_float32_faithful)."""
    from visiondepth3d_amd.depth import conv_transpose_gemm_weight
    g = torch.Generator(device="cuda").manual_seed(s * 7 + C)
    B, H, W = 1, 24, 24
    x = torch.randn(B, H, W, C, device="cuda", generator=g) * torch.exp(torch.randn(1, 1, 1, C, device="cuda", generator=g))   # NHWC rows
    w = torch.randn(C, C, s, s, device="cuda", generator=g) / C ** 0.5
    b = torch.randn(C, device="cuda", generator=g) * 0.1
    img = R.gemm_x3_pack(conv_transpose_gemm_weight(w), mode)
    y = R.linear_x3(x.view(B * H * W, C), img, s * s * C, None, mode=mode)
    out = R.depth_to_space_bias(y, B, H, W, s, b)
    xn = x.permute(0, 3, 1, 2)
    ref = F.conv_transpose2d(xn.double(), w.double(), b.double(), stride=s)
    y32 = F.conv_transpose2d(xn.cpu(), w.cpu(), b.cpu(), stride=s).to(x.device)
    scale = F.conv_transpose2d(xn.abs().double(), w.abs().double(), b.abs().double(), stride=s) + 1e-30
    e3, e32 = float(((out.double() - ref).abs() / scale).max()), float(((y32.double() - ref).abs() / scale).max())
    r3 = float((out.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    r32 = float((y32.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    assert e3 <= max(2.5 * e32, 2.0 ** -21), (e3, e32)
    assert r3 <= 1.5 * r32 + 1e-9, (r3, r32)


@pytest.mark.parametrize("mode", ["bf16x3", "fp16x2"])
def test_dpt_large_split_meets_the_float32_legs_bar_1080p(R, mode):
    """DPT-Large in a split mode against the STOCK float32 graph: raw prediction within 1e-4 of its range, >= 99.5 % of the uint8 hand-off bytes identical,
    no byte off by more than one level -- the bar of the DA modes (tests/test_hip_gemm.py)."""
    from visiondepth3d_amd.depth import DepthPipe
    H, W = 1080, 1920
    frames = _frames(2, H, W)
    exp_u8, exp_pred = _stock_dpt_u8_planes(frames)
    pipe = DepthPipe("dpt-large", device="cuda", dtype=torch.float32, renderer=R, gemm=mode, seed=SEED)
    assert pipe.dpt_vit and pipe.arch == "generic"
    pred = pipe.infer_bgr_u8(frames, raw=True)
    assert pred.shape == exp_pred.shape == (2, 384, 384)
    st = _plane_stats(R.depth_handoff(pred, H, W), exp_u8)
    st["pred_max_err_of_range"] = float((pred - exp_pred).abs().max()) / float(exp_pred.max() - exp_pred.min())
    st["stock_zero_fraction"] = float((exp_pred == 0).float().mean())
    _record("dpt_" + mode + "_1080p", st)
    assert st["pred_max_err_of_range"] < 1e-4, st
    assert st["exact"] >= 0.995 and st["max"] <= 1, st


@pytest.mark.parametrize("mode", ["bf16x3", "fp16x2"])
def test_dpt_large_split_runs_on_the_library_kernels(R, mode, monkeypatch):
    """No silent fallback: one forward calls the split attention once per layer, the split GEMM for the 4 linears of each of the 24 layers plus the 4 readout
    and 4 projection linears (and the two transposed convolutions), and the scatter for hooks 0 and 1."""
    from visiondepth3d_amd.depth import DepthPipe
    pipe = DepthPipe("dpt-large", device="cuda", dtype=torch.float32, renderer=R, gemm=mode, seed=SEED)
    calls = dict(linear_x3=0, attention_x3=0, depth_to_space_bias=0)
    for name in calls:
        orig = getattr(R, name)

        def counted(*a, _orig=orig, _name=name, **kw):
            calls[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(R, name, counted)
    pipe.infer_bgr_u8(_frames(1), raw=True)
    assert calls["attention_x3"] >= 24, calls
    assert calls["linear_x3"] >= 4 * 24 + 4 + 4, calls
    assert calls["depth_to_space_bias"] == 2, calls


def test_split_modes_refuse_dpt_hybrid_and_beit(R):
    import transformers
    from visiondepth3d_amd.depth import DepthPipe
    hybrid = transformers.DPTConfig(is_hybrid=True, hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=768, image_size=64,
                                    backbone_out_indices=[0, 1], neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=32, readout_type="project",
                                    backbone_config=dict(model_type="bit", global_padding="same", layer_type="bottleneck", depths=[1, 1, 1],
                                                         out_features=["stage1", "stage2", "stage3"], embedding_dynamic_padding=True,
                                                         hidden_sizes=[64, 128, 256], num_groups=8))
    beit = transformers.DPTConfig(backbone_config=transformers.BeitConfig(hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=768,
                                                                         image_size=64, use_relative_position_bias=True, out_features=["stage1", "stage2"],
                                                                         reshape_hidden_states=False),
                                  neck_hidden_sizes=[16, 32], fusion_hidden_size=32, reassemble_factors=[2, 1], readout_type="project")
    for cfg, what in ((hybrid, "DPT-Hybrid"), (beit, "Beit")):
        with pytest.raises(NotImplementedError, match=what):
            DepthPipe("tiny-dpt", device="cuda", model=transformers.DPTForDepthEstimation(cfg).eval(), renderer=R, gemm="bf16x3")


def test_dpt_f32_with_renderer_is_the_stock_graph(R):
    """gemm="f32" with a renderer leaves DPT-Large's module graph as transformers builds it: no forward replaced, no method patched, the parameters bit for bit
    the stock model's, and the prediction the stock model's on the same input.  The bit-for-bit statement of the output is the CPU test
    (tests/test_dpt_split_rewrite.py); on the GPU the float32 library kernels do not repeat bit for bit from one model instance to the next, so the output is held
    to 1e-5 of its range (the split modes' bar is 1e-4)."""
    from transformers import DPTForDepthEstimation
    from visiondepth3d_amd.depth import DepthPipe, build_config, synthetic_weights_
    pipe = DepthPipe("dpt-large", device="cuda", dtype=torch.float32, renderer=R, seed=SEED)
    assert pipe.arch == "generic" and pipe.dpt_vit is False
    assert all("forward" not in m.__dict__ for m in pipe.model.modules())
    assert "_resize_pos_embed" not in pipe.model.dpt.embeddings.__dict__
    stock = DPTForDepthEstimation(build_config("dpt-large")).eval()
    synthetic_weights_(stock, SEED)
    stock = stock.cuda().float().to(memory_format=torch.channels_last)
    ps, ss = dict(pipe.model.named_parameters()), dict(stock.named_parameters())
    assert ps.keys() == ss.keys() and all(torch.equal(ps[k], ss[k]) for k in ps)
    x = pipe.renderer.depth_preprocess(_frames(2), 384, 384, pipe.proc["mean"], pipe.proc["std"])
    with torch.no_grad():
        got = pipe.model(pixel_values=x).predicted_depth
        exp = stock(pixel_values=x).predicted_depth
    err = float((got - exp).abs().max()) / float(exp.max() - exp.min())
    _record("dpt_f32_vs_stock", dict(pred_max_err_of_range=err, bit_equal=bool(torch.equal(got, exp))))
    assert err < 1e-5, err


def test_from_pretrained_dpt_folder_reaches_the_split_modes(R, tmp_path):
    """A local DPT checkpoint folder (config.json + model.safetensors + preprocessor_config.json) through from_pretrained with gemm="bf16x3": the split
    rewrite runs and computes the stock graph's prediction."""
    import transformers
    from visiondepth3d_amd.depth import DepthPipe, synthetic_weights_
    cfg = transformers.DPTConfig(hidden_size=384, num_hidden_layers=4, num_attention_heads=6, intermediate_size=1536, image_size=384, patch_size=16,
                                 backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[64, 128, 256, 256], fusion_hidden_size=64, readout_type="project")
    model = transformers.DPTForDepthEstimation(cfg).eval()
    synthetic_weights_(model, 7)   # this small net's head leaves 0.1 % of a synthetic frame at zero with seed 7
    model.save_pretrained(str(tmp_path))
    (tmp_path / "preprocessor_config.json").write_text(json.dumps(dict(size={"height": 384, "width": 384}, keep_aspect_ratio=False, ensure_multiple_of=1,
                                                                       image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5], resample=3)))
    pipe = DepthPipe.from_pretrained(str(tmp_path), renderer=R, gemm="bf16x3")
    assert pipe.dpt_vit
    stock = model.cuda()
    x = R.depth_preprocess(_frames(1), 384, 384, pipe.proc["mean"], pipe.proc["std"])
    with torch.no_grad():
        got = pipe.model(pixel_values=x).predicted_depth
        exp = stock(pixel_values=x.contiguous()).predicted_depth
    assert float(exp.max() - exp.min()) > 0
    assert float((got - exp).abs().max()) <= 1e-4 * float(exp.max() - exp.min()), (got - exp).abs().max()
