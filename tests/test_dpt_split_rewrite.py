"""CPU checks of DepthPipe's split-mode rewrite of DPT-Large (DPTForDepthEstimation on its plain ViT encoder, readout_type="project"):
the wiring -- packed QKV, the stash that hands each layer's first LayerNorm over from the layer before, the readout / projection linears, the transposed
convolutions as a GEMM + scatter, hook order, the fusion glue and the head tail -- against the stock transformers graph, with a torch double of every
renderer entry point that states what the HIP kernel computes.  The GPU tests (tests/test_hip_dpt.py) run the same graph on the kernels themselves."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
F = torch.nn.functional

from renderer_doubles import SplitDouble   # noqa: E402


def _tiny_cfg(**kw):
    # 384-wide ViT with 64-wide heads (what the split kernels build), 4 layers, a 4 x 4 patch grid: the DPT-Large graph at a CPU test's size
    base = dict(hidden_size=384, num_hidden_layers=4, num_attention_heads=6, intermediate_size=768, image_size=64, patch_size=16,
                backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=32, readout_type="project")
    base.update(kw)
    return transformers.DPTConfig(**base)


def _model(cfg, seed=1):
    from visiondepth3d_amd.depth import synthetic_weights_
    m = transformers.DPTForDepthEstimation(cfg).eval()
    synthetic_weights_(m, seed)
    return m


def _split_pipe(cfg, mode="bf16x3"):
    """A CPU pipe with the split rewrite applied by hand (the constructor refuses split modes without a GPU renderer)."""
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    pipe = DepthPipe("tiny-dpt", device="cpu", model=_model(cfg), processor=dict(PROCESSORS["dpt"], size=(64, 64)))
    pipe.renderer, pipe.gemm = SplitDouble(), mode
    assert pipe._split_scope() == "dpt-vit"
    pipe._rewrite_dpt_vit()
    return pipe


@pytest.mark.parametrize("mode", ["bf16x3", "fp16x2"])
def test_dpt_vit_split_rewrite_is_the_module_graph(mode):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = _tiny_cfg()
    pipe = _split_pipe(cfg, mode)
    assert pipe.dpt_vit and pipe.arch == "generic"
    stock = _model(cfg)
    pv = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        got = pipe.model(pixel_values=pv).predicted_depth
        exp = stock(pixel_values=pv).predicted_depth
    assert got.shape == exp.shape == (2, 64, 64)
    assert float((got - exp).abs().max() / exp.abs().max()) < 1e-5
    c = pipe.renderer.calls
    L = cfg.num_hidden_layers
    # 4 linears per layer + 4 readouts + 4 projections + 2 transposed convolutions; one attention per layer; two scatters (hooks 0 / 1)
    assert c["linear_x3"] == 4 * L + 4 + 4 + 2 and c["attention_x3"] == L and c["depth_to_space_bias"] == 2, c
    # stash chaining: the first block's LayerNorm alone, then two add + LayerNorm launches per block, the last block's second residual add stands alone
    assert c["add_layernorm"] == 1 + 2 * L - 1, c
    # 4 fusion layers (7 residual units x 2 glue launches), 4 projections + head conv1 hand their bias to the up-sampling, one head tail
    assert (c["bias_act"], c["upsample_bilinear_bias"], c["dpt_head_tail"]) == (14, 5, 1), c
    with torch.no_grad():   # the memoised position embedding and the stash leave nothing behind between forwards
        assert torch.equal(pipe.model(pixel_values=pv).predicted_depth, got)


def test_dpt_vit_split_flops_count_what_runs():
    """flops_per_frame counts the EXECUTED convolution flops: the 1x1 projections and transposed convolutions that bypass the module hooks count
    themselves -- a transposed convolution with kernel == stride s is a GEMM of P x s^2 C x C, s^2 less than the hook's formula -- and the fusion
    projections run before their up-samplings (a quarter of the pixels), as in the DA rewrite."""
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    cfg = _tiny_cfg()
    stock = DepthPipe("tiny-dpt", device="cpu", model=_model(cfg), processor=dict(PROCESSORS["dpt"], size=(64, 64))).flops_per_frame(126, 224)
    mine = _split_pipe(cfg).flops_per_frame(126, 224)
    g, Cf = 4, cfg.fusion_hidden_size
    d_ct = sum(2.0 * C * C * s * s * g * g * (s * s - 1) for C, s in zip(cfg.neck_hidden_sizes[:2], (4, 2)))
    px_stock = g * g * (1 + 4 + 16 + 64)
    px_mine = (g // 2) ** 2 + g * g * (1 + 4 + 16)
    d_fusion = 2.0 * Cf * Cf * (px_stock - px_mine)
    assert abs((stock - mine) - (d_ct + d_fusion)) <= 1e-9 * stock, (stock, mine, d_ct, d_fusion)


def test_dpt_f32_pipe_is_the_stock_graph_bit_for_bit():
    """gemm="f32" (the default) leaves a DPT model's module graph exactly as transformers builds it: same bits through DepthPipe's CPU front end."""
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = _tiny_cfg()
    pipe = DepthPipe("tiny-dpt", device="cpu", model=_model(cfg), processor=dict(PROCESSORS["dpt"], size=(64, 64)))
    assert pipe.arch == "generic" and pipe.dpt_vit is False
    assert all("forward" not in m.__dict__ for m in pipe.model.modules())
    assert "_resize_pos_embed" not in pipe.model.dpt.embeddings.__dict__
    frames = torch.from_numpy(synth.synth_frame(3, 126, 224)[0][None].copy())
    got = pipe.infer_bgr_u8(frames, raw=True)
    stock = _model(cfg)
    x = frames.flip(-1).permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=(64, 64), mode="bicubic", antialias=True, align_corners=False)
    mean = torch.tensor(PROCESSORS["dpt"]["mean"]).view(1, 3, 1, 1)
    std = torch.tensor(PROCESSORS["dpt"]["std"]).view(1, 3, 1, 1)
    with torch.no_grad():
        exp = stock(pixel_values=((x / 255.0) - mean) / std).predicted_depth.float()
    assert torch.equal(got, exp)


def test_split_scope_refuses_what_is_not_built():
    """Everything the split rewrite does not build is refused by name, never run on a partial rewrite."""
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe

    def scope(model):
        pipe = DepthPipe("tiny", device="cpu", model=model, processor=dict(PROCESSORS["dpt"], size=(64, 64)))
        pipe.gemm = "bf16x3"
        return pipe._split_scope()

    for kw, why in ((dict(readout_type="add"), "readout_type"), (dict(readout_type="ignore"), "readout_type"),
                    (dict(add_projection=True, fusion_hidden_size=256), "head projection"),
                    (dict(use_batch_norm_in_fusion_residual=True), "batch norm"),
                    (dict(hidden_size=256, num_attention_heads=4, intermediate_size=512), "hidden size 256")):
        with pytest.raises(NotImplementedError, match=why):
            scope(_model(_tiny_cfg(**kw)))
    hybrid = transformers.DPTConfig(is_hybrid=True, hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=768,
                                    image_size=64, backbone_out_indices=[0, 1], neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=32,
                                    readout_type="project",
                                    backbone_config=dict(model_type="bit", global_padding="same", layer_type="bottleneck", depths=[1, 1, 1],
                                                         out_features=["stage1", "stage2", "stage3"], embedding_dynamic_padding=True, hidden_sizes=[64, 128, 256], num_groups=8))
    with pytest.raises(NotImplementedError, match="DPT-Hybrid"):
        scope(transformers.DPTForDepthEstimation(hybrid).eval())
    beit = transformers.DPTConfig(backbone_config=transformers.BeitConfig(hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=768,
                                                                         image_size=64, use_relative_position_bias=True, out_features=["stage1", "stage2"],
                                                                         reshape_hidden_states=False),
                                  neck_hidden_sizes=[16, 32], fusion_hidden_size=32, reassemble_factors=[2, 1], readout_type="project")
    with pytest.raises(NotImplementedError, match="BEiT|Beit"):
        scope(transformers.DPTForDepthEstimation(beit).eval())
    da = DepthPipe("depth-anything-v2-small", device="cpu")
    da.gemm = "bf16x3"
    assert da._split_scope() == "dinov2"
    with pytest.raises(NotImplementedError, match="depth-anything-v2-small"):
        da._split_scope(fuse_backbone=False)
