"""CPU checks of DepthPipe's split-mode rewrite of DPT-Large (DPTForDepthEstimation on its plain ViT encoder, readout_type="project"):
the wiring -- packed QKV, the stash that hands each layer's first LayerNorm over from the layer before, the readout / projection linears, the transposed
convolutions as a GEMM + scatter, hook order, the fusion glue and the head tail -- against the stock transformers graph, with a torch double of every
renderer entry point that states what the HIP kernel computes.  The GPU tests (tests/test_hip_dpt.py) run the same graph on the kernels themselves."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
F = torch.nn.functional


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


class SplitDouble:
    """Float32 torch statements of the renderer entry points the rewrite calls (include/vd3d.h)."""

    def __init__(self):
        self.calls = dict(linear_x3=0, attention_x3=0, add_layernorm=0, depth_to_space_bias=0, bias_act=0, upsample_bilinear_bias=0, dpt_head_tail=0)

    def gemm_x3_pack(self, w, mode="bf16x3"):
        return w.detach().float().contiguous()

    def linear_x3(self, x, img, N, bias=None, gelu=False, mode="bf16x3"):
        self.calls["linear_x3"] += 1
        assert x.is_contiguous() and img.shape == (N, x.shape[-1])
        y = F.linear(x, img, bias)
        return F.gelu(y) if gelu else y

    def attention_x3(self, qkv, n_heads, scale, mode="bf16x3"):
        self.calls["attention_x3"] += 1
        B, T, C3 = qkv.shape
        q, k, v = qkv.view(B, T, 3, n_heads, C3 // (3 * n_heads)).unbind(2)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=scale)
        return o.transpose(1, 2).reshape(B, T, C3 // 3)

    def add_layernorm(self, x, y, norm):
        self.calls["add_layernorm"] += 1
        s = x if y is None else x + y
        return s, F.layer_norm(s, norm.normalized_shape, norm.weight, norm.bias, norm.eps)

    def depth_to_space_bias(self, y, B, H, W, s, bias=None):
        self.calls["depth_to_space_bias"] += 1
        C = y.shape[1] // (s * s)
        o = y.view(B, H, W, s, s, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H * s, W * s, C)
        if bias is not None:
            o = o + bias
        return o.permute(0, 3, 1, 2)

    def conv3x3_x2_pack(self, w):
        return w.detach().float().contiguous() if w.shape[0] in (32, 64, 128) and w.shape[1] % 16 == 0 else None

    def conv3x3_x2(self, x, img, Cout):
        return F.conv2d(x, img, None, 1, 1).contiguous(memory_format=torch.channels_last)

    def upsample_bilinear(self, x, size):
        return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)

    def bias_act(self, y, bias=None, r1=None, r2=None, relu=False, want_relu_copy=False):
        self.calls["bias_act"] += 1
        v = y if bias is None else y + bias.view(1, -1, 1, 1)
        if r1 is not None:
            v = v + r1
        if r2 is not None:
            v = r2 + v
        if relu:
            v = torch.relu(v)
        y.copy_(v)
        return (y, torch.relu(y)) if want_relu_copy else y

    def upsample_bilinear_bias(self, x, size, bias):
        self.calls["upsample_bilinear_bias"] += 1
        return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True) + bias.view(1, -1, 1, 1)

    def dpt_head_tail(self, y, b2, w3, b3, scale):
        self.calls["dpt_head_tail"] += 1
        return torch.relu((torch.relu(y + b2.view(1, -1, 1, 1)) * w3.view(1, -1, 1, 1)).sum(1) + b3) * scale


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
