"""Host-only tests of the DPT-Hybrid (MiDaS 3.0, Intel/dpt-hybrid-midas) entry of DepthPipe: the published configuration, the stock CPU model built from it, the
scope rule of the split modes, the refusals of DepthPipe(self_contained=True) for a BiT prefix it does not build (raised before a device or a renderer is touched,
so they run here), the folded weight standardisation and the column order of vd3d_im2col_nhwc_f32's GEMM weight."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
import torch.nn.functional as F   # noqa: E402

NAME = "dpt-hybrid-midas"
BIT = dict(model_type="bit", layer_type="bottleneck", depths=[3, 4, 9], out_features=["stage1", "stage2", "stage3"], global_padding="same",
           embedding_dynamic_padding=True, num_groups=32)


def _tiny_hybrid(bit=None, **kw):
    """A hybrid in the published geometry at a small size: ViT of 2 layers, hidden 384, a BiT prefix of one bottleneck per stage, 64 x 64 input (a 4 x 4 grid)."""
    cfg = dict(is_hybrid=True, hidden_size=384, num_hidden_layers=4, num_attention_heads=6, intermediate_size=768, image_size=64, patch_size=16,
               backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[256, 512, 64, 64], neck_ignore_stages=[0, 1], reassemble_factors=[1, 1, 1, 0.5],
               fusion_hidden_size=32, readout_type="project", backbone_featmap_shape=[1, 1024, 4, 4],
               backbone_config=dict(BIT, depths=[1, 1, 1], **(bit or {})))
    cfg.update(kw)
    return transformers.DPTForDepthEstimation(transformers.DPTConfig(**cfg)).eval()


def _scope(model, **attrs):
    from visiondepth3d_amd.depth import DepthPipe
    pipe = DepthPipe.__new__(DepthPipe)
    pipe.name, pipe.model, pipe.arch, pipe.gemm, pipe.self_contained = "probe", model, "generic", "bf16x3", False
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe._split_scope()


def test_build_config_carries_the_published_geometry():
    from visiondepth3d_amd.depth import MODEL_ZOO, PROCESSORS, build_config
    assert NAME in MODEL_ZOO and MODEL_ZOO[NAME]["arch"] == "dpt"
    c = build_config(NAME)
    assert c.is_hybrid is True and (c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size) == (768, 12, 12, 3072)
    assert (c.image_size, c.patch_size, c.readout_type, c.fusion_hidden_size) == (384, 16, "project", 256)
    assert list(c.backbone_out_indices) == [2, 5, 8, 11] and list(c.neck_hidden_sizes) == [256, 512, 768, 768]
    assert list(c.neck_ignore_stages) == [0, 1] and list(c.reassemble_factors) == [1, 1, 1, 0.5] and list(c.backbone_featmap_shape) == [1, 1024, 24, 24]
    b = c.backbone_config
    assert (b.model_type, b.layer_type, list(b.depths), list(b.out_features)) == ("bit", "bottleneck", [3, 4, 9], ["stage1", "stage2", "stage3"])
    assert (str(b.global_padding).lower(), b.embedding_dynamic_padding, b.num_groups) == ("same", True, 32)
    assert PROCESSORS["dpt"] == dict(size=(384, 384), keep_aspect_ratio=False, multiple=1, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))


@pytest.fixture(scope="module")
def stock():
    from visiondepth3d_amd.depth import build_config, synthetic_weights_
    m = transformers.DPTForDepthEstimation(build_config(NAME)).eval()
    synthetic_weights_(m, 5)
    return m


def test_stock_cpu_model_maps_384_to_384(stock):
    with torch.no_grad():
        y = stock(pixel_values=torch.zeros(2, 3, 384, 384)).predicted_depth
    assert tuple(y.shape) == (2, 384, 384) and bool(torch.isfinite(y).all())


def test_split_scope_accepts_the_published_geometry_and_refuses_every_other_hybrid(stock):
    assert _scope(stock) == "dpt-hybrid"
    assert _scope(_tiny_hybrid()) == "dpt-hybrid"
    # the two-hook / 8-group hybrid of tests/test_hip_dpt.py and tests/test_dpt_split_rewrite.py
    two = transformers.DPTConfig(is_hybrid=True, hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=768, image_size=64,
                                 backbone_out_indices=[0, 1], neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=32, readout_type="project",
                                 backbone_config=dict(model_type="bit", global_padding="same", layer_type="bottleneck", depths=[1, 1, 1],
                                                      out_features=["stage1", "stage2", "stage3"], embedding_dynamic_padding=True, hidden_sizes=[64, 128, 256], num_groups=8))
    with pytest.raises(NotImplementedError, match="DPT-Hybrid"):
        _scope(transformers.DPTForDepthEstimation(two).eval())
    with pytest.raises(NotImplementedError, match="DPT-Hybrid.*8 groups"):
        _scope(_tiny_hybrid(bit=dict(num_groups=8)))
    with pytest.raises(NotImplementedError, match="DPT-Hybrid.*preactivation"):
        _scope(_tiny_hybrid(bit=dict(layer_type="preactivation")))
    # transformers itself refuses to construct a hybrid with readout_type="add"; the rule reads the configuration, so the probe sets it on a constructed model
    add = _tiny_hybrid()
    add.config.readout_type = "add"
    with pytest.raises(NotImplementedError, match="DPT-Hybrid.*readout_type='add'"):
        _scope(add)
    with pytest.raises(NotImplementedError, match="DPT-Hybrid.*neck_ignore_stages"):
        m = _tiny_hybrid()
        m.config.neck_ignore_stages = [0]
        _scope(m)
    with pytest.raises(NotImplementedError, match="hidden size 256"):
        _scope(_tiny_hybrid(hidden_size=256, num_attention_heads=4, intermediate_size=512))


def test_self_contained_refuses_a_prefix_it_does_not_build_by_name():
    """bit_prefix_plan reads the module graph only; DepthPipe(self_contained=True) calls it in its constructor before the renderer or a device is used."""
    from visiondepth3d_amd.depth import bit_prefix_plan

    def plan(m):
        return bit_prefix_plan(m.dpt.embeddings.backbone, {id(mod): n for n, mod in m.named_modules()})
    ok = plan(_tiny_hybrid())
    kinds = sorted(ok["conv"].values())
    assert kinds.count("im2col") == 5 and kinds.count("tile") == 1 and kinds.count("gemm") == 7 and len(ok["relu"]) == 13, kinds
    m = _tiny_hybrid()
    conv = m.dpt.embeddings.backbone.bit.encoder.stages[1].layers[0].conv1
    conv.bias = torch.nn.Parameter(torch.zeros(conv.out_channels))
    with pytest.raises(NotImplementedError, match=r"stages\.1\.layers\.0\.conv1 has a bias"):
        plan(m)
    with pytest.raises(NotImplementedError, match="layer_type='preactivation'"):
        plan(_tiny_hybrid(bit=dict(layer_type="preactivation")))
    with pytest.raises(NotImplementedError, match="num_groups=8"):
        plan(_tiny_hybrid(bit=dict(num_groups=8)))
    with pytest.raises(NotImplementedError, match="global_padding=None"):
        plan(_tiny_hybrid(bit=dict(global_padding=None)))
    m = _tiny_hybrid()
    m.dpt.embeddings.backbone.bit.encoder.stages[0].layers[0].conv2.dilation = (2, 2)
    with pytest.raises(NotImplementedError, match=r"stages\.0\.layers\.0\.conv2: kernel \(3, 3\).*dilation \(2, 2\)"):
        plan(m)


def test_folded_standardised_weights_are_the_modules_own(stock, monkeypatch):
    """bit_standardized_weight(m) equals, bit for bit, the weight WeightStandardizedConv2d hands to conv2d in its forward (the stem, a 1 x 1, both 3 x 3 kinds and
    a strided shortcut of the full-size model)."""
    from visiondepth3d_amd.depth import bit_standardized_weight
    bit = stock.dpt.embeddings.backbone.bit
    l10 = bit.encoder.stages[1].layers[0]
    seen = []
    real = F.conv2d
    monkeypatch.setattr(F, "conv2d", lambda x, w, *a, **k: (seen.append(w), real(x, w, *a, **k))[1])
    for m in (bit.embedder.convolution, l10.conv1, l10.conv2, bit.encoder.stages[0].layers[1].conv2, l10.downsample.conv):
        seen.clear()
        with torch.no_grad():
            m(torch.zeros(1, m.in_channels, 8, 8))
        assert len(seen) == 1 and seen[0].dtype == torch.float32
        assert torch.equal(bit_standardized_weight(m), seen[0]), type(m)
        assert not torch.equal(seen[0], m.weight)


@pytest.mark.parametrize("k,cin", [(7, 3), (3, 16), (1, 32)])
@pytest.mark.parametrize("side", [(12, 10), (11, 13)])
def test_im2col_column_order_and_same_padding(k, cin, side):
    """The torch statement of vd3d_im2col_nhwc_f32's rows -- pad, unfold, permute to (ky, kx, c), zero tail -- times im2col_gemm_weight(W) equals F.conv2d on
    the same padded input to float32 rounding (a different summation order over K <= 160 terms of magnitude <= 1: 1e-5 is 40 ulp of the largest sum), at stride
    2 with TensorFlow "same" padding on even and odd sides; same_padding agrees with transformers' DynamicPad2d."""
    from transformers.models.bit.modeling_bit import DynamicPad2d
    from visiondepth3d_amd.depth import im2col_gemm_weight, same_padding
    H, W = side
    g = torch.Generator().manual_seed(k * 100 + H)
    x = torch.rand(2, cin, H, W, generator=g) * 2 - 1
    w = (torch.rand(8, cin, k, k, generator=g) * 2 - 1) / (k * k * cin) ** 0.5
    (pt, pb), (pl, pr) = same_padding(H, k, 2), same_padding(W, k, 2)
    xp = F.pad(x, (pl, pr, pt, pb))
    assert torch.equal(xp, DynamicPad2d(k, 2, 1)(x))
    if k == 7 and H % 2 == 0:
        assert (pt, pb) == (2, 3)
    if k == 3 and H % 2 == 0:
        assert (pt, pb) == (0, 1)
    exp = F.conv2d(xp, w, None, 2)
    Ho, Wo = exp.shape[2:]
    cols = F.unfold(xp, k, stride=2).view(2, cin, k, k, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(2, Ho * Wo, k * k * cin)   # [(ky, kx, c)]
    kp = (k * k * cin + 15) // 16 * 16
    rows = F.pad(cols, (0, kp - k * k * cin))
    wg = im2col_gemm_weight(w)
    assert tuple(wg.shape) == (8, kp) and bool((wg[:, k * k * cin:] == 0).all())
    got = (rows @ wg.t()).view(2, Ho, Wo, 8).permute(0, 3, 1, 2)
    assert float((got - exp).abs().max()) <= 1e-5
