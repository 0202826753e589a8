"""Host tests (no GPU) of ZoeDepth in DepthPipe: the zoo entry, the processor's size rule and front end against transformers' own code, the pipe on the CPU against
model + restated post-process, the composed metric head against the stock modules in float64, the multi-head route's device-index selection, every refusal by its
wording, and the from_pretrained round trip."""
import copy
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import zoedepth_cases as cases   # noqa: E402

IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


@pytest.fixture(scope="module")
def multi():
    return cases.tiny_model(True, seed=1)


@pytest.fixture(scope="module")
def single():
    return cases.tiny_model(False, seed=2)


def test_the_zoo_entry_builds():
    """MODEL_ZOO["zoedepth-nyu-kitti"] (a KeyError before this feature): the published geometry, built on the meta device -- 345 073 307 parameters."""
    from visiondepth3d_amd import zoedepth
    from visiondepth3d_amd.depth import MODEL_ZOO, PROCESSORS, build_config
    assert MODEL_ZOO["zoedepth-nyu-kitti"]["arch"] == "zoedepth"
    c = build_config("zoedepth-nyu-kitti")
    bc = c.backbone_config
    assert (bc.model_type, bc.hidden_size, bc.num_hidden_layers, bc.num_attention_heads, bc.patch_size, bc.image_size) == ("beit", 1024, 24, 16, 16, 384)
    assert bc.use_relative_position_bias and not bc.use_absolute_position_embeddings and not bc.reshape_hidden_states
    assert list(bc.out_features) == ["stage6", "stage12", "stage18", "stage24"]
    assert list(c.neck_hidden_sizes) == [256, 512, 1024, 1024] and c.fusion_hidden_size == c.bottleneck_features == 256 and c.num_relative_features == 32
    assert c.bin_embedding_dim == 128 and list(c.num_attractors) == [16, 8, 4, 1] and c.bin_centers_type == "softplus"
    assert [(b["name"], b["n_bins"], b["min_depth"], b["max_depth"]) for b in c.bin_configurations] == [("nyu", 64, 1e-3, 10.0), ("kitti", 64, 1e-3, 80.0)]
    assert (c.num_patch_transformer_layers, c.patch_transformer_hidden_size, c.patch_transformer_intermediate_size, c.patch_transformer_num_attention_heads) == (4, 128, 1024, 4)
    with torch.device("meta"):
        m = transformers.ZoeDepthForDepthEstimation(c)
    assert sum(p.numel() for p in m.parameters()) == 345_073_307
    assert type(m.metric_head).__name__ == "ZoeDepthMultipleMetricDepthEstimationHeads"
    assert PROCESSORS["zoedepth"] == dict(size=(384, 512), keep_aspect_ratio=True, multiple=32, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), resample=2, pad=True)
    assert zoedepth.ZOE_SWITCHES == ("VD3D_ZOE_HEAD",)
    from visiondepth3d_amd.depth_routes import _SWITCHES
    assert "VD3D_ZOE_HEAD" not in _SWITCHES


@pytest.mark.parametrize("multiple", [32, 1 / 32, 14])
def test_resize_target_is_the_processors_rule(multiple):
    from transformers.models.zoedepth.image_processing_pil_zoedepth import get_resize_output_image_size
    from visiondepth3d_amd.zoedepth import pad_amounts, resize_target
    n = 0
    for h in list(range(5, 400, 23)) + [1080, 1218, 2160]:
        for w in list(range(5, 700, 31)) + [1920, 2104, 3840]:
            for keep in (True, False):
                ref = get_resize_output_image_size(np.zeros((3, h, w), np.float32), (384, 512), keep, multiple, transformers.image_utils.ChannelDimension.FIRST)
                assert resize_target(h, w, (384, 512), multiple, keep) == (int(ref[0]), int(ref[1])), (h, w, keep)
                n += 1
    assert n > 800
    assert pad_amounts(1080, 1920) == (69, 92) and resize_target(1080 + 138, 1920 + 184, (384, 512), 32) == (384, 672)
    assert pad_amounts(5, 5) == (4, 4)


@pytest.mark.parametrize("norm", [dict(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)), IMAGENET], ids=["half", "imagenet"])
@pytest.mark.parametrize("multiple", [32, 1 / 32])
@pytest.mark.parametrize("H,W", [(5, 5), (37, 53), (270, 481), (384, 512), (100, 640), (720, 1280), (1080, 1920)])
def test_preprocess_statement_is_the_class_bit_for_bit(H, W, multiple, norm):
    from visiondepth3d_amd import zoedepth
    proc = dict(zoedepth.PROCESSOR, multiple=multiple, **norm)
    fr = cases.frames(1, H, W, H + W)
    ref = cases.processor_in_class(fr, proc)
    got = zoedepth.preprocess_statement(fr, proc)
    assert got.dtype == torch.float32 and torch.equal(got, ref)
    # a plain float32 product is NOT the class's rescale
    tab = zoedepth.rescale_table()
    assert not torch.equal(tab, torch.arange(256, dtype=torch.float32) * torch.tensor(1 / 255, dtype=torch.float32))


@pytest.mark.parametrize("which", ["multi", "single"])
def test_pipe_on_the_cpu_is_model_plus_restated_post_process(which, multi, single):
    from visiondepth3d_amd import zoedepth
    from visiondepth3d_amd.depth import DepthPipe
    m = multi if which == "multi" else single
    p = DepthPipe("zoe-tiny", device="cpu", model=copy.deepcopy(m), processor=cases.TINY_PROCESSOR)
    assert p.arch == "zoedepth" and p.zoe_routes["metric_head"].startswith("stock") and p.zoe_domain is None
    fr = cases.frames(2, 45, 61, 7)
    x = zoedepth.preprocess_statement(fr, cases.TINY_PROCESSOR)
    assert tuple(x.shape[-2:]) == (64, 96)
    with torch.no_grad():
        pred = m(pixel_values=x).predicted_depth
    exp = torch.stack(cases.post_process_in_torch(pred, [(45, 61)] * 2))
    got = p.infer_bgr_u8(fr)
    assert p.front_end_route == "statement" and got.shape == (2, 45, 61) and torch.equal(got, exp)
    assert torch.equal(p.infer_bgr_u8(fr, raw=True), pred)
    rgb = np.ascontiguousarray(fr[0].numpy()[..., ::-1])
    one = p([rgb])[0]["predicted_depth"]
    with torch.no_grad():   # (the multi-head vote runs over the batch: a single frame is its own batch)
        exp1 = cases.post_process_in_torch(m(pixel_values=x[:1]).predicted_depth, [(45, 61)])[0]
    assert torch.equal(one, exp1)
    # with an inference size the pipeline sees the pre-resized image
    got = p.infer_bgr_u8(fr, inference_size=(80, 48), at_inference_size=True)
    assert got.shape == (2, 48, 80) and p.front_end_route == "statement"
    assert p.depth_frames_u8(fr).shape == (2, 45, 61)


def _stock64(head, inp):
    h = copy.deepcopy(head).double()
    with torch.no_grad():
        return h(inp[0].double(), inp[1].double(), [f.double() for f in inp[2]], inp[3].double())


@pytest.mark.parametrize("is_multi", [True, False], ids=["multi", "single"])
def test_head_statement_is_the_stock_head_in_float64(is_multi):
    """The composed form (W1 . cat(last, up(e)) = W1_last . last + up(W1_e . e)) against the stock module, both in float64.  With default-initialised weights the
    prediction is the constant log 2 and the log-binomial table cancels: exact up to association, 1e-12.  With synthetic weights the bar is 1e-7: the table --
    log_binom(k_minus_1, k_idx) on integer buffers plus a Python float, hence FLOAT32 in the stock module whatever its dtype -- is the whole difference between
    this figure and rounding error; the statement takes the module's table, so both sides carry the same float32 values."""
    from visiondepth3d_amd import zoedepth
    for synthetic, bar in ((False, 1e-12), (True, 1e-7)):
        m = cases.tiny_model(is_multi, seed=3, synthetic=synthetic)
        inp = cases.head_inputs(m, 2, 64, 96, seed=5)
        ref, ref_logits = _stock64(m.metric_head, inp)
        got, logits = zoedepth.head_statement(m.metric_head, *inp)
        rel = float(((got - ref).abs() / ref.abs()).max())
        print("ZOE_HEAD_STATEMENT", dict(multi=is_multi, synthetic=synthetic, max_rel=rel, lo=float(ref.min()), hi=float(ref.max())))
        assert got.dtype == torch.float64 and got.shape == ref.shape and rel <= bar
        assert (logits is None) == (ref_logits is None) == (not is_multi)
        if is_multi:
            assert torch.allclose(logits, ref_logits, rtol=1e-12, atol=1e-12)
        if synthetic:
            assert float(ref.max() - ref.min()) > 1e-3 * float(ref.mean())   # not the degenerate constant


def test_multi_head_route_picks_the_voted_configuration_by_a_device_index(multi):
    """head_forward without a renderer (the route's own code with the two kernels as their ATen statements) in float32 against the stock module, for a batch voted nyu
    and one voted kitti (the classifier's last bias forces the vote): the error against the stock module in float64 is held to the project's bar, max(2.5 x the stock
    float32 module's own error, 2^-21 of the magnitude)."""
    from visiondepth3d_amd import zoedepth
    outs = []
    for which in (0, 1):
        m = copy.deepcopy(multi)
        cases.force_domain(m, which)
        inp = cases.head_inputs(m, 3, 64, 96, seed=9)
        ref64, _ = _stock64(m.metric_head, inp)
        with torch.no_grad():
            ref32, logits32 = m.metric_head(*inp)
            got, logits, index = zoedepth.head_forward(m.metric_head, zoedepth._HeadWeights(m.metric_head), *inp)
        assert isinstance(index, torch.Tensor) and index.dtype == torch.int64 and index.tolist() == [which]
        assert int(torch.argmax(logits32.sum(0))) == which and torch.equal(logits, logits32)
        scale = float(ref64.abs().max())
        e_route, e_stock = float((got.double() - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
        print("ZOE_MULTI_ROUTE_CPU", dict(domain=which, route_err=e_route, stock_f32_err=e_stock, scale=scale))
        assert e_route <= max(2.5 * e_stock, 2.0 ** -21 * scale)
        outs.append(got)
    assert not torch.allclose(outs[0], outs[1], rtol=1e-3)   # the two configurations are different networks


def _scope(model, **attrs):
    from visiondepth3d_amd.depth import DepthPipe
    pipe = DepthPipe.__new__(DepthPipe)
    pipe.name, pipe.model, pipe.arch, pipe.gemm, pipe.self_contained = "probe", model, "zoedepth", "bf16x3", False
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe._split_scope()


def test_refusals_name_the_model(multi):
    from visiondepth3d_amd import zoedepth
    from visiondepth3d_amd.depth import DepthPipe
    with pytest.raises(NotImplementedError, match=r"gemm='fp16x2': 'probe' \(ZoeDepthForDepthEstimation\).*BEiT.*not built"):
        _scope(multi, gemm="fp16x2")
    with pytest.raises(NotImplementedError, match=r"self_contained=True: 'probe' \(ZoeDepthForDepthEstimation\).*not built"):
        _scope(multi, self_contained=True)
    with pytest.raises(NotImplementedError, match=r"front_end='pil': 'zoe' \(ZoeDepthForDepthEstimation\)"):
        DepthPipe("zoe", device="cpu", model=multi, processor=cases.TINY_PROCESSOR, front_end="pil")
    from visiondepth3d_amd import depth_pro
    with pytest.raises(NotImplementedError, match=r"encoders='bf16x3': 'zoe' \(ZoeDepthForDepthEstimation\)"):
        depth_pro.encoders_scope(multi, "zoe", "bf16x3", None)
    with pytest.raises(ValueError, match="decoder='bf16x3' needs encoders"):
        DepthPipe("zoe", device="cpu", model=multi, processor=cases.TINY_PROCESSOR, decoder="bf16x3")
    p = DepthPipe("zoe", device="cpu", model=copy.deepcopy(multi), processor=cases.TINY_PROCESSOR)
    with pytest.raises(NotImplementedError, match="flops_per_frame.*ZoeDepthForDepthEstimation"):
        p.flops_per_frame(135, 241)
    p.renderer = object()   # (the tiler asks for a renderer first)
    with pytest.raises(NotImplementedError, match="tiled depth: 'zoe' \\(ZoeDepthForDepthEstimation\\).*reflect padding"):
        p.infer_tiled_bgr_u8(cases.frames(1, 45, 61))
    # the head route's scope
    zoedepth.head_scope(multi, "zoe")
    with pytest.raises(NotImplementedError, match="bin_centers_type='normed'.*sorts"):
        zoedepth.head_scope(cases.tiny_model(False, synthetic=False, bin_centers_type="normed"), "zoe")
    bad = copy.deepcopy(multi)
    object.__setattr__(bad.config, "attractor_kind", "max")   # (the configuration class validates the field; a checkpoint from elsewhere need not)
    with pytest.raises(NotImplementedError, match="attractor_kind='max'"):
        zoedepth.head_scope(bad, "zoe")
    with pytest.raises(NotImplementedError, match="260 bins"):
        zoedepth.head_scope(cases.tiny_model(False, synthetic=False, bin_configurations=[dict(n_bins=260, min_depth=1e-3, max_depth=10.0)]), "zoe")
    with pytest.raises(NotImplementedError, match="62 bins"):
        zoedepth.head_scope(cases.tiny_model(False, synthetic=False, bin_configurations=[dict(n_bins=62, min_depth=1e-3, max_depth=10.0)]), "zoe")
    with pytest.raises(NotImplementedError, match=r"bin configurations of \[64, 32\] bins"):
        zoedepth.head_scope(cases.tiny_model(True, synthetic=False, bin_configurations=[dict(name="a", n_bins=64, min_depth=1e-3, max_depth=10.0),
                                                                                         dict(name="b", n_bins=32, min_depth=1e-3, max_depth=80.0)]), "zoe")
    with pytest.raises(NotImplementedError, match="hidden channels"):
        zoedepth.head_scope(cases.tiny_model(False, synthetic=False, bin_embedding_dim=512), "zoe")
    with pytest.raises(NotImplementedError, match="num_attractors"):
        zoedepth.head_scope(cases.tiny_model(False, synthetic=False, num_attractors=[32, 8, 4, 1]), "zoe")
    with pytest.raises(NotImplementedError, match="ZoeDepthForDepthEstimation"):
        zoedepth.head_scope(torch.nn.Linear(1, 1), "other")
    with pytest.raises(KeyError):
        zoedepth.zoe_switch("VD3D_NECK_GLUE")


def test_a_refused_head_keeps_the_stock_module(monkeypatch):
    """Without a renderer, in bfloat16, with VD3D_ZOE_HEAD=0 or for a model head_scope refuses, route_head leaves metric_head.forward alone and says why."""
    from types import SimpleNamespace

    from visiondepth3d_amd import zoedepth
    m = cases.tiny_model(False, synthetic=False, bin_centers_type="normed")
    pipe = SimpleNamespace(model=m, name="zoe", renderer=object(), dtype=torch.float32)
    zoedepth.route_head(pipe)
    assert "forward" not in m.metric_head.__dict__ and pipe.zoe_routes["metric_head"].startswith("stock: zoedepth head route: 'zoe'") and pipe.zoe_domain is None
    m = cases.tiny_model(True, synthetic=False)
    monkeypatch.setenv("VD3D_ZOE_HEAD", "0")
    pipe = SimpleNamespace(model=m, name="zoe", renderer=object(), dtype=torch.float32)
    zoedepth.route_head(pipe)
    assert "forward" not in m.metric_head.__dict__ and pipe.zoe_routes == {"metric_head": "stock: VD3D_ZOE_HEAD=0"}
    monkeypatch.delenv("VD3D_ZOE_HEAD")
    pipe = SimpleNamespace(model=m, name="zoe", renderer=object(), dtype=torch.bfloat16)
    zoedepth.route_head(pipe)
    assert "forward" not in m.metric_head.__dict__ and "float32" in pipe.zoe_routes["metric_head"]


def test_from_pretrained_round_trip(tmp_path, single):
    from visiondepth3d_amd import zoedepth
    from visiondepth3d_amd.depth import DepthPipe
    d = tmp_path / "zoedepth-tiny"
    single.save_pretrained(str(d))
    pc = dict(do_resize=True, do_rescale=True, do_normalize=True, do_pad=True, resample=2, keep_aspect_ratio=True, ensure_multiple_of=32, size=dict(height=64, width=96),
              image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
    (d / "preprocessor_config.json").write_text(json.dumps(pc))
    p = DepthPipe.from_pretrained(str(d), device="cpu")
    assert p.arch == "zoedepth" and p.proc == dict(cases.TINY_PROCESSOR)
    fr = cases.frames(1, 45, 61, 21)
    with torch.no_grad():
        pred = single(pixel_values=zoedepth.preprocess_statement(fr, cases.TINY_PROCESSOR)).predicted_depth
    assert torch.equal(p.infer_bgr_u8(fr)[0], cases.post_process_in_torch(pred, [(45, 61)])[0])
    # a file that gives no multiple: the CLASS default, 1 / 32; do_pad False is read
    (d / "preprocessor_config.json").write_text(json.dumps({k: v for k, v in dict(pc, do_pad=False).items() if k != "ensure_multiple_of"}))
    p = DepthPipe.from_pretrained(str(d), device="cpu")
    assert p.proc["multiple"] == 1 / 32 and p.proc["pad"] is False
    # any other ZoeDepth processor is refused by name
    (d / "preprocessor_config.json").write_text(json.dumps(dict(pc, resample=3)))
    with pytest.raises(NotImplementedError, match="ZoeDepth image processor"):
        DepthPipe.from_pretrained(str(d), device="cpu")
    (d / "preprocessor_config.json").write_text(json.dumps(dict(pc, do_normalize=False)))
    with pytest.raises(NotImplementedError, match="ZoeDepth image processor"):
        DepthPipe.from_pretrained(str(d), device="cpu")
