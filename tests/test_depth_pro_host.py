"""Host-only tests of the DepthPro entry of DepthPipe (apple/DepthPro-hf, DepthProForDepthEstimation): the zoo entry, the refusals raised before a device is
touched, the CPU pipe against the image processor restated in torch + the stock module + the processor's post-process, and the NumPy statements of the patch
pyramid and the patch merge (visiondepth3d_amd/depth_pro.py) against transformers' own split_to_patches / merge_patches / reconstruct_feature_maps."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
import torch.nn.functional as F   # noqa: E402

import depth_pro_cases as cases   # noqa: E402

NAME = "depth-pro"


def test_zoo_entry_builds_the_published_geometry():
    from visiondepth3d_amd.depth import MODEL_ZOO, PROCESSORS, build_config
    assert MODEL_ZOO[NAME]["arch"] == "depth_pro"        # (a KeyError before DepthPro was added)
    c = build_config(NAME)
    assert type(c).__name__ == "DepthProConfig" and (c.patch_size, c.fusion_hidden_size) == (384, 256)
    assert list(c.intermediate_hook_ids) == [11, 5] and list(c.intermediate_feature_dims) == [256, 256]
    assert list(c.scaled_images_ratios) == [0.25, 0.5, 1] and list(c.scaled_images_overlap_ratios) == [0.0, 0.5, 0.25]
    assert list(c.scaled_images_feature_dims) == [1024, 1024, 512] and c.merge_padding_value == 3 and c.use_fov_model is True and c.num_fov_head_layers == 2
    for e in (c.image_model_config, c.patch_model_config, c.fov_model_config):
        assert (e.model_type, e.hidden_size, e.num_hidden_layers, e.num_attention_heads, e.image_size, e.patch_size, e.use_mask_token) == ("dinov2", 1024, 24, 16, 384, 16, False)
    assert PROCESSORS["depth_pro"] == dict(size=(1536, 1536), keep_aspect_ratio=False, multiple=1, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), resample=2)
    from visiondepth3d_amd import depth_pro
    lv = depth_pro.pyramid_levels(1536, 384)
    assert [(s, st, n) for _, s, st, n in lv] == [(384, 384, 1), (768, 192, 3), (1536, 288, 5)] and sum(n * n for *_, n in lv) == 35


@pytest.fixture(scope="module")
def mini():
    return cases.build(cases.mini_config())


@pytest.fixture(scope="module")
def pipe(mini):
    from visiondepth3d_amd.depth import DepthPipe
    return DepthPipe("mini-depth-pro", device="cpu", model=mini, processor=cases.mini_processor())


def _expected(model, fr, sizes):
    x = cases.processor_in_torch(fr, 256)
    with torch.no_grad():
        out = model(pixel_values=x)
    return out, cases.post_process_in_torch(out.predicted_depth, out.field_of_view, sizes)


def test_cpu_pipe_is_the_processor_the_stock_module_and_the_post_process_bit_for_bit(pipe, mini):
    """The expectation's two ends (depth_pro_cases.processor_in_torch / post_process_in_torch) are restatements of the processor's lines written for the tests,
    because its class cannot be imported without torchvision; the package's own statements (depth_pro.preprocess_statement / post_statement) are written from
    the same lines, so this test compares near copies around the stock module.  What it does establish: the pipe routes DepthPro to that order (normalise,
    bilinear without antialias, the reciprocal last) at the sizes the pipeline sees, and not to the bicubic path of every other model."""
    fr = cases.frames(2, 135, 241, 11)
    out, exp = _expected(mini, fr, [(135, 241)] * 2)
    assert pipe.arch == "depth_pro" and out.field_of_view is not None
    got = pipe.infer_bgr_u8(fr)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 135, 241)
    for b in range(2):
        assert torch.equal(got[b], exp[b]), b
    # the reciprocal is there: the pipeline's value is an inverse depth between 1e-4 and 1e4
    assert float(got.min()) >= 0.99e-4 and float(got.max()) <= 1.01e4
    # raw: the model-resolution inverse depth -- the scale for the model's own width, no resize
    raw = pipe.infer_bgr_u8(fr, raw=True)
    for b in range(2):
        focal = 0.5 * 256 / torch.tan(0.5 * torch.deg2rad(out.field_of_view[b]))
        assert torch.equal(raw[b], 1.0 / torch.clamp(out.predicted_depth[b] * 256 / focal, min=1e-4, max=1e4))
    # the reference protocol: RGB arrays in, a list of dicts out, at the size the pipeline saw
    rgb = np.ascontiguousarray(fr[0].numpy()[..., ::-1])
    res = pipe([rgb])
    assert torch.equal(res[0]["predicted_depth"], _expected(mini, fr[:1], [(135, 241)])[1][0])   # (one image per forward, as the protocol runs it)
    # depth_frames_u8: the reference min-max normalises the inverse depth
    from visiondepth3d_amd.depth import depth_to_u8
    assert torch.equal(pipe.depth_frames_u8(fr), depth_to_u8(torch.stack(exp)))


def test_cpu_pipe_with_an_inference_size(pipe, mini):
    """hf_batch_safe_pipe resizes the image first; the pipe's float statement of that resize feeds the processor and the post-process targets the inference size."""
    fr = cases.frames(1, 90, 160, 12)
    pre = F.interpolate(fr.flip(-1).permute(0, 3, 1, 2).float(), size=(54, 96), mode="bicubic", antialias=True, align_corners=False).clamp_(0, 255)
    x = F.interpolate((pre - 127.5) / 127.5, size=(256, 256), mode="bilinear", align_corners=False, antialias=False)
    with torch.no_grad():
        out = mini(pixel_values=x)
    exp = cases.post_process_in_torch(out.predicted_depth, out.field_of_view, [(54, 96)])[0]
    assert torch.equal(pipe.infer_bgr_u8(fr, inference_size=(96, 54), at_inference_size=True)[0], exp)
    assert tuple(pipe.infer_bgr_u8(fr, inference_size=(96, 54)).shape) == (1, 90, 160)


def test_a_model_without_the_field_of_view_branch_is_not_scaled():
    from visiondepth3d_amd.depth import DepthPipe
    m = cases.build(cases.mini_config(use_fov_model=False), seed=4)
    p = DepthPipe("mini-depth-pro-nofov", device="cpu", model=m, processor=cases.mini_processor())
    fr = cases.frames(1, 64, 80, 13)
    out, exp = _expected(m, fr, [(64, 80)])
    assert out.field_of_view is None and torch.equal(p.infer_bgr_u8(fr)[0], exp[0])


def _scope(model, **attrs):
    from visiondepth3d_amd.depth import DepthPipe
    pipe = DepthPipe.__new__(DepthPipe)
    pipe.name, pipe.model, pipe.arch, pipe.gemm, pipe.self_contained = "probe", model, "depth_pro", "bf16x3", False
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe._split_scope()


def test_refusals_name_the_model(mini, pipe):
    from visiondepth3d_amd.depth import DepthPipe
    # the split modes and self_contained=True: the rewrite is not built; the refusal reads the module graph only
    with pytest.raises(NotImplementedError, match=r"gemm='fp16x2': 'probe' \(DepthProForDepthEstimation\).*not built"):
        _scope(mini, gemm="fp16x2")
    with pytest.raises(NotImplementedError, match=r"self_contained=True: 'probe' \(DepthProForDepthEstimation\).*not built"):
        _scope(mini, self_contained=True)
    # front_end="pil": this processor has no Pillow pass
    with pytest.raises(NotImplementedError, match=r"front_end='pil': 'mini' \(DepthProForDepthEstimation\)"):
        DepthPipe("mini", device="cpu", model=mini, processor=cases.mini_processor(), front_end="pil")
    with pytest.raises(NotImplementedError, match="flops_per_frame.*DepthProForDepthEstimation"):
        pipe.flops_per_frame(135, 241)


def test_from_pretrained_takes_bilinear_for_depth_pro_only(tmp_path, mini):
    from visiondepth3d_amd.depth import DepthPipe
    d = tmp_path / "DepthPro-mini"
    mini.save_pretrained(str(d))
    pc = dict(do_resize=True, do_rescale=True, do_normalize=True, resample=2, size=dict(height=256, width=256), image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
    (d / "preprocessor_config.json").write_text(json.dumps(pc))
    p = DepthPipe.from_pretrained(str(d), device="cpu")
    assert p.arch == "depth_pro" and p.proc["size"] == (256, 256) and p.proc["resample"] == 2 and not p.proc["keep_aspect_ratio"]
    fr = cases.frames(1, 50, 70, 14)
    out, exp = _expected(mini, fr, [(50, 70)])
    assert torch.equal(p.infer_bgr_u8(fr)[0], exp[0])
    (d / "preprocessor_config.json").write_text(json.dumps(dict(pc, resample=3)))
    with pytest.raises(NotImplementedError, match="DepthPro image processor"):
        DepthPipe.from_pretrained(str(d), device="cpu")
    # any other model: bilinear is refused as before
    t = tmp_path / "dpt-tiny"
    cfg = transformers.DPTConfig(hidden_size=64, num_hidden_layers=4, num_attention_heads=2, intermediate_size=128, image_size=32, patch_size=16,
                                 backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[16, 16, 16, 16], fusion_hidden_size=16, readout_type="project")
    transformers.DPTForDepthEstimation(cfg).save_pretrained(str(t))
    (t / "preprocessor_config.json").write_text(json.dumps(dict(resample=2, size=dict(height=32, width=32))))
    with pytest.raises(NotImplementedError, match="other than bicubic"):
        DepthPipe.from_pretrained(str(t), device="cpu")


# ---------------------------------------------------------------------------------------------------------------- the NumPy statements
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S,p", [(256, 64), (1536, 384)])
def test_patch_statement_is_split_to_patches(B, S, p):
    """Order and geometry: pixels carry their own (b, c, y, x), so a wrong patch order cannot pass.  The ratio-1 level is bit-equal; on the two scaled levels all
    four weights are exactly 0.25 and every product is exact, so ATen and the statement can differ only in the order of a four-term sum:
    |a - b| <= 6 * 2^-24 * 0.25 * sum |x_i|."""
    from transformers.models.depth_pro import modeling_depth_pro as M
    from visiondepth3d_amd import depth_pro
    b, c, y, x = np.meshgrid(np.arange(B), np.arange(3), np.arange(S), np.arange(S), indexing="ij")
    img = (((b * 3 + c) * S + y) * S + x).astype(np.float32) * np.float32(1.0 / 1024) + np.float32(0.37) * ((y * 7 + x * 3) % 11).astype(np.float32)
    xt = torch.from_numpy(img)
    lv = [M.split_to_patches(F.interpolate(xt, scale_factor=r, mode="bilinear", align_corners=False), p, o) for r, o in zip((0.25, 0.5, 1), (0.0, 0.5, 0.25))]
    ref = torch.cat(lv[::-1], 0).numpy()
    got = depth_pro.patches_statement(img, p)
    assert got.shape == ref.shape == (35 * B, 3, p, p)
    n1 = 25 * B
    assert np.array_equal(got[:n1], ref[:n1])
    a = np.abs(img)
    s2 = a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2]
    s4 = a[..., 1::4, 1::4] + a[..., 1::4, 2::4] + a[..., 2::4, 1::4] + a[..., 2::4, 2::4]
    # sum |x_i| in the patches' own order: the half level of the 2 x 2-repeated sums is the sums themselves (exact), the quarter level is one patch per frame
    half = depth_pro.patches_statement(np.repeat(np.repeat(s2, 2, -1), 2, -2), p)[n1:n1 + 9 * B]
    bound = np.concatenate([half, s4]) * (6 * cases.U * 0.25)
    assert bool((np.abs(got[n1:] - ref[n1:]) <= bound).all()), float(np.abs(got[n1:] - ref[n1:]).max())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("g", [4, 24])
def test_merge_statement_is_reconstruct_feature_maps(B, g):
    """Rows carry their own (sequence, token, channel).  Bit-equal wherever the resize is the identity; where it is not, within cases.bilinear_bound."""
    from transformers.models.depth_pro import modeling_depth_pro as M
    from visiondepth3d_amd import depth_pro
    C = 8
    for n, padding in ((35, 3), (25, 3), (25, 6), (9, 6), (9, 3), (4, 3), (3, 3), (1, 0)):
        s, t, c = np.meshgrid(np.arange(n * B), np.arange(1 + g * g), np.arange(C), indexing="ij")
        rows = ((s * (1 + g * g) + t) * C + c).astype(np.float32) * np.float32(0.001) + np.float32(0.5) * ((t * 5 + c) % 7).astype(np.float32)
        side, pad, Mm = depth_pro.merge_geometry(n, g, padding)
        assert pad == (0 if n < 4 else min(g // 4, padding)) and Mm == side * g - 2 * pad * (side - 1)
        for o in (Mm, Mm + Mm // 3, 2 * Mm - 3):
            ref = M.reconstruct_feature_maps(torch.from_numpy(rows), B, padding, (o, o)).permute(0, 2, 3, 1).numpy()
            got = depth_pro.merge_statement(rows, B, g, padding, o, o)
            assert got.shape == ref.shape == (B, o, o, C)
            if o == Mm:
                assert np.array_equal(got, ref), (n, padding, o)
            else:
                lim = cases.bilinear_bound(float(np.abs(rows).max()), float(rows.max() - rows.min()), Mm, Mm)
                assert float(np.abs(got - ref).max()) <= lim, (n, padding, o, float(np.abs(got - ref).max()), lim)
    # MINI's and the published model's own numbers
    assert depth_pro.merge_geometry(25, 4, 3) == (5, 1, 12) and depth_pro.merge_geometry(9, 4, 6) == (3, 1, 8)
    assert depth_pro.merge_geometry(35, 24, 3) == (5, 3, 96) and depth_pro.merge_geometry(9, 24, 6) == (3, 6, 48) and depth_pro.merge_geometry(1, 24, 12) == (1, 0, 24)
