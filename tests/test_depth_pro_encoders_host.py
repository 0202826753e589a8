"""DepthPipe(encoders=...) without a GPU: every refusal of the keyword, by message, raised at construction before the module is moved to a device; and
``encoders=None`` builds exactly the pipe there was before the keyword.  ``renderer=object()``, ``device="cuda"``: any use of the renderer, and any move to the
(absent) GPU, would raise something else than the refusal."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import depth_pro_cases as cases   # noqa: E402
from visiondepth3d_amd.depth import DepthPipe   # noqa: E402

ON = dict(device="cuda", renderer=object(), tuned_gemm=False)


def _mini(**over):
    return cases.build(cases.mini_config(**over))


def _refused(exc, match, model, processor=None, **kw):
    with pytest.raises(exc, match=match):
        DepthPipe("mini", model=model, processor=cases.mini_processor() if processor is None else processor, **dict(ON, **kw))
    if model is not None:
        assert {p.device.type for p in model.parameters()} == {"cpu"}   # refused before the module was moved to a device


@pytest.mark.parametrize("mode", ["bf16x3", "fp16x2"])
def test_arguments_are_refused_by_name(mode):
    m = _mini()
    _refused(ValueError, r"encoders must be None, 'bf16x3' or 'fp16x2'", m, encoders="f32")
    with pytest.raises(ValueError, match=r"encoders='bf16x3' / 'fp16x2' are modes of the float32 pipe on the GPU and need a renderer"):
        DepthPipe("mini", model=m, processor=cases.mini_processor(), device="cuda", tuned_gemm=False, encoders=mode)
    with pytest.raises(ValueError, match=r"need a renderer"):
        DepthPipe("mini", model=m, processor=cases.mini_processor(), device="cpu", renderer=object(), encoders=mode)
    _refused(ValueError, r"need a renderer", m, encoders=mode, dtype=torch.bfloat16)
    # together with gemm= / self_contained=True the existing messages win, unchanged
    _refused(NotImplementedError, rf"gemm='{mode}': 'mini' \(DepthProForDepthEstimation\).*not built", m, encoders=mode, gemm=mode)
    _refused(NotImplementedError, r"self_contained=True: 'mini' \(DepthProForDepthEstimation\).*not built", m, encoders=mode, gemm=mode, conv=mode, self_contained=True)
    _refused(ValueError, r"self_contained=True needs ", m, encoders=mode, self_contained=True)


def test_another_model_is_refused_by_name():
    with pytest.raises(NotImplementedError, match=r"encoders='bf16x3': 'depth-anything-v2-small' \(DepthAnythingForDepthEstimation\) -- the keyword routes the three ViT "
                                                  r"encoders of DepthProForDepthEstimation"):
        DepthPipe("depth-anything-v2-small", encoders="bf16x3", **ON)


@pytest.mark.parametrize("which,key", [("patch", "patch_model_config"), ("image", "image_model_config"), ("fov", "fov_model_config")])
def test_encoders_outside_the_kernels_sizes_are_refused_by_name(which, key):
    _refused(NotImplementedError, rf"encoders='fp16x2': 'mini' \(DepthProForDepthEstimation\): the {which} encoder has hidden size 128 with 4 heads.*64-wide heads",
             _mini(**{key: dict(cases.encoder(64), hidden_size=128, num_attention_heads=4)}), encoders="fp16x2")
    vit = dict(model_type="vit", hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=1536, image_size=64, patch_size=16)
    _refused(NotImplementedError, rf"the {which} encoder is a ViTModel -- _split_block is built for Dinov2Model encoders", _mini(**{key: vit}), encoders="bf16x3")


def test_geometries_outside_the_two_kernels_are_refused_by_name():
    _refused(NotImplementedError, r"scaled_images_ratios=\[0.125, 0.5, 1\] -- vd3d_depthpro_patches_f32 builds the pyramid of \[0.25, 0.5, 1\]",
             _mini(scaled_images_ratios=[0.125, 0.5, 1]), encoders="bf16x3")
    m = _mini()
    _refused(NotImplementedError, r"a processor size of \(258, 258\) -- the pyramid kernel takes a square side that is a multiple of 4", m,
             processor=dict(cases.mini_processor(), size=(258, 258)), encoders="bf16x3")
    _refused(NotImplementedError, r"a processor size of \(256, 128\)", m, processor=dict(cases.mini_processor(), size=(256, 128)), encoders="bf16x3")
    _refused(NotImplementedError, r"a pyramid vd3d_depthpro_patches_f32 is not built for -- depth-pro: a 128 x 128 image scaled by 0.25 is smaller than the 64 x 64 patch", m,
             processor=dict(cases.mini_processor(), size=(128, 128)), encoders="bf16x3")
    pe = m.depth_pro.encoder.image_encoder.model.embeddings.patch_embeddings
    pe.projection = torch.nn.Conv2d(3, 384, kernel_size=16, stride=8)
    _refused(NotImplementedError, r"the image encoder's patch embedding is not Conv2d\(3, C, kernel_size=p, stride=p\), p <= 64 -- vd3d_patchify_f32 does not take it", m,
             encoders="bf16x3")


def test_encoders_none_builds_the_pipe_as_it_was():
    m = _mini()
    pipe = DepthPipe("mini", model=m, processor=cases.mini_processor(), device="cpu")
    assert pipe.encoders is None and pipe.encoders_resize == {} and pipe.gemm == "f32" and pipe.arch == "depth_pro"
    enc = pipe.model.depth_pro.encoder
    for mod in (enc.patch_encoder, enc.image_encoder, pipe.model.fov_model.fov_encoder, *enc.patch_encoder.model.encoder.layer):
        assert "forward" not in vars(mod)   # the stock graph: no forward replaced
    x = cases.processor_in_torch(cases.frames(1, 40, 56, 3), 256)
    with torch.no_grad():
        a, b = pipe.model(pixel_values=x), _mini()(pixel_values=x)
    assert torch.equal(a.predicted_depth, b.predicted_depth) and torch.equal(a.field_of_view, b.field_of_view)
