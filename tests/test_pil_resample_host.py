"""The integer statement of the reference's 8-bit input path (visiondepth3d_amd/pil_resample.py) against what it states, on the CPU: Pillow's own
``Image.resize(size, Image.BICUBIC)``, transformers' ``DPTImageProcessor`` and, through ``DepthPipe(front_end="pil")``, the transformers depth pipeline.
The first two are equalities; the third is the existing bar for two module graphs on identical pixel values (tests/test_host_logic.py: 1e-4)."""
import numpy as np
import pytest
import torch

Image = pytest.importorskip("PIL.Image")
transformers = pytest.importorskip("transformers")

from visiondepth3d_amd import pil_resample, synth  # noqa: E402
from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD, DepthPipe, build_config, dpt_resize_target, synthetic_weights_  # noqa: E402

# (input h, w), (output h, w): the geometries tests/test_hip_pil_front_end.py runs on the GPU
NAMED = [((54, 96), (26, 47)), ((37, 53), (70, 112)), ((40, 64), (80, 30)), ((33, 20), (33, 77)), ((20, 33), (77, 33)), ((48, 48), (48, 48)),
         ((3, 5), (14, 14)), ((300, 534), (70, 126)), ((64, 200), (31, 65)), ((64, 64), (1, 1))]


def content(kind, rng, h, w):
    """0: random bytes, 1: binary 0 / 255 (both clamp ends), 2: ramps"""
    if kind % 3 == 0:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind % 3 == 1:
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return ((np.arange(h)[:, None, None] * 7 + np.arange(w)[None, :, None] * 3 + np.arange(3) * 50) % 256).astype(np.uint8)


def processor():
    return transformers.DPTImageProcessor(do_resize=True, size={"height": 518, "width": 518}, keep_aspect_ratio=True, ensure_multiple_of=14,
                                          resample=3, do_rescale=True, rescale_factor=1 / 255, do_normalize=True,
                                          image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD, do_pad=False)


def test_resize_equals_pillow_on_210_geometries():
    rng = np.random.default_rng(19)
    geos = list(NAMED) + [((int(rng.integers(1, 141)), int(rng.integers(1, 141))), (int(rng.integers(1, 141)), int(rng.integers(1, 141))))
                          for _ in range(200)]
    assert len(geos) == 210
    for i, ((H, W), (h, w)) in enumerate(geos):
        a = content(1 if i == 2 else i, rng, H, W)   # the kinds in rotation; the mixed-axes case is binary
        exp = np.asarray(Image.fromarray(a).resize((w, h), Image.BICUBIC))
        got = pil_resample.resize(torch.from_numpy(a), w, h).numpy()
        assert got.shape == exp.shape and np.array_equal(got, exp), ((H, W), (h, w), i % 3)


def test_resize_takes_batches_and_copies_at_equal_size():
    rng = np.random.default_rng(2)
    a = torch.from_numpy(rng.integers(0, 256, (2, 3, 17, 23, 3), dtype=np.uint8))
    got = pil_resample.resize(a, 40, 9)
    assert got.shape == (2, 3, 9, 40, 3)
    for i in range(2):
        for j in range(3):
            assert np.array_equal(got[i, j].numpy(), np.asarray(Image.fromarray(a[i, j].numpy()).resize((40, 9), Image.BICUBIC)))
    same = pil_resample.resize(a, 23, 17)
    assert torch.equal(same, a) and same.data_ptr() != a.data_ptr()
    with pytest.raises(TypeError):
        pil_resample.resize(a.float(), 4, 4)


def test_coefficients_are_what_the_issue_states():
    xmin, count, k = pil_resample.coeffs(3840, 924)
    assert k.shape == (924, 19) and xmin.shape == count.shape == (924,)   # Pillow's ksize = 2 ceil(support) + 1 = 19 at the 4K ratio
    assert int(count.max()) == 17 and not k[np.arange(19)[None, :] >= count[:, None]].any()   # 2 * 8.31 taps lie inside; past the count: zero
    assert (k.sum(1) - (1 << 22)).__abs__().max() <= 19             # every row sums to one in 22-bit fixed point, up to a rounding per tap
    assert np.abs(k).max() < (1 << 23)                               # a byte times a coefficient is a 24-bit multiply
    xmin, count, k = pil_resample.coeffs(5, 14)                      # up-scaling: support 2, taps clipped at both borders
    assert int(count.max()) <= 5 and int(xmin.min()) == 0 and int((xmin + count).max()) == 5


def test_pixel_values_equal_the_image_processor():
    proc = processor()
    lut = pil_resample.normalise_lut(IMAGENET_MEAN, IMAGENET_STD)
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    for i, (h, w) in enumerate([(135, 240), (270, 480), (70, 112), (600, 1100)]):
        bgr = synth.synth_frame(i, h, w)[0]
        exp = proc(images=Image.fromarray(bgr[..., ::-1].copy()), return_tensors="pt")["pixel_values"]
        th, tw = dpt_resize_target(h, w)
        got = pil_resample.pixel_values(torch.from_numpy(bgr)[None], th, tw, IMAGENET_MEAN, IMAGENET_STD).permute(0, 3, 1, 2)
        assert got.shape == exp.shape and got.dtype == exp.dtype and torch.equal(got, exp), (h, w)


def test_depth_pipe_pil_front_end_against_the_transformers_pipeline():
    """The images and the pipeline of test_depth_pipe_protocol_against_the_transformers_pipeline; with the reference's own pixel values what is left is the
    distance of the two module graphs (fused QKV, folded LayerScale), the 1e-4 of that test's first assertion -- the float front end needs 3e-2 / 5e-2."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    pipe = DepthPipe("depth-anything-v2-small", device="cpu", dtype=torch.float32, front_end="pil")
    model = transformers.DepthAnythingForDepthEstimation(build_config("depth-anything-v2-small")).eval()
    synthetic_weights_(model, 0)
    hf = transformers.pipeline("depth-estimation", model=model, image_processor=processor(), device="cpu")
    img = Image.fromarray(synth.synth_frame(1, 126, 224)[0][..., ::-1].copy())
    exp = hf([img])[0]["predicted_depth"].squeeze()
    got = pipe([img])[0]["predicted_depth"]
    assert pipe.front_end_route == "statement"
    assert tuple(got.shape) == tuple(exp.shape) == (126, 224)
    rel = float((got - exp).abs().max() / exp.abs().max())
    print("front_end='pil' against the pipeline, max relative difference:", rel)
    assert rel < 1e-4
    small = img.resize((112, 70), Image.BICUBIC)
    exp2 = hf([small])[0]["predicted_depth"].squeeze()
    got2 = pipe([img], inference_size=(112, 70))[0]["predicted_depth"]
    assert tuple(got2.shape) == tuple(exp2.shape) == (70, 112)
    rel2 = float((got2 - exp2).abs().max() / exp2.abs().max())
    print("... with inference_size=(112, 70):", rel2)
    assert rel2 < 1e-4


def test_front_end_keyword():
    with pytest.raises(ValueError):
        DepthPipe("depth-anything-v2-small", device="cpu", front_end="opencv")
    pipe = DepthPipe("depth-anything-v2-small", device="cpu")
    assert pipe.front_end == "float" and pipe.front_end_route is None
    pil = DepthPipe("depth-anything-v2-small", device="cpu", front_end="pil")
    with pytest.raises(TypeError):
        pil.infer_bgr_u8(torch.zeros(1, 28, 28, 3))
