"""GPU tests (-m gpu) of the Pillow-exact depth front end (csrc/vd3d_pilresample.hip, DepthPipe(front_end="pil")).  Everything up to the network input is
an equality: the uint8 form against the integer statement (visiondepth3d_amd/pil_resample.py) and against Pillow itself, the fused form against
transformers' DPTImageProcessor on the PIL image, the self-contained forward against the same network on the processor's values.  The default float32 mode is
held to the uint8-plane bar of tests/test_hip_depth_e2e.py against the reference chain (the transformers pipeline on the CPU, then depth_to_u8)."""
import numpy as np
import pytest

from visiondepth3d_amd import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
Image = pytest.importorskip("PIL.Image")
transformers = pytest.importorskip("transformers")

# (input h, w), (output h, w), what it exercises
GEOMETRIES = [((54, 96), (26, 47), "non-integer down-scale"),
              ((37, 53), (70, 112), "up-scale"),
              ((40, 64), (80, 30), "mixed axes, both clamp ends"),
              ((33, 20), (33, 77), "horizontal pass only"),
              ((20, 33), (77, 33), "vertical pass only"),
              ((48, 48), (48, 48), "copy"),
              ((3, 5), (14, 14), "taps clipped at both borders at once"),
              ((300, 534), (70, 126), "19 taps, the 4K ratio"),
              ((64, 200), (31, 65), "output width one past a multiple of 32"),
              ((64, 64), (1, 1), "beyond any tap budget"),
              ((240, 40), (48, 40), "a band of 32 output rows would need 181 input rows: the band halves")]


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def proc():
    from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD
    return transformers.DPTImageProcessor(do_resize=True, size={"height": 518, "width": 518}, keep_aspect_ratio=True, ensure_multiple_of=14,
                                          resample=3, do_rescale=True, rescale_factor=1 / 255, do_normalize=True,
                                          image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD, do_pad=False)


def _three_frames(h, w, seed):
    """random bytes, binary 0 / 255, ramps -- behind a leading frame that is cut off, so that the frames start at whatever byte the sizes give"""
    rng = np.random.default_rng(seed)
    a = np.empty((4, h, w, 3), np.uint8)
    a[0] = 0
    a[1] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[2] = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    a[3] = ((np.arange(h)[:, None, None] * 7 + np.arange(w)[None, :, None] * 3 + np.arange(3) * 50) % 256).astype(np.uint8)
    return a


@pytest.mark.parametrize("src,dst,what", GEOMETRIES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d, _ in GEOMETRIES])
def test_u8_form_equals_the_statement_and_pillow(R, src, dst, what):
    from visiondepth3d_amd import pil_resample
    (H, W), (h, w) = src, dst
    a = _three_frames(H, W, H * 1000 + w)
    frames = torch.from_numpy(a).cuda()[1:]
    got = R.resize_pil_bicubic_u8(frames, h, w)
    assert R.pil_route == ("statement" if (h, w) == (1, 1) else "kernel"), what
    assert got.shape == (3, h, w, 3) and got.dtype == torch.uint8
    assert torch.equal(got, pil_resample.resize(frames, w, h)), what
    pil = np.stack([np.asarray(Image.fromarray(a[i]).resize((w, h), Image.BICUBIC)) for i in (1, 2, 3)])
    assert np.array_equal(got.cpu().numpy(), pil), what
    one = R.resize_pil_bicubic_u8(frames[2], h, w)   # a single frame comes back as one
    assert one.shape == (h, w, 3) and torch.equal(one, got[2])


def _frames_and_images(h, w, n=2):
    bgr = np.stack([synth.synth_frame(i, h, w)[0] for i in range(n)])
    return torch.from_numpy(bgr).cuda(), [Image.fromarray(f[..., ::-1].copy()) for f in bgr]


@pytest.mark.parametrize("h,w", [(135, 240), (270, 480)])
def test_fused_form_equals_the_image_processor(R, proc, h, w):
    from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD, dpt_resize_target
    frames, imgs = _frames_and_images(h, w)
    exp = proc(images=imgs, return_tensors="pt")["pixel_values"]
    th, tw = dpt_resize_target(h, w)
    R.set_profiling(True)
    got = R.depth_preprocess_pil(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.float32)
    assert R.stage_calls("depth_prep_pil") == 1 and R.pil_route == "kernel"
    R.set_profiling(False)
    assert got.shape == exp.shape and got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got.cpu(), exp)
    got16 = R.depth_preprocess_pil(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.bfloat16)
    assert got16.dtype == torch.bfloat16 and got16.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got16.cpu(), exp.to(torch.bfloat16))
    # the depth tab's inference size: img.resize((112, 70), BICUBIC) first
    exp2 = proc(images=[im.resize((112, 70), Image.BICUBIC) for im in imgs], return_tensors="pt")["pixel_values"]
    th2, tw2 = dpt_resize_target(70, 112)
    R.set_profiling(True)
    got2 = R.depth_preprocess_pil(frames, th2, tw2, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.float32, inference_size=(112, 70))
    assert R.stage_calls("depth_prep_pil") == 2 and R.pil_route == "kernel"
    R.set_profiling(False)
    assert got2.shape == exp2.shape and got2.is_contiguous(memory_format=torch.channels_last) and torch.equal(got2.cpu(), exp2)
    got2h = R.depth_preprocess_pil(frames, th2, tw2, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.bfloat16, inference_size=(112, 70))
    assert torch.equal(got2h.cpu(), exp2.to(torch.bfloat16))


def test_fused_form_past_the_tap_budget_runs_the_statement(R, proc):
    """168 x 300 -> the inference size 14 x 28 is a 10.7- and 12-fold down-scale (up to 49 taps): the entry point refuses both launches, the statement gives
    the processor's values all the same."""
    from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD
    frames, imgs = _frames_and_images(168, 300, 1)
    exp = proc(images=[imgs[0].resize((28, 14), Image.BICUBIC)], return_tensors="pt")["pixel_values"]
    got = R.depth_preprocess_pil(frames, exp.shape[2], exp.shape[3], IMAGENET_MEAN, IMAGENET_STD, inference_size=(28, 14))
    assert R.pil_route == "statement"
    assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(got.cpu(), exp)


def test_whole_forward_is_the_network_on_the_processors_values(R, proc, monkeypatch):
    """The self-contained bf16x3 mode repeats bit for bit, so with the reference's pixel values the whole forward is an equality."""
    import torch.nn.functional as F
    from visiondepth3d_amd.depth import DepthPipe
    frames, imgs = _frames_and_images(135, 240)
    pipe = DepthPipe("depth-anything-v2-small", gemm="bf16x3", conv="bf16x3", self_contained=True, front_end="pil", renderer=R)
    pv = proc(images=imgs, return_tensors="pt")["pixel_values"].cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        exp = pipe.model(pixel_values=pv).predicted_depth
        small = [im.resize((112, 70), Image.BICUBIC) for im in imgs]
        pv2 = proc(images=small, return_tensors="pt")["pixel_values"].cuda().contiguous(memory_format=torch.channels_last)
        exp2 = pipe.model(pixel_values=pv2).predicted_depth
    resizes = []
    real = F.interpolate

    def spy(x, *a, **kw):
        if kw.get("antialias") or kw.get("mode") == "bicubic":
            resizes.append(kw)
        return real(x, *a, **kw)
    monkeypatch.setattr(F, "interpolate", spy)
    R.set_profiling(True)
    got = pipe.infer_bgr_u8(frames, raw=True)
    assert R.stage_calls("depth_prep_pil") == 1 and R.stage_calls("depth_prep") == 0 and pipe.front_end_route == "kernel"
    R.set_profiling(False)
    assert torch.equal(got, exp)
    R.set_profiling(True)
    got2 = pipe.infer_bgr_u8(frames, inference_size=(112, 70), raw=True)
    assert R.stage_calls("depth_prep_pil") == 2 and R.stage_calls("depth_prep") == 0
    R.set_profiling(False)
    assert torch.equal(got2, exp2)
    assert not resizes   # no ATen resize in front of the network
    full = pipe.infer_bgr_u8(frames, inference_size=(112, 70), at_inference_size=True)
    assert full.shape == (2, 70, 112)
    assert pipe.infer_bgr_u8(frames).shape == (2, 135, 240)


def test_default_f32_mode_against_the_reference_chain(R, proc):
    """depth_frames_u8 of the default float32 mode with front_end="pil" against the reference chain -- the transformers pipeline on the CPU with the same
    weights, then depth_to_u8 -- at 126 x 224, on the uint8 bar of tests/test_hip_depth_e2e.py: >= 99.5 % of the bytes identical, none off by more than one."""
    from visiondepth3d_amd.depth import DepthPipe, build_config, depth_to_u8, synthetic_weights_
    frames, imgs = _frames_and_images(126, 224)
    model = transformers.DepthAnythingForDepthEstimation(build_config("depth-anything-v2-small")).eval()
    synthetic_weights_(model, 0)
    hf = transformers.pipeline("depth-estimation", model=model, image_processor=proc, device="cpu")
    exp = torch.stack([depth_to_u8(o["predicted_depth"].squeeze()[None])[0] for o in hf(imgs)])
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R, front_end="pil")
    got = pipe.depth_frames_u8(frames).cpu()
    assert pipe.front_end_route == "kernel" and got.shape == exp.shape == (2, 126, 224) and got.dtype == torch.uint8
    d = (got.to(torch.int16) - exp.to(torch.int16)).abs()
    exact, worst = float((d == 0).float().mean()), int(d.max())
    print(f"front_end='pil', default f32 mode against the reference chain: {exact * 100:.3f} % of the bytes identical, largest difference {worst}")
    assert exact >= 0.995 and worst <= 1, (exact, worst)
