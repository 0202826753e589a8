"""GPU test (-m gpu) of the fused depth-net input preparation (vd3d_depth_preprocess, boundary B3 / SURVEY a25) against
the plain PyTorch float32 statement of the same operator chain (antialiased bicubic resize -> 1/255 -> ImageNet
normalise).  Floating-point kernel: tolerance = bf16 rounding of the result (1/2 ulp = 2^-9 relative) plus the float32
association noise of the 2-D filter sums.  These are the loose checks on smooth frames; the kernel's bits are pinned on random bytes
against its NumPy statement in tests/test_hip_depthprep_bits.py, and the statement against float64 in tests/test_depthprep_host.py."""
import numpy as np
import pytest

from visiondepth3d_amd import synth
from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD, dpt_resize_target

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _ref(frames_u8, th, tw):
    import torch.nn.functional as F
    x = frames_u8.flip(-1).permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=(th, tw), mode="bicubic", antialias=True, align_corners=False)
    mean = torch.tensor(IMAGENET_MEAN, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=x.device).view(1, 3, 1, 1)
    return ((x / 255.0) - mean) / std


@pytest.mark.parametrize("hw", [(1080, 1920), (2160, 3840), (270, 480)])
def test_depth_preprocess_f32_matches_torch(hw):
    """float32 output (the reference's precision): only the association of the 2-D filter sums differs from ATen's."""
    from visiondepth3d_amd.render_3d import Renderer
    H, W = hw
    r = Renderer(0)
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, H, W)[0] for i in range(2)])).cuda()
    th, tw = dpt_resize_target(H, W)
    got = r.depth_preprocess(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.float32)
    assert got.shape == (2, 3, th, tw) and got.dtype == torch.float32
    assert got.is_contiguous(memory_format=torch.channels_last)
    ref = _ref(frames, th, tw)
    err = (got - ref).abs()
    assert float(err.max()) < 2e-4, float(err.max())     # values are O(1): ~1e-5 relative filter-sum noise times 1/std
    r.close()


@pytest.mark.parametrize("hw", [(1080, 1920), (2160, 3840), (270, 480), (518, 924), (101, 333)])
def test_depth_preprocess_matches_torch(hw):
    from visiondepth3d_amd.render_3d import Renderer
    H, W = hw
    r = Renderer(0)
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, H, W)[0] for i in range(2)])).cuda()
    th, tw = dpt_resize_target(H, W)
    got = r.depth_preprocess(frames, th, tw, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.bfloat16)
    assert got.shape == (2, 3, th, tw) and got.dtype == torch.bfloat16
    assert got.is_contiguous(memory_format=torch.channels_last)
    ref = _ref(frames, th, tw)
    err = (got.float() - ref).abs()
    tol = ref.abs() * 2.0 ** -8 + 2e-3       # bf16 half-ulp (2^-9) with margin + filter-sum noise near zero
    assert bool((err <= tol).all()), float((err - tol).max())
    same = (got == ref.to(torch.bfloat16)).float().mean().item()
    assert same > 0.98, same                  # almost every element is the SAME bf16 value as the rounded torch result
    r.close()


def test_depth_pipe_uses_fused_front_end():
    """DepthPipe(renderer=...) runs the fused launch and produces (almost) the same prediction as the ATen front end."""
    from visiondepth3d_amd.depth import DepthPipe
    from visiondepth3d_amd.render_3d import Renderer
    r = Renderer(0)
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, 270, 480)[0] for i in range(2)])).cuda()
    pa = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.bfloat16)
    pb = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.bfloat16, renderer=r)
    a = pa.infer_bgr_u8(frames, raw=True)
    r.set_profiling(True)
    b = pb.infer_bgr_u8(frames, raw=True)
    assert r.stage_calls("depth_prep") == 1
    rel = ((a - b).abs().mean() / a.abs().mean()).item()
    assert rel < 2e-2, rel                    # bf16 network: inputs differ in a few last bf16 bits
    # the stock HF module graph (separate q/k/v, LayerScale modules, unpadded token sequence) gives the same prediction
    pc = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.bfloat16, fuse_backbone=False)
    c = pc.infer_bgr_u8(frames, raw=True)
    rel = ((a - c).abs().mean() / c.abs().mean()).item()
    assert rel < 2e-2, rel
    r.close()


@pytest.mark.parametrize("cols", [384, 768, 1024])
def test_add_layernorm_matches_torch(cols):
    from visiondepth3d_amd.render_3d import Renderer
    r = Renderer(0)
    g = torch.Generator(device="cuda").manual_seed(cols)
    x = (torch.randn(2, 1237, cols, device="cuda", generator=g) * 2).to(torch.bfloat16)
    y = torch.randn(2, 1237, cols, device="cuda", generator=g).to(torch.bfloat16)
    ln = torch.nn.LayerNorm(cols, eps=1e-6).cuda().to(torch.bfloat16)
    with torch.no_grad():
        ln.weight.copy_(1 + 0.1 * torch.randn(cols, device="cuda", generator=g))
        ln.bias.copy_(0.1 * torch.randn(cols, device="cuda", generator=g))
        s_ref = x + y
        n_ref = torch.nn.functional.layer_norm(s_ref.float(), (cols,), ln.weight.float(), ln.bias.float(), 1e-6)
        s, n = r.add_layernorm(x, y, ln)
        assert torch.equal(s, s_ref)                                   # bf16 add is exactly ATen's
        err = (n.float() - n_ref).abs()
        assert bool((err <= n_ref.abs() * 2.0 ** -8 + 1e-2).all()), float(err.max())
        x2, n2 = r.add_layernorm(x, None, ln)
        assert x2 is x
        n2_ref = torch.nn.functional.layer_norm(x.float(), (cols,), ln.weight.float(), ln.bias.float(), 1e-6)
        assert bool(((n2.float() - n2_ref).abs() <= n2_ref.abs() * 2.0 ** -8 + 1e-2).all())
    r.close()


@pytest.mark.parametrize("shape", [(2, 64, 19, 33, 37, 66), (2, 32, 37, 66, 70, 126), (1, 64, 5, 7, 10, 14), (1, 8, 3, 3, 2, 2)])
def test_upsample_bilinear_nhwc_matches_torch(shape):
    from visiondepth3d_amd.render_3d import Renderer
    import torch.nn.functional as F
    B, Cc, ih, iw, oh, ow = shape
    r = Renderer(0)
    g = torch.Generator(device="cuda").manual_seed(ih * iw)
    x = torch.randn(B, Cc, ih, iw, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    got = r.upsample_bilinear(x, (oh, ow))
    ref = F.interpolate(x.float(), size=(oh, ow), mode="bilinear", align_corners=True)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
    err = (got.float() - ref).abs()
    assert bool((err <= ref.abs() * 2.0 ** -8 + 1e-6).all()), float(err.max())
    same = (got == F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=True)).float().mean().item()
    assert same > 0.99, same        # bit-identical to ATen's bf16 kernel on (almost) every element
    r.close()


@pytest.mark.parametrize("cols", [384, 768, 1024])
def test_add_layernorm_f32_matches_torch(cols):
    from visiondepth3d_amd.render_3d import Renderer
    r = Renderer(0)
    g = torch.Generator(device="cuda").manual_seed(cols)
    x = torch.randn(2, 1237, cols, device="cuda", generator=g) * 2
    y = torch.randn(2, 1237, cols, device="cuda", generator=g)
    ln = torch.nn.LayerNorm(cols, eps=1e-6).cuda()
    with torch.no_grad():
        ln.weight.copy_(1 + 0.1 * torch.randn(cols, device="cuda", generator=g))
        ln.bias.copy_(0.1 * torch.randn(cols, device="cuda", generator=g))
        s, n = r.add_layernorm(x, y, ln)
        assert torch.equal(s, x + y)                                   # float32 add is exactly ATen's
        n_ref = torch.nn.functional.layer_norm((x + y).double(), (cols,), ln.weight.double(), ln.bias.double(), 1e-6)
        assert float((n.double() - n_ref).abs().max()) < 5e-6
        x2, n2 = r.add_layernorm(x, None, ln)
        assert x2 is x
        n2_ref = torch.nn.functional.layer_norm(x.double(), (cols,), ln.weight.double(), ln.bias.double(), 1e-6)
        assert float((n2.double() - n2_ref).abs().max()) < 5e-6
    r.close()


@pytest.mark.parametrize("shape", [(2, 64, 19, 33, 37, 66), (1, 32, 37, 66, 70, 126), (1, 4, 3, 3, 2, 2)])
def test_upsample_bilinear_nhwc_f32_matches_torch(shape):
    from visiondepth3d_amd.render_3d import Renderer
    import torch.nn.functional as F
    B, Cc, ih, iw, oh, ow = shape
    r = Renderer(0)
    g = torch.Generator(device="cuda").manual_seed(ih * iw)
    x = torch.randn(B, Cc, ih, iw, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    got = r.upsample_bilinear(x, (oh, ow))
    ref = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=True)
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    assert float((got - ref).abs().max()) < 1e-5
    r.close()


def test_dpt_neck_head_glue_kernels_match_torch():
    """vd3d_nhwc_bias_act_f32 / vd3d_upsample_bilinear_bias_nhwc_f32 / vd3d_dpt_head_tail_f32 (round 4: what sits between the library
    convolutions of the DPT neck / head) against the torch expressions they replace.  The element-wise ones perform the same float32
    operations in the same order: bit for bit; the head tail sums its C products in another order: 1e-6 of the range."""
    from visiondepth3d_amd.render_3d import Renderer
    import torch.nn.functional as F
    r = Renderer(0)
    g = torch.Generator(device="cuda").manual_seed(7)
    CL = torch.channels_last

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=g)
    for (B, Cc, h, w) in ((2, 128, 19, 33), (1, 64, 37, 66), (3, 4, 5, 7)):
        y0, r1, r2 = (rnd(B, Cc, h, w).contiguous(memory_format=CL) for _ in range(3))
        bias = rnd(Cc)
        bv = bias.view(1, -1, 1, 1)
        # bias + ReLU in place
        y = y0.clone(memory_format=torch.preserve_format)
        out = r.bias_act(y, bias, relu=True)
        assert out.data_ptr() == y.data_ptr() and torch.equal(out, torch.relu(y0 + bv))
        # bias + unit input + running state, and the ReLU'd copy
        y = y0.clone(memory_format=torch.preserve_format)
        out, rc = r.bias_act(y, bias, r1=r1, r2=r2, want_relu_copy=True)
        ref = r2 + ((y0 + bv) + r1)
        assert torch.equal(out, ref) and torch.equal(rc, torch.relu(ref)) and rc.is_contiguous(memory_format=CL)
        # no bias, one residual
        y = y0.clone(memory_format=torch.preserve_format)
        assert torch.equal(r.bias_act(y, None, r1=r1), y0 + r1)
        # up-sampling with the producing convolution's bias on the interpolated value
        oh, ow = 2 * h + 1, 2 * w
        got = r.upsample_bilinear_bias(y0, (oh, ow), bias)
        assert got.shape == (B, Cc, oh, ow) and got.is_contiguous(memory_format=CL)
        assert torch.equal(got, r.upsample_bilinear(y0, (oh, ow)) + bv)
        assert float((got - (F.interpolate(y0, size=(oh, ow), mode="bilinear", align_corners=True) + bv)).abs().max()) < 1e-5
    for (B, Cc, h, w) in ((2, 32, 37, 66), (1, 64, 9, 5), (1, 16, 3, 3)):
        y = rnd(B, Cc, h, w).contiguous(memory_format=CL)
        b2, w3 = rnd(Cc), rnd(Cc)
        pre = (torch.relu(y.double() + b2.double().view(1, -1, 1, 1)) * w3.double().view(1, -1, 1, 1)).sum(1)
        b3, scale = -float(pre.mean()), 1.5          # the 1x1 convolution's bias placed so that the final ReLU clips about half of the pixels
        got = r.dpt_head_tail(y, b2, w3, b3, scale)
        ref = torch.relu(pre + b3) * scale
        assert got.shape == (B, h, w) and got.dtype == torch.float32
        assert float((got.double() - ref).abs().max()) < 1e-5 * max(1.0, float(pre.abs().max()))
        assert float(got.min()) >= 0.0 and 0.2 < float((got == 0).float().mean()) < 0.8
    with pytest.raises(ValueError):
        r.bias_act(torch.zeros(1, 8, 4, 4, device="cuda"), None)      # NCHW-contiguous: not the kernels' layout
    r.close()
