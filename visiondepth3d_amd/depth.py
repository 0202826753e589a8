"""Depth-model callable (boundary B3, core/render_depth.py:1106-1119) on PyTorch-ROCm.

The reference wraps ``transformers.pipeline("depth-estimation")`` in
``pipe(images: list[PIL], inference_size=None) -> list[{"predicted_depth": Tensor}]``.  This module
keeps that protocol (``DepthPipe.__call__``) and adds a device-resident fast path
(``DepthPipe.infer_bgr_u8``) that consumes uint8 BGR frames already in HBM and returns depth planes in HBM,
so the 2D->3D stage can start without the reference's host round trip and 8-bit depth video on disk
(core/render_depth.py:1907-1935) -- while still reproducing that hand-off's per-frame min-max -> uint8
truncation (``depth_to_u8``, a24) so the DIBR stage sees the same quantised values.

MFMA work (DINOv2 GEMMs / attention, DPT convs) goes through PyTorch-ROCm (hipBLASLt / MIOpen / SDPA): per
BASELINE.json:north_star the depth net is NOT hand-written.

Precision: the reference loads ``AutoModelForDepthEstimation.from_pretrained(checkpoint)`` with no dtype, i.e. float32
(core/render_depth.py:758-759,823-824); float32 is the DEFAULT here (f32-input MFMA on gfx950) and bfloat16 is an opt-in
whose uint8 depth-plane deviation is measured by tests/test_hip_depth_e2e.py.

Checkpoints: ``DepthPipe.from_pretrained(dir)`` loads a local Hugging Face folder (config.json + model.safetensors +
preprocessor_config.json) exactly like the reference's local-model branch (:756-760) and then applies the fused-weight
rewrites.  No network and no checkpoints exist in the build environment, so benchmarks and tests use deterministic
synthetic weights (NumPy PCG64 keyed by parameter name) on the real architectures.
"""
from __future__ import annotations

import json
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from .vit_blocks import dinov2_operands, dpt_vit_operands, encoder_blocks, head_geometry_ok, query_padding

# Architectures of the reference's model list (core/render_depth.py:686-712) that go through its Hugging Face branch
# (AutoModelForDepthEstimation, :756-760,823-824).  "da" = DepthAnythingForDepthEstimation on a DINOv2 backbone: Depth-Anything V1
# (LiheYoung/depth-anything-*-hf), V2 (depth-anything/Depth-Anything-V2-*-hf) and Distill-Any-Depth
# (xingyang1/Distill-Any-Depth-*-hf) share these three shapes and differ only in their weights.  "dpt" = DPTForDepthEstimation
# (MiDaS 3.0 family: Intel/dpt-large).  Marigold / DepthCrafter / ONNX entries are other pipelines (out of scope).
_DA_S = dict(arch="da", hidden=384, layers=12, heads=6, out_indices=[9, 10, 11, 12], neck=[48, 96, 192, 384], fusion=64, head=32)
_DA_B = dict(arch="da", hidden=768, layers=12, heads=12, out_indices=[9, 10, 11, 12], neck=[96, 192, 384, 768], fusion=128, head=32)
_DA_L = dict(arch="da", hidden=1024, layers=24, heads=16, out_indices=[21, 22, 23, 24], neck=[256, 512, 1024, 1024], fusion=256, head=32)
MODEL_ZOO = {
    "depth-anything-v2-small": _DA_S, "depth-anything-v2-base": _DA_B, "depth-anything-v2-large": _DA_L,
    "depth-anything-v1-small": _DA_S, "depth-anything-v1-base": _DA_B, "depth-anything-v1-large": _DA_L,
    "distill-any-depth-small": _DA_S, "distill-any-depth-large": _DA_L,
    # depth-anything/Depth-Anything-V2-Metric-{Indoor,Outdoor}-Large-hf: the same DINOv2-L network with depth_estimation_type="metric" -- the head ends in
    # Sigmoid() * max_depth (metres: 20 indoor / Hypersim, 80 outdoor / Virtual KITTI 2) instead of ReLU() * max_depth
    "depth-anything-v2-metric-indoor-large": dict(_DA_L, metric=True, max_depth=20),
    "depth-anything-v2-metric-outdoor-large": dict(_DA_L, metric=True, max_depth=80),
    "dpt-large": dict(arch="dpt", hidden=1024, layers=24, heads=16, out_indices=[5, 11, 17, 23], neck=[256, 512, 1024, 1024], fusion=256),
    # Intel/dpt-hybrid-midas ("MiDaS 3.0"): ViT-B/16 behind a BiT ResNet-50 prefix (stages 1 - 3, weight-standardised convolutions, GroupNorm(32)); hooks 0 / 1 are the
    # prefix's stage-1 / stage-2 maps and go to the neck as they are (neck_ignore_stages), hooks 2 / 3 are ViT layers 8 / 11 through the "project" readout
    "dpt-hybrid-midas": dict(arch="dpt", hybrid=True, hidden=768, layers=12, heads=12, out_indices=[2, 5, 8, 11], neck=[256, 512, 768, 768], fusion=256),
    # apple/DepthPro-hf (DepthProForDepthEstimation): three DINOv2 ViT-L/16 encoders (image, patch, field of view) at 384 x 384 over a 1 + 9 + 25 patch pyramid of
    # the 1536 x 1536 input; depth_pro.py states the geometry (as far as it is known here) and the processor
    "depth-pro": dict(arch="depth_pro", hidden=1024, layers=24, heads=16, fusion=256),
}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_CL = torch.channels_last
# image-processor constants (preprocessor_config.json of the checkpoints): DA = DPTImageProcessor(size 518, keep_aspect_ratio,
# ensure_multiple_of 14, bicubic, ImageNet mean/std); DPT-Large = 384 x 384, no aspect keeping, mean = std = 0.5
PROCESSORS = {
    "da": dict(size=(518, 518), keep_aspect_ratio=True, multiple=14, mean=IMAGENET_MEAN, std=IMAGENET_STD),
    "dpt": dict(size=(384, 384), keep_aspect_ratio=False, multiple=1, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)),
    # DepthProImageProcessor: 1536 x 1536, no aspect keeping, BILINEAR (PIL resample 2) without antialias AFTER rescale + normalise, mean = std = 0.5
    "depth_pro": dict(size=(1536, 1536), keep_aspect_ratio=False, multiple=1, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), resample=2),
}


def build_config(name: str):
    from transformers import DepthAnythingConfig, Dinov2Config
    z = MODEL_ZOO[name]
    if z["arch"] == "depth_pro":
        from . import depth_pro
        return depth_pro.config()
    if z["arch"] == "dpt":
        from transformers import DPTConfig
        if z.get("hybrid"):   # the published config.json of Intel/dpt-hybrid-midas
            return DPTConfig(is_hybrid=True, hidden_size=z["hidden"], num_hidden_layers=z["layers"], num_attention_heads=z["heads"], intermediate_size=4 * z["hidden"],
                             image_size=384, patch_size=16, backbone_out_indices=z["out_indices"], neck_hidden_sizes=z["neck"], neck_ignore_stages=[0, 1],
                             reassemble_factors=[1, 1, 1, 0.5], fusion_hidden_size=z["fusion"], readout_type="project", backbone_featmap_shape=[1, 1024, 24, 24],
                             backbone_config=dict(model_type="bit", layer_type="bottleneck", depths=[3, 4, 9], out_features=["stage1", "stage2", "stage3"],
                                                  global_padding="same", embedding_dynamic_padding=True, num_groups=32))
        return DPTConfig(hidden_size=z["hidden"], num_hidden_layers=z["layers"], num_attention_heads=z["heads"],
                         intermediate_size=4 * z["hidden"], image_size=384, patch_size=16, backbone_out_indices=z["out_indices"],
                         neck_hidden_sizes=z["neck"], fusion_hidden_size=z["fusion"], readout_type="project")
    bc = Dinov2Config(hidden_size=z["hidden"], num_hidden_layers=z["layers"], num_attention_heads=z["heads"], patch_size=14,
                      image_size=518, out_indices=z["out_indices"], reshape_hidden_states=False, apply_layernorm=True)
    metric = dict(depth_estimation_type="metric", max_depth=int(z["max_depth"])) if z.get("metric") else {}   # (the config class takes an int there)
    return DepthAnythingConfig(backbone_config=bc, reassemble_hidden_size=z["hidden"], neck_hidden_sizes=z["neck"],
                               fusion_hidden_size=z["fusion"],
                               head_hidden_size=z["head"], reassemble_factors=[4, 2, 1, 0.5], patch_size=14, **metric)


@torch.no_grad()
def synthetic_weights_(model: torch.nn.Module, seed: int = 0) -> None:
    """Deterministic, platform-stable weights: PCG64 keyed by crc32(parameter name) ^ seed."""
    for name, p in model.named_parameters():
        rng = np.random.Generator(np.random.PCG64((zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0xFFFFFFFF))
        if p.ndim >= 2 and "position_embeddings" not in name and "token" not in name:
            fan_in = int(np.prod(p.shape[1:]))
            a = float(np.sqrt(3.0 / max(fan_in, 1)))  # unit-gain uniform
            v = rng.uniform(-a, a, size=tuple(p.shape)).astype(np.float32)
        elif name.endswith("bias"):
            v = rng.uniform(-0.02, 0.02, size=tuple(p.shape)).astype(np.float32)
        elif "lambda" in name or "layer_scale" in name:
            v = np.full(tuple(p.shape), 0.2, np.float32)
        elif p.ndim == 1:
            v = (1.0 + rng.uniform(-0.05, 0.05, size=tuple(p.shape))).astype(np.float32)
        else:
            v = rng.uniform(-0.02, 0.02, size=tuple(p.shape)).astype(np.float32)
        p.copy_(torch.from_numpy(v).to(p.dtype))


def dpt_resize_target(h: int, w: int, size=518, multiple: int = 14, keep_aspect_ratio: bool = True):
    """DPTImageProcessor.get_resize_output_image_size (keep_aspect_ratio, ensure_multiple_of=14): 1080x1920 -> 518x924."""
    size_h, size_w = (size, size) if isinstance(size, int) else size
    sh, sw = size_h / h, size_w / w
    if keep_aspect_ratio:
        if abs(1 - sw) < abs(1 - sh):
            sh = sw
        else:
            sw = sh

    def snap(v):
        return max(int(round(v / multiple)) * multiple, multiple)

    return snap(sh * h), snap(sw * w)


def depth_to_u8(pred: torch.Tensor, invert: bool = False) -> torch.Tensor:
    """convert_depth_to_grayscale (core/render_depth.py:585-611) per frame, on device: min-max normalise,
    ``(norm*255).astype(uint8)`` truncation; invalid / flat frames -> zeros; optional ``255 - u8`` (:1914-1916)."""
    p = pred.float()
    flat = p.flatten(1)
    mn, mx = flat.min(dim=1).values, flat.max(dim=1).values
    bad = torch.isnan(mn) | torch.isnan(mx) | ((mx - mn) < 1e-6)
    norm = (p - mn[:, None, None]) / (mx - mn + 1e-6)[:, None, None]
    u8 = (norm * 255).clamp(0, 255).to(torch.uint8)
    u8 = torch.where(bad[:, None, None], torch.zeros_like(u8), u8)
    return 255 - u8 if invert else u8


def conv_transpose_gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d weight [C_in, C_out, s, s] (kernel == stride: non-overlapping windows) -> the GEMM weight [(i, j, c_out)][c_in] of
    Y[p][(i, j, co)] = sum_ci X[p][ci] W[ci][co][i][j]; vd3d_depth_to_space_bias_nhwc_f32 then scatters Y's rows to their s x s windows."""
    return w.detach().permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()


class _ConvTransposeGemm:
    """ConvTranspose2d ``m`` with kernel == stride s and no padding (the caller has checked) on renderer R: packed once as conv_transpose_gemm_weight for
    vd3d_gemm_x3 in ``mode``; a call takes the pixel rows [..., C_in] of a B x gh x gw map through the GEMM (``n`` = s s C_out columns, no bias) and
    vd3d_depth_to_space_bias_nhwc_f32, which adds the module's bias: the channels_last [B, C_out, s gh, s gw] map."""

    def __init__(self, R, m, mode):
        self.R, self.m, self.mode, self.n = R, m, mode, m.kernel_size[0] * m.kernel_size[1] * m.out_channels
        self.img = R.gemm_x3_pack(conv_transpose_gemm_weight(m.weight), mode)

    def __call__(self, rows, B, gh, gw):
        y = self.R.linear_x3(rows, self.img, self.n, None, mode=self.mode)
        return self.R.depth_to_space_bias(y.view(B * gh * gw, self.n), B, gh, gw, self.m.kernel_size[0], self.m.bias)


def _is_conv(m, k, s, p):
    """Module m convolves with a k x k kernel at stride s and padding p, dilation 1, in one group."""
    return m.kernel_size == (k, k) and m.stride == (s, s) and m.padding == (p, p) and m.dilation == (1, 1) and m.groups == 1


def neck_poly_offsets(f: int):
    """The blocks of the polyphase form of conv3x3(ConvTranspose2d(kernel = stride = f)) in the order vd3d_neck_poly_conv_f32 sums them: [(pa, pb, di, dj)], phases
    (pa, pb) row-major, inside a phase di ascending, then dj ascending.  A fine tap dy in {-1, 0, 1} of phase coordinate a lands in coarse offset (a + dy) // f:
    coordinate 0 reaches {-1, 0}, f - 1 reaches {0, 1}, any other {0}.  (f + 2)^2 blocks: 36 for f = 4 (2.25 per output pixel), 16 for f = 2 (4)."""
    if int(f) != f or f < 2:
        raise ValueError(f"neck_poly: factor {f!r}: an integer of at least 2 expected")
    reach = [sorted({(a + d) // f for d in (-1, 0, 1)}) for a in range(f)]
    return [(pa, pb, di, dj) for pa in range(f) for pb in range(f) for di in reach[pa] for dj in reach[pb]]


def neck_poly_compose(wt: torch.Tensor, bt, w3: torch.Tensor, f: int, dtype=torch.float32):
    """ConvTranspose2d(C, C, kernel_size=f, stride=f) (weight ``wt`` [C_in, C, f, f], bias ``bt`` [C] or None) followed by a bias-free 3 x 3 / padding 1 convolution
    (``w3`` [C_out, C, 3, 3]) as one linear map on the COARSE grid -> (Wc [blocks, C_out, C_in], bc [blocks, C_out]) float32 in ``neck_poly_offsets(f)``'s order:
        out[:, f i + pa, f j + pb] = sum over the blocks k of phase (pa, pb) whose coarse pixel (i + di, j + dj) lies inside the map of  Wc[k] @ x[:, i + di, j + dj] + bc[k]
    Wc[k] sums W3[dy, dx] @ Wt[(pa + dy) % f, (pb + dx) % f]^T over the fine taps (dy, dx) that land in offset (di, dj) = ((pa + dy) // f, (pb + dx) // f), bc[k] sums
    W3[dy, dx] @ bt over the same taps (a coarse pixel outside the map contributes neither: the convolution pads the fine map with zeros, not with the bias).
    Composed in float64, rounded once to ``dtype``.  C_in x blocks / f^2 multiply-adds per output pixel and channel instead of C_in + 9 C."""
    offs = neck_poly_offsets(f)
    if wt.dim() != 4 or w3.dim() != 4 or tuple(wt.shape[2:]) != (f, f) or tuple(w3.shape[2:]) != (3, 3) or w3.shape[1] != wt.shape[1]:
        raise ValueError(f"neck_poly: weights {tuple(wt.shape)} / {tuple(w3.shape)} are not [C_in, C, {f}, {f}] and [C_out, C, 3, 3]")
    if bt is not None and tuple(bt.shape) != (wt.shape[1],):
        raise ValueError(f"neck_poly: bias {tuple(bt.shape)} is not [{wt.shape[1]}]")
    wt64, w364 = wt.detach().to(torch.float64), w3.detach().to(torch.float64)
    bt64 = torch.zeros(wt.shape[1], dtype=torch.float64, device=wt.device) if bt is None else bt.detach().to(torch.float64)
    Wc = torch.zeros(len(offs), w3.shape[0], wt.shape[0], dtype=torch.float64, device=wt.device)
    bc = torch.zeros(len(offs), w3.shape[0], dtype=torch.float64, device=wt.device)
    at = {o: k for k, o in enumerate(offs)}
    for pa in range(f):
        for pb in range(f):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    k = at[pa, pb, (pa + dy) // f, (pb + dx) // f]
                    Wc[k] += w364[:, :, dy + 1, dx + 1] @ wt64[:, :, (pa + dy) % f, (pb + dx) % f].t()
                    bc[k] += w364[:, :, dy + 1, dx + 1] @ bt64
    return Wc.to(dtype).contiguous(), bc.to(dtype).contiguous()


HEAD_UPCONV_BUILT = ((128, 64), (64, 32))   # (C, C_out) of head.conv1 that vd3d_head_upconv_gather_f32 builds and the probe cleared (profiles/r26_head_upconv.md)


def head_upconv_compose(proj_w: torch.Tensor, proj_b, conv1_w: torch.Tensor, dtype=torch.float32):
    """A 1 x 1 projection (weight ``proj_w`` [C, C_in, 1, 1] or [C, C_in], bias ``proj_b`` [C] or None), a bilinear up-sampling and a bias-free 3 x 3 convolution
    (``conv1_w`` [C_out, C, 3, 3], zero padding) have nothing non-linear between them, the up-sampling U acts per channel and a tap's matrix W_t per pixel:
        conv1(U(P h + b_p)) = sum over the 9 taps t of  S_t U ( (W_t P) h + W_t b_p )           (S_t: the tap's shift on the fine grid, zero outside it)
    -> (Wc [9 * C_out, C_in], bc [9 * C_out]): tap t = 3 ky + kx, channel t * C_out + o,
        Wc[t * C_out + o, i] = sum_c conv1_w[o, c, ky, kx] proj_w[c, i],      bc[t * C_out + o] = sum_c conv1_w[o, c, ky, kx] proj_b[c]
    (folding W_t b_p into the coarse map relies on the interpolation weights summing to one).  Composed in float64, rounded once to ``dtype``.  The coarse GEMM
    Z = h Wc^T + bc has a quarter of the fine map's pixels: 9 C_in multiply-adds per coarse pixel and channel instead of C_in per coarse and 9 C per fine one."""
    if conv1_w.dim() != 4 or tuple(conv1_w.shape[2:]) != (3, 3):
        raise ValueError(f"head_upconv: convolution weight {tuple(conv1_w.shape)} is not [C_out, C, 3, 3]")
    Co, Cm = int(conv1_w.shape[0]), int(conv1_w.shape[1])
    if proj_w.dim() not in (2, 4) or proj_w.shape[0] != Cm or (proj_w.dim() == 4 and tuple(proj_w.shape[2:]) != (1, 1)):
        raise ValueError(f"head_upconv: projection weight {tuple(proj_w.shape)} is not [{Cm}, C_in, 1, 1]")
    if proj_b is not None and tuple(proj_b.shape) != (Cm,):
        raise ValueError(f"head_upconv: projection bias {tuple(proj_b.shape)} is not [{Cm}]")
    P = proj_w.detach().to(torch.float64).reshape(Cm, -1)
    W = conv1_w.detach().to(torch.float64).permute(2, 3, 0, 1).reshape(9, Co, Cm)   # [t = 3 ky + kx][o][c]
    b = torch.zeros(Cm, dtype=torch.float64, device=P.device) if proj_b is None else proj_b.detach().to(torch.float64)
    return (W @ P).reshape(9 * Co, -1).to(dtype).contiguous(), (W @ b).reshape(9 * Co).to(dtype).contiguous()


HEAD_CONV2_GATHER_BUILT = (32, 64, 128)    # C_in of head.conv2 (-> 32 channels) that vd3d_head_conv_gather_f32 builds
HEAD_CONV2_GATHER_ROUTED = (32, 64)        # ... and routes by default: those whose probe cleared its bar (profiles/r27_head_conv2_gather.md)


def head_conv2_compose(conv2_w: torch.Tensor, conv1_b: torch.Tensor, dtype=torch.float32):
    """A bias ``conv1_b`` [C], a bilinear up-sampling U and a bias-free 3 x 3 convolution (``conv2_w`` [C_out, C, 3, 3], zero padding) have nothing non-linear between
    them (``head_upconv_compose``'s identity with the identity as projection):
        conv2(U(y1 + b1)) = sum over the 9 taps t of  S_t U ( W_t y1 + W_t b1 )
    -> (Wt [9 * C_out, C], bc [9 * C_out]): tap t = 3 ky + kx, row t * C_out + o,  Wt[t * C_out + o, c] = conv2_w[o, c, ky, kx],  bc[t * C_out + o] = sum_c conv2_w[o, c, ky, kx] b1[c].
    Computed in float64, rounded once to ``dtype`` (Wt is a permutation of the weight: exact)."""
    if conv2_w.dim() != 4 or tuple(conv2_w.shape[2:]) != (3, 3):
        raise ValueError(f"head_conv2: convolution weight {tuple(conv2_w.shape)} is not [C_out, C, 3, 3]")
    Co, Cm = int(conv2_w.shape[0]), int(conv2_w.shape[1])
    if tuple(conv1_b.shape) != (Cm,):
        raise ValueError(f"head_conv2: bias {tuple(conv1_b.shape)} is not [{Cm}]")
    W = conv2_w.detach().to(torch.float64).permute(2, 3, 0, 1).reshape(9, Co, Cm)   # [t = 3 ky + kx][o][c]
    b = conv1_b.detach().to(torch.float64)
    return W.reshape(9 * Co, Cm).to(dtype).contiguous(), (W @ b).reshape(9 * Co).to(dtype).contiguous()


def patch_embedding_gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """Patch-embedding weight [C, 3, p, p] (kernel == stride: every patch is one GEMM row) -> [C, Kp]: the flattened (c, ky, kx) columns, zero-padded from 3 p^2
    to the next multiple of 16 (vd3d_gemm_x3's K unit; p = 14: 588 -> 592).  vd3d_patchify_f32 writes the matching rows, zero tail included."""
    C, k = w.shape[0], w[0].numel()
    return F.pad(w.detach().reshape(C, k), (0, (k + 15) // 16 * 16 - k)).contiguous()


def patch_embedding_conv_ok(conv) -> bool:
    """Conv2d(3, C, kernel_size=p, stride=p), p <= 64: the patch embeddings vd3d_patchify_f32 takes."""
    p = conv.kernel_size[0] if isinstance(conv, torch.nn.Conv2d) else 0
    return 0 < p <= 64 and conv.kernel_size == (p, p) and conv.stride == (p, p) and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.in_channels == 3


def patch_embedding_rows(R, conv, mode: str):
    """A patch-embedding convolution (``patch_embedding_conv_ok``) as vd3d_patchify_f32 + vd3d_gemm_x3 in ``mode``, its weight packed once, here: returns
    ``x -> [B, T - 1, C]`` for a float32 [B, 3, th, tw] image in channels_last memory, bias included."""
    img = R.gemm_x3_pack(patch_embedding_gemm_weight(conv.weight), mode)
    return lambda x: R.linear_x3(R.patchify(x, conv.kernel_size[0]), img, conv.out_channels, conv.bias, mode=mode)


def _memoise(obj, attr: str, key):
    """``obj.attr(t, *args)`` -- a position-embedding interpolation, a constant of the input size -- memoised per ``key(t, *args)``."""
    orig, cache = getattr(obj, attr), {}

    def cached(t, *args):   # (positional, as the embeddings modules call it)
        k = key(t, *args)
        if k not in cache:
            cache[k] = orig(t, *args).detach()
        return cache[k]
    setattr(obj, attr, cached)


def im2col_gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """Convolution weight [C_out, C_in, k, k] -> the GEMM weight [C_out, Kp] whose columns are in vd3d_im2col_nhwc_f32's order, (ky, kx, c_in): a permute to
    [C_out, k, k, C_in], flattened, zero-padded from k k C_in to the next multiple of 16 (the 7 x 7 stem on 3 channels: 147 -> 160)."""
    Cout, kk = w.shape[0], w[0].numel()
    return F.pad(w.detach().permute(0, 2, 3, 1).reshape(Cout, kk), (0, (kk + 15) // 16 * 16 - kk)).contiguous()


def same_padding(size: int, k: int, stride: int):
    """TensorFlow "same" padding of one axis as transformers' DynamicPad2d computes it (dilation 1) -> (low, high): 384 / 7 / 2 -> (2, 3); 96 / 3 / 2 -> (0, 1)."""
    total = max((-(-size // stride) - 1) * stride + k - size, 0)
    return total // 2, total - total // 2


def bit_standardized_weight(m) -> torch.Tensor:
    """The weight a WeightStandardizedConv2d convolves with, by the module's own expression (it recomputes this on every forward), in float32 on the CPU --
    the values the CPU module computes, whatever device the module is on.  Folded once, before packing, by DepthPipe(self_contained=True)."""
    w = m.weight.detach().to("cpu", torch.float32)
    return F.batch_norm(w.reshape(1, m.out_channels, -1), None, None, training=True, momentum=0.0, eps=m.eps).reshape_as(w)


def _bit_conv_kind(m, name: str, stem: bool = False) -> str:
    """How self_contained=True routes the convolution ``m`` of a BiT prefix: "gemm" (1 x 1 / stride 1: vd3d_gemm_x3 over the pixel rows), "tile" (3 x 3 / stride 1 /
    padding 1: the tile convolution of the mode) or "im2col" (stride 2 with dynamic "same" padding -- the 7 x 7 stem, 3 x 3, 1 x 1: vd3d_im2col_nhwc_f32 +
    vd3d_gemm_x3).  Anything else is refused by name.  Reads the module only."""
    tag = f"self_contained=True: {name}"
    if type(m).__name__ != "WeightStandardizedConv2d":
        raise NotImplementedError(f"{tag} ({type(m).__name__}) is no weight-standardised convolution -- not built")
    if m.bias is not None:
        raise NotImplementedError(f"{tag} has a bias (BiT's convolutions have none) -- not built")
    k, s, dyn = m.kernel_size, m.stride, m.pad is not None
    if m.groups == 1 and m.dilation == (1, 1):
        cin16 = m.in_channels % 16 == 0
        if k == (1, 1) and s == (1, 1) and m.padding == (0, 0) and not dyn and cin16:
            return "gemm"
        if k == (3, 3) and s == (1, 1) and m.padding == (1, 1) and not dyn and cin16 and m.out_channels in (32, 64, 128, 256):
            return "tile"
        if s == (2, 2) and m.padding == (0, 0) and dyn and ((k in ((1, 1), (3, 3)) and cin16) or (stem and k == (7, 7) and m.in_channels == 3)):
            return "im2col"
    raise NotImplementedError(f"{tag}: kernel {k} / stride {s} / padding {m.padding}{' + dynamic same-padding' if dyn else ''} / dilation {m.dilation} / groups "
                              f"{m.groups}, {m.in_channels} -> {m.out_channels} channels (built: 1 x 1 and 3 x 3 -> 32 / 64 / 128 / 256 at stride 1, 1 x 1 and 3 x 3 at "
                              "stride 2 with 'same' padding, C_in % 16; the 7 x 7 stride-2 stem on 3 channels) -- not built")


def _bit_norm_relu(n, name: str) -> bool:
    """The BitGroupNormActivation ``n`` as vd3d_groupnorm_nhwc_f32 runs it -> whether a ReLU follows; anything the kernel does not build is refused by name."""
    if (type(n).__name__ != "BitGroupNormActivation" or n.num_groups != 32 or not n.affine or n.num_channels not in (64, 128, 256, 512, 1024)
            or not isinstance(n.activation, (torch.nn.ReLU, torch.nn.Identity))):
        raise NotImplementedError(f"self_contained=True: {name} ({type(n).__name__}, {getattr(n, 'num_channels', '?')} channels in {getattr(n, 'num_groups', '?')} groups, "
                                  f"activation {type(getattr(n, 'activation', None)).__name__}) -- built: GroupNorm(32) with an affine on 64 / 128 / 256 / 512 / 1024 "
                                  "channels, followed by ReLU or nothing")
    return isinstance(n.activation, torch.nn.ReLU)


def bit_prefix_plan(backbone, names: dict) -> dict:
    """What self_contained=True runs for the BitBackbone ``backbone`` of a DPT-Hybrid (``names``: id(module) -> name): per convolution its route, per
    normalisation whether a ReLU follows -- or NotImplementedError naming the first module the mode does not build (a bias, a pre-activation layer, groups != 32,
    global_padding other than "same", ...).  Reads the module graph and its configuration only: no device, no renderer."""
    cfg, top = backbone.config, names[id(backbone)]
    for what, ok in ((f"global_padding={cfg.global_padding!r} (built: 'same')", str(cfg.global_padding or "").lower() == "same"),
                     (f"layer_type={cfg.layer_type!r} (built: 'bottleneck')", cfg.layer_type == "bottleneck"),
                     (f"num_groups={cfg.num_groups} (built: 32)", int(cfg.num_groups) == 32)):
        if not ok:
            raise NotImplementedError(f"self_contained=True: {top}: a BiT backbone with {what} -- not built")
    emb, pool = backbone.bit.embedder, backbone.bit.embedder.pooler
    if not (type(pool).__name__ == "BitMaxPool2d" and tuple(pool.kernel_size) == (3, 3) and tuple(pool.stride) == (2, 2) and tuple(pool.padding) == (0, 0)
            and tuple(pool.dilation) == (1, 1) and not pool.ceil_mode and type(pool.pad).__name__ == "DynamicPad2d" and isinstance(emb.pad, torch.nn.Identity)):
        raise NotImplementedError(f"self_contained=True: {names[id(pool)]}: a stem pool other than 3 x 3 / stride 2 with dynamic 'same' padding and no ConstantPad2d "
                                  "in front of the norm (embedding_dynamic_padding=True, global_padding='same') -- not built")
    plan = {"conv": {}, "relu": {}, "layers": []}

    def conv(m, stem=False):
        plan["conv"][id(m)] = _bit_conv_kind(m, names[id(m)], stem)

    def norm(n, want_relu):
        plan["relu"][id(n)] = _bit_norm_relu(n, names[id(n)])
        if plan["relu"][id(n)] != want_relu:
            raise NotImplementedError(f"self_contained=True: {names[id(n)]}: {'a' if want_relu else 'no'} ReLU expected behind this normalisation -- not built")
    conv(emb.convolution, stem=True)
    norm(emb.norm, True)
    for stage in backbone.bit.encoder.stages:
        for lay in stage.layers:
            if type(lay).__name__ != "BitBottleneckLayer" or not isinstance(lay.activation, torch.nn.ReLU):
                raise NotImplementedError(f"self_contained=True: {names[id(lay)]} ({type(lay).__name__}) is no post-activation bottleneck ending in ReLU -- not built")
            if lay.downsample is not None:
                conv(lay.downsample.conv)
                norm(lay.downsample.norm, False)
            for c, n, r in ((lay.conv1, lay.norm1, True), (lay.conv2, lay.norm2, True), (lay.conv3, lay.norm3, False)):
                conv(c)
                norm(n, r)
            plan["layers"].append(lay)
    return plan


class _BitPrefix:
    """The BiT ResNet prefix of DPT-Hybrid on renderer R without a library call (self_contained=True): ``plan`` = bit_prefix_plan(backbone).  The standardised
    weights (bit_standardized_weight) are folded and packed once, here; activations are contiguous float32 NHWC [B, H, W, C] from the first launch to the last.
    Per bottleneck: three GEMM / convolution launches (four in a stage's first layer, whose shortcut is a convolution too; an im2col launch in front of a strided
    one) and one vd3d_groupnorm_nhwc_f32 behind each (one fixed summation order: batch-independent, bit-repeatable) -- the last one with the shortcut and the ReLU in
    its apply pass; the stem's pool is vd3d_maxpool3x3_s2_nhwc_f32 (TensorFlow "same" padding).  A call returns the stage-1, -2 and -3 maps."""

    def __init__(self, pipe, backbone, plan, names):
        self.pipe, self.bb, self.plan, self.names = pipe, backbone, plan, names
        R, gm = pipe.renderer, pipe.gemm
        self.ops = {}
        mods = {id(m): m for m in backbone.modules()}
        for mid, kind in plan["conv"].items():
            m = mods[mid]
            w = bit_standardized_weight(m)
            if kind == "tile":
                op = R.conv3x3_tile_pack(w, gm, 1)
                if op is None:
                    raise NotImplementedError(f"self_contained=True: {names[mid]}: vd3d_conv3x3_{R.TILE_CONVS[gm, 1]} does not build {m.in_channels} -> {m.out_channels} channels")
            else:
                op = R.gemm_x3_pack(w.reshape(m.out_channels, -1) if kind == "gemm" else im2col_gemm_weight(w), gm)
            self.ops[mid] = (kind, op)

    def conv(self, m, x):
        pipe, R, gm = self.pipe, self.pipe.renderer, self.pipe.gemm
        kind, op = self.ops[id(m)]
        if kind == "gemm":
            y, how = R.linear_x3(x, op, m.out_channels, None, mode=gm), "vd3d_gemm_x3 over the pixel rows"
        elif kind == "tile":
            y = R.conv3x3_tile(x.permute(0, 3, 1, 2), op, m.out_channels, gm, 1).permute(0, 2, 3, 1)
            how = "vd3d_conv3x3_" + R.TILE_CONVS[gm, 1]
        else:
            k, s = m.kernel_size[0], m.stride[0]
            rows = R.im2col(x, k, s, same_padding(x.shape[1], k, s) + same_padding(x.shape[2], k, s))
            y, how = R.linear_x3(rows, op, m.out_channels, None, mode=gm), "vd3d_im2col_nhwc_f32 + vd3d_gemm_x3"
        pipe.conv_routes[self.names[id(m)]] = (gm, "self-contained: " + how)
        pipe._count_conv(m, y)   # the bypassed module's hook: NHWC or NCHW, the element count per frame is the same
        return y

    def norm(self, n, y, residual=None, relu=None):
        relu = self.plan["relu"][id(n)] if relu is None else relu
        self.pipe.conv_routes[self.names[id(n)]] = (self.pipe.gemm, "self-contained: vd3d_groupnorm_nhwc_f32" + (" + shortcut + ReLU" if residual is not None else ""))
        return self.pipe.renderer.groupnorm(y, n.num_groups, n.weight, n.bias, n.eps, residual=residual, relu=relu, out=y)

    def __call__(self, pixel_values):
        R = self.pipe.renderer
        emb = self.bb.bit.embedder
        if pixel_values.dtype != torch.float32 or pixel_values.shape[1] != emb.num_channels:
            raise NotImplementedError(f"self_contained=True: the BiT stem takes a float32 [B, {emb.num_channels}, th, tw] image")
        x = pixel_values.permute(0, 2, 3, 1).contiguous()   # what depth_preprocess hands over is NHWC storage already
        x = self.norm(emb.norm, self.conv(emb.convolution, x))
        x = R.maxpool3x3_s2(x, same_padding(x.shape[1], 3, 2) + same_padding(x.shape[2], 3, 2), float(emb.pooler.pad.value))
        self.pipe.conv_routes[self.names[id(emb.pooler)]] = (self.pipe.gemm, "self-contained: vd3d_maxpool3x3_s2_nhwc_f32")
        maps, at = [], 0
        for stage in self.bb.bit.encoder.stages:
            for _ in stage.layers:
                lay = self.plan["layers"][at]
                at += 1
                short = x if lay.downsample is None else self.norm(lay.downsample.norm, self.conv(lay.downsample.conv, x))
                h = self.norm(lay.norm1, self.conv(lay.conv1, x))
                h = self.norm(lay.norm2, self.conv(lay.conv2, h))
                x = self.norm(lay.norm3, self.conv(lay.conv3, h), residual=short, relu=True)   # the layer's own ReLU behind the shortcut add
            maps.append(x)
        return maps


class _PerVersion:
    """``get(*tensors)`` -> the value of ``build()``, built ONCE per version of the parameters it is made of.  The key is (data_ptr, _version) per tensor (None entries
    are skipped): an in-place update (load_state_dict, .copy_) bumps a version counter, a replaced ``.data`` moves the address, and either is picked up at the next
    call -- no compose, pack or host read per call.  Inference tensors (created / loaded under torch.inference_mode()) track no version counter; they are
    immutable outside inference mode, so the storage address alone identifies the value.  A None value ("shape not built") is cached like any other."""

    def __init__(self, build):
        self.build, self.key, self.value = build, None, None

    def get(self, *tensors):
        ts = [t for t in tensors if t is not None]
        try:
            key = tuple((t.data_ptr(), t._version) for t in ts)
        except RuntimeError:
            key = tuple((t.data_ptr(),) for t in ts)
        if key != self.key:
            self.value, self.key = self.build(), key
        return self.value


def _head_tail_operands(conv3: torch.nn.Conv2d):
    """() -> (w3, b3) of the head's 1x1 convolution to one channel, for vd3d_dpt_head_tail_f32.  The scalar bias is read on the host ONCE per parameter
    version (_PerVersion: no per-call sync)."""
    tail = _PerVersion(lambda: (conv3.weight.detach().reshape(-1).contiguous(), float(conv3.bias.detach().float().item())))
    return lambda: tail.get(conv3.weight, conv3.bias)


_TUNABLE_DIR = None


def _tunable_scratch_dir() -> str:
    """One private scratch directory per process for TunableOp's results file (see DepthPipe._library_selection)."""
    global _TUNABLE_DIR
    if _TUNABLE_DIR is None:
        import atexit
        import glob
        import shutil
        import tempfile
        import time
        base = tempfile.gettempdir()
        for old in glob.glob(os.path.join(base, "vd3d_tunable_*")):   # what earlier processes of this user left behind (TunableOp writes at exit, after us)
            try:
                if os.stat(old).st_uid == os.getuid() and time.time() - os.stat(old).st_mtime > 86400:
                    shutil.rmtree(old, ignore_errors=True)
            except OSError:
                pass
        _TUNABLE_DIR = tempfile.mkdtemp(prefix="vd3d_tunable_")
        atexit.register(shutil.rmtree, _TUNABLE_DIR, True)
    return _TUNABLE_DIR


# DepthPipe(conv="bf16x3"): a 3 x 3 convolution takes vd3d_conv3x3_x3 from this many 8 x 32 output tiles (frames x tiles per frame, one workgroup each); below
# it the float32 library convolution stays.  Measured on the DA-V2-Small / -Base / -Large neck, fusion and head shapes (tools/probe_conv_x3.py,
# profiles/r08_conv_x3.md): every shape with 200 tiles or more ran in 0.59 - 0.97 of the library's time (MIOpen find mode on), every shape with 96 tiles or
# fewer (the 19 x 33 and 37 x 66 maps, where the library's split-K kernels fill the chip) in 1.06 - 2.76 of it; nothing was measured in between, so the rule
# is the smallest size that won.
CONV_X3_MIN_TILES = 200
# DepthPipe(gemm="fp16x2", conv="fp16x2") without self_contained: a 3 x 3 convolution takes vd3d_conv3x3_s1_x2 from this many 8 x 32 output tiles PER FRAME;
# below it the float32 library convolution stays.  The rule reads the map (and, through the weight image, the module), never the batch size: a frame's routes and
# bits do not depend on what it is batched with.  Measured on the DA-V2-Small / -Base / -Large neck, fusion and head shapes at the 4K patch grid, one frame
# and sixteen (tools/probe_fp16x2_self_contained.py --shapes, profiles/r18_fp16x2_self_contained.md; MIOpen find mode on), as kernel / library time: 171 tiles
# and more 0.39 - 0.71 at both batch sizes; 50 tiles (74 x 132) 0.45 - 0.73 at sixteen frames and 0.86 - 1.20 at one (break-even: four shapes win, two lose);
# 15 tiles (37 x 66) 0.49 - 0.63 at sixteen frames but 0.96 - 2.99 at one; 6 tiles 0.76 - 8.37.  Nothing was measured between 15 and 50, so the rule is the
# smallest size that did not lose on balance at one frame -- the batch a batch-blind rule has to be safe for.
CONV_X2_MIN_TILES = 50

# The A/B switches of the neck / head routes (environment variables): name -> (what unset or any other value means, when it is read, what "0" does); "1" reads True.
# VD3D_HEAD_CONV2_GATHER alone is tri-state: unset (None) the shape rule decides.  Setting one between two forwards of a pipe flips the per-forward ones.
_SWITCHES = {
    "VD3D_NECK_GLUE": (True, "construction", "the float32 neck / head keep the module graph's own bias, ReLU and add passes; every composed route below is off too"),
    "VD3D_HEAD_FUSED": (True, "forward", "head.conv2 and the tail stay three launches instead of one vd3d_dpt_head_conv_f32"),
    "VD3D_HEAD_CONV2_GATHER": (None, "forward", "the fused head launch keeps its conv form; 1: the gather form for every built C_in, unset: for HEAD_CONV2_GATHER_ROUTED"),
    "VD3D_HEAD_UPCONV": (True, "forward", "the last projection, its up-sampling and head.conv1 stay separate launches"),
    "VD3D_NECK_POLY": (True, "forward", "the reassemble stage's transposed convolution and neck.convs[i] stay two library calls"),
}


def _switch(name: str):
    """The A/B switch ``name`` of _SWITCHES as it stands in the environment NOW: False for "0", True for "1", the table's default for unset or anything else."""
    return {"0": False, "1": True}.get(os.environ.get(name), _SWITCHES[name][0])


class _ConvRouter:
    """Where the convolutions of the DPT neck / fusion stage / head of ``pipe`` run (Depth-Anything's rewrite and DPT-Large's / DPT-Hybrid's alike).  ``f32``: the float32
    glue is on (float32 pipe, VD3D_NECK_GLUE not "0"); without it every method here declines and the modules run as they are.
      * ``conv_nb(m, x)``: m's convolution WITHOUT its bias, counted for flops_per_frame (the modules' hooks are bypassed): ``conv_x2``, else ``conv_x3``, else the library's.
      * ``conv_x2``: ``gemm="fp16x2"`` with ``conv=None`` -- vd3d_conv3x3_x2 where it builds the shape and the launch has 256 tiles of 16 x 32 or more.
      * ``conv_x3``: ``conv="bf16x3"`` | ``"fp16x2"`` -- the 3 x 3 / stride 1 / padding 1 convolutions (``neck.convs``, the fusion stage's residual units, the head's
        two) on the tile convolution of the mode (Renderer.TILE_CONVS), one 8 x 32 tile kernel for every routed convolution: vd3d_conv3x3_x3, the three-term /
        six-product arithmetic of the GEMM (include/vd3d.h), or vd3d_conv3x3_s1_x2, the two-term fp16 arithmetic of its mode (three products per MAC, weights
        pre-scaled per output channel by an exact power of two, |x| < 65 504; vd3d_conv3x3_x2 stays the route of ``conv=None``) -- for 32 / 64 / 128 / 256 output
        channels and input channels in multiples of 16.  Maps below the measured launch-size rule stay on the library (CONV_X3_MIN_TILES tiles of 8 x 32 over the batch;
        CONV_X2_MIN_TILES PER FRAME in fp16x2, whose rule reads the map and the module, never the batch size); nothing else falls back.  ``pipe.conv_routes``
        (module name -> (mode | "library", reason)) records, per forward, where each of these convolutions ran and why.
      * ``self_contained=True``: no size rule -- EVERY 3 x 3 stride-1 convolution takes the tile convolution (DPT-Large: 4 x 4 to 48 x 48 maps at 384 x 384), the fusion layers'
        1 x 1 projections run as vd3d_gemm_x3 over the pixel rows (``conv1x1_x3``), and a module the mode cannot route is refused by name, never handed to a library.
    The weight images (``conv_img``, ``conv3_img``, ``gemm_img``) are keyed by id(module) and PACK ONCE, at first use: no parameter-version tracking (unlike _PerVersion)."""

    def __init__(self, pipe, f32: bool):
        self.pipe, self.R, self.f32, self.sc, self.cm, self.names = pipe, pipe.renderer, f32, pipe.self_contained, pipe.conv, pipe._names
        self.min_tiles = CONV_X2_MIN_TILES if self.cm == "fp16x2" else CONV_X3_MIN_TILES
        self.conv_img, self.conv3_img, self.gemm_img = {}, {}, {}   # None = shape not built
        if self.cm is not None and f32:   # neck.convs (3 x 3, no bias) are plain module calls in the stock neck: route them too (their forward hooks still count)
            for m in pipe.model.neck.convs:
                if self.sc and m.bias is not None:
                    raise NotImplementedError(f"self_contained=True: {self.names[id(m)]} has a bias (the stock neck convolutions have none) -- not built")
                if m.bias is None:
                    m.forward = lambda x, m=m: self._or_library(m, x, self.conv_x3(m, x))

    def record(self, label, operand, why, *modules):
        """The one route record: conv_routes[name] = (label, why) for each module where the route runs (``operand`` is not None), ("library", why) where not."""
        for m in modules:
            self.pipe.conv_routes[self.names[id(m)]] = (label if operand is not None else "library", why)

    def up(self, x, size):
        if x.dtype in (torch.bfloat16, torch.float32) and x.shape[1] % 8 == 0 and x.is_contiguous(memory_format=_CL):
            return self.R.upsample_bilinear(x, size)
        return F.interpolate(x, size=size, mode="bilinear", align_corners=True)

    def conv_x2(self, m, x):
        if self.pipe.gemm != "fp16x2" or self.cm is not None or not self.f32 or not _is_conv(m, 3, 1, 1) or x.dtype != torch.float32:
            return None
        if id(m) not in self.conv_img:
            self.conv_img[id(m)] = self.R.conv3x3_x2_pack(m.weight)
        # one workgroup per 16 x 32 output tile: below one tile per CU the library's split-K kernels win (19 x 33 maps with 768 input channels: measured 0.43 vs 0.17 ms)
        if self.conv_img[id(m)] is None or x.shape[0] * ((x.shape[2] + 15) // 16) * ((x.shape[3] + 31) // 32) < 256:
            return None
        return self.R.conv3x3_x2(x.contiguous(memory_format=_CL), self.conv_img[id(m)], m.out_channels)

    def conv_x3(self, m, x):
        cm, R = self.cm, self.R
        if cm is None or not self.f32 or not _is_conv(m, 3, 1, 1) or x.dtype != torch.float32:
            return None
        if id(m) not in self.conv3_img:
            self.conv3_img[id(m)] = R.conv3x3_tile_pack(m.weight, cm, 1)
        img = self.conv3_img[id(m)]
        if img is None:
            if self.sc:
                raise NotImplementedError(f"self_contained=True: {self.names[id(m)]}: vd3d_conv3x3_{R.TILE_CONVS[cm, 1]} does not build {m.in_channels} -> {m.out_channels} channels")
            return self.record(cm, None, f"shape not built: {m.in_channels} -> {m.out_channels} channels", m)
        why = "self-contained"   # no size rule: every map, the 19 x 33 ones included
        if not self.sc:
            # one workgroup per 8 x 32 output tile; fp16x2's rule reads the map alone, never the batch: a frame's route and bits do not depend on what it is batched with
            tiles = (1 if cm == "fp16x2" else x.shape[0]) * ((x.shape[2] + 7) // 8) * ((x.shape[3] + 31) // 32)
            if tiles < self.min_tiles:
                return self.record(cm, None, f"size rule: {tiles} tiles < {self.min_tiles}", m)
            why = f"{tiles} tiles"
        self.record(cm, img, why, m)
        return R.conv3x3_tile(x.contiguous(memory_format=_CL), img, m.out_channels, cm, 1)

    def _or_library(self, m, x, y):   # y, or the library's convolution of x by module m without its bias where no kernel took it (y is None): refused if self-contained
        if y is None and self.sc:
            raise NotImplementedError(f"self_contained=True: {self.names[id(m)]} is not a float32 3 x 3 / stride 1 / padding 1 convolution -- not built")
        return F.conv2d(x, m.weight, None, m.stride, m.padding, m.dilation, m.groups) if y is None else y

    def conv_nb(self, m, x):
        y = self.conv_x2(m, x)
        if y is None:
            y = self.conv_x3(m, x)
        if y is None:
            y = self._or_library(m, x, None).contiguous(memory_format=_CL)
        self.pipe._count_conv(m, y)
        return y

    def conv1x1_x3(self, m, x):
        """Self-contained: a 1 x 1 convolution WITHOUT its bias as vd3d_gemm_x3 over the pixel rows of a channels_last map (its NHWC storage is the row matrix)."""
        pipe, name = self.pipe, self.names[id(m)]
        if not _is_conv(m, 1, 1, 0) or m.in_channels % 16 or x.dtype != torch.float32:
            raise NotImplementedError(f"self_contained=True: {name} is not a float32 1 x 1 convolution with C_in a multiple of 16 -- not built")
        if id(m) not in self.gemm_img:
            self.gemm_img[id(m)] = self.R.gemm_x3_pack(m.weight.reshape(m.out_channels, m.in_channels), pipe.gemm)
        rows = x.contiguous(memory_format=_CL).permute(0, 2, 3, 1)   # [B, h, w, C] contiguous
        y = self.R.linear_x3(rows, self.gemm_img[id(m)], m.out_channels, None, mode=pipe.gemm).permute(0, 3, 1, 2)
        pipe.conv_routes[name] = (pipe.gemm, "self-contained: vd3d_gemm_x3 over the pixel rows")
        pipe._count_conv(m, y)   # what conv_nb adds for the same module
        return y

    def head_tail3(self, y1, conv1, conv2, size, tail, scale, act="relu"):
        """The three-launch head tail (DA and DPT): ``y1`` = conv1 without its bias -> the bias inside the align_corners up-sampling to ``size``, conv2 bias-free,
        then ONE launch for bias, ReLU, the 1 x 1 convolution to one channel (``tail()`` = its operands), bias, ReLU | Sigmoid and ``scale`` (vd3d_dpt_head_tail_f32 | vd3d_dpt_head_tail_act_f32: torch.sigmoid's CPU values)."""
        y = self.conv_nb(conv2, self.R.upsample_bilinear_bias(y1, size, conv1.bias))
        self.pipe._count_flops(2.0 * y.numel() / y.shape[0])   # the 1x1 convolution to one channel inside the tail kernel
        if act == "sigmoid":   # vd3d_dpt_head_tail_act_f32
            return self.R.dpt_head_tail(y, conv2.bias, *tail(), scale, act="sigmoid")
        return self.R.dpt_head_tail(y, conv2.bias, *tail(), scale)


class _Route:
    """A composed route of the default float32 mode (``gemm="f32"``, hence ``conv=None`` and no ``self_contained``; a renderer on the GPU; the float32 glue on).
    ``route(...)`` -> (operand | None, why): ``decide`` reads the route's switch (_SWITCHES, per forward) and its shape rules and takes the operand from a
    _PerVersion (composed and packed once per parameter version); _ConvRouter.record notes (``label`` | "library", why) under the names of ``modules``."""
    label, modules = None, ()

    def route(self, *args):
        operand, why = self.decide(*args)
        self.cr.record(self.label, operand, why, *self.modules)
        return operand, why


class _PolyRoute(_Route):
    """"f32-poly": an up-scaling reassemble stage's ConvTranspose2d ``rz`` (kernel == stride == f, bias) and the bias-free 3 x 3 neck convolution ``cv`` behind it are one
    linear map; composed on the coarse grid (neck_poly_compose) they run as ONE exact-float32 MFMA launch (vd3d_neck_poly_conv_f32: DA-V2-Base's and -Small's shapes)
    with 2.25 (f = 4) / 4 (f = 2) coarse taps per output pixel instead of 9 fine ones, and the fine map between them is never written.  conv_routes of both modules
    (``neck.reassemble_stage.layers.{0,1}.resize``, ``neck.convs.{0,1}``) read ("f32-poly", ...), or ("library", reason): a shape that is not built, VD3D_NECK_POLY=0.
    ``pending``: the packed blocks the reassemble stage hands to ``cv`` in this forward (None: it ran the transposed convolution itself)."""
    label = "f32-poly"

    def __init__(self, cr, rz, cv):
        self.cr, self.rz, self.cv, self.modules, self.pending = cr, rz, cv, (rz, cv), None
        self.packed = _PerVersion(lambda: cr.R.neck_poly_pack(*neck_poly_compose(rz.weight, rz.bias, cv.weight, rz.kernel_size[0]), rz.kernel_size[0]))
        cv.forward = self.conv_fwd

    def decide(self, x):
        rz, cv, f = self.rz, self.cv, self.rz.kernel_size[0]
        if x.dtype != torch.float32:
            return None, f"{x.dtype} map"
        if not _switch("VD3D_NECK_POLY"):
            return None, "VD3D_NECK_POLY=0"
        if not (rz.kernel_size == rz.stride == (f, f) and f >= 2 and rz.padding == (0, 0) and rz.output_padding == (0, 0) and rz.dilation == (1, 1) and rz.groups == 1
                and _is_conv(cv, 3, 1, 1) and cv.bias is None and cv.in_channels == rz.out_channels and cv.padding_mode == "zeros"):
            return None, "not a ConvTranspose2d with kernel == stride in front of a bias-free 3 x 3 / stride 1 / padding 1 convolution"
        packed = self.packed.get(rz.weight, rz.bias, cv.weight)
        if packed is None:
            return None, f"shape not built: {rz.in_channels} -> {cv.out_channels} channels, factor {f}"
        return packed, f"{rz.in_channels} -> {cv.out_channels} channels, factor {f}: {len(neck_poly_offsets(f))} composed blocks"

    def conv_fwd(self, x):
        rz, m, f = self.rz, self.cv, self.rz.kernel_size[0]
        packed, self.pending = self.pending, None
        if packed is None:
            return F.conv2d(x, m.weight, None, m.stride, m.padding, m.dilation, m.groups)
        self.cr.pipe._count_flops(2.0 * rz.out_channels * (f * x.shape[2]) * (f * x.shape[3]) * rz.in_channels * f * f)   # the bypassed transposed convolution's hook
        return self.cr.R.neck_poly_conv(x.contiguous(memory_format=_CL), packed)


class _UpconvRoute(_Route):
    """"f32-upconv": the LAST fusion layer's biased 1 x 1 projection ``proj``, its up-sampling and ``head.conv1`` (3 x 3, zero padding) are one linear map; all channel
    mixing runs as ONE library GEMM on the coarse map (head_upconv_compose: C -> 9 C_out channels) and vd3d_head_upconv_gather_f32 sums the 9 taps' bilinear samples
    per fine pixel: a quarter of conv1's flops, and neither the projected nor the up-sampled map is written.  conv_routes of both modules
    (``neck.fusion_stage.layers.<last>.projection``, ``head.conv1``) read ("f32-upconv", ...), or ("library", reason): a shape that is not built, VD3D_HEAD_UPCONV=0.
    ``armed``: inside the model's own forward, where the head consumes the neck's output (the neck called alone materialises the up-sampled projection as ever);
    ``pending``: (coarse map, target size, (Wc, bc)), what the last fusion layer hands to the head in this forward."""
    label = "f32-upconv"

    def __init__(self, cr, proj, conv1):
        self.cr, self.proj, self.conv1, self.modules, self.armed, self.pending = cr, proj, conv1, (proj, conv1), False, None
        self.wb = _PerVersion(lambda: head_upconv_compose(proj.weight, proj.bias, conv1.weight))
        model, model_fwd = cr.pipe.model, cr.pipe.model.forward

        def armed_fwd(*args, **kwargs):   # the head follows the neck in here and nowhere else
            self.armed, self.pending = True, None
            try:
                return model_fwd(*args, **kwargs)
            finally:
                self.armed, self.pending = False, None
        model.forward = armed_fwd

    def decide(self, tgt):
        pj, c1 = self.proj, self.conv1
        if not _switch("VD3D_HEAD_UPCONV"):
            return None, "VD3D_HEAD_UPCONV=0"
        if not (_is_conv(pj, 1, 1, 0) and pj.bias is not None and _is_conv(c1, 3, 1, 1) and c1.padding_mode == "zeros" and c1.in_channels == pj.out_channels):
            return None, "not a biased 1 x 1 projection in front of a 3 x 3 / stride 1 / padding 1 / zeros convolution"
        if (c1.in_channels, c1.out_channels) not in HEAD_UPCONV_BUILT:
            return None, f"shape not built: {c1.in_channels} -> {c1.out_channels} channels"
        if tgt[0] < 2 or tgt[1] < 2:
            return None, f"output {tgt[0]} x {tgt[1]} below 2 x 2"
        return self.wb.get(pj.weight, pj.bias, c1.weight), f"{pj.in_channels} -> 9 x {c1.out_channels} channels on the coarse map"

    def take(self, x):   # what the last fusion layer handed over in this forward (None: nothing) -- for the head, whose input x it must be
        pend, self.pending = self.pending, None
        if pend is not None and pend[0] is not x:
            raise RuntimeError("head_upconv: the head did not receive the last fusion layer's output")
        return pend

    def run(self, hc, tgt, wb):   # head.conv1 without its bias from the coarse map hc: the composed GEMM over its rows (the NHWC storage is the row matrix) and the gather
        hc = hc.contiguous(memory_format=_CL)
        B, Cc, hh, ww = hc.shape
        z = F.linear(hc.permute(0, 2, 3, 1).reshape(B * hh * ww, Cc), wb[0], wb[1])
        y1 = self.cr.R.head_upconv_gather(z.view(B, hh, ww, -1), tgt, self.conv1.out_channels)
        self.cr.pipe._count_flops(2.0 * self.proj.out_channels * hh * ww * Cc)   # the module graph's count: what conv_nb adds for the projection (on the coarse map) ...
        self.cr.pipe._count_conv(self.conv1, y1)                                # ... and for conv1
        return y1


class _HeadFusedRoute(_Route):
    """"f32-fused": the head's up-sampling, its second convolution and everything behind it as ONE exact-float32 MFMA launch (vd3d_dpt_head_conv_f32: 32 | 64 | 128 ->
    32 channels).  conv_routes["head.conv2"] reads ("f32-fused", ...), or ("library", reason) where the three launches stay (a shape that is not built,
    VD3D_HEAD_FUSED=0).  For 32 | 64 input channels (HEAD_CONV2_GATHER_ROUTED: a rule on the shape alone) the launch takes the "coarse GEMM + fine gather" form
    (vd3d_head_conv_gather_f32, composed by head_conv2_compose: all channel mixing on the coarse map, Z kept in LDS, a third of conv2's flops, close but not equal
    bits) where the launch is not refused; the reason string names the form, VD3D_HEAD_CONV2_GATHER=0 switches back and =1 routes every built count.  Operand: (image, form)."""
    label = "f32-fused"

    def __init__(self, cr, head, tail):
        self.cr, self.head, self.tail, self.modules = cr, head, tail, (head.conv2,)
        self.img = _PerVersion(lambda: cr.R.dpt_head_conv_pack(head.conv2.weight) if head.conv2.out_channels == 32 else None)
        self.gimg = _PerVersion(lambda: cr.R.head_conv_gather_pack(*head_conv2_compose(head.conv2.weight, head.conv1.bias)))

    def decide(self, in_size, size):
        head, m, sw = self.head, self.head.conv2, _switch("VD3D_HEAD_CONV2_GATHER")
        if not _switch("VD3D_HEAD_FUSED"):
            return None, "VD3D_HEAD_FUSED=0"
        if not _is_conv(m, 3, 1, 1):
            return None, "not a 3 x 3 / stride 1 / padding 1 convolution"
        img = self.img.get(m.weight)
        if img is None:
            return None, f"shape not built: {m.in_channels} -> {m.out_channels} channels"
        if head.conv1.bias.data_ptr() % 16 or m.bias.data_ptr() % 16 or self.tail()[0].data_ptr() % 16:
            return None, "a bias or the 1x1 weight is not 16-byte aligned"
        if size[0] < 2 or size[1] < 2:
            return None, f"output {size[0]} x {size[1]} below 2 x 2"
        # the gather form: where the channel count is routed, a tile serves the ratio (else the launch would be refused) and the image is built
        if (sw is not False and m.out_channels == 32 and m.in_channels in (HEAD_CONV2_GATHER_BUILT if sw else HEAD_CONV2_GATHER_ROUTED) and m.padding_mode == "zeros"
                and self.cr.R.head_conv_gather_tile(in_size, size, m.in_channels) is not None and self.gimg.get(m.weight, head.conv1.bias) is not None):
            return (self.gimg.value, "gather"), f"{m.in_channels} -> {m.out_channels} channels, form gather (coarse GEMM + fine gather)"
        return (img, "conv"), f"{m.in_channels} -> {m.out_channels} channels, form conv"


class _FusionStage:
    """The fusion stage of ``pipe`` (transformers FeatureFusionLayer / PreActResidualLayer, reproduced verbatim otherwise; DA and DPT alike) with the float32 glue on:
    every convolution runs WITHOUT its bias pass (_ConvRouter.conv_nb) and the glue between two convolutions is one HIP launch -- bias + ReLU in place behind a
    unit's first convolution; bias + unit input (+ the fusion layer's running state) behind its second one, which also writes the ReLU'd copy the next unit starts
    from; the layer's 1 x 1 projection runs BEFORE its up-sampling (both are linear and per-pixel / per-channel: conv1x1(up(x)) == up(conv1x1(x)), a quarter of the
    pixels) and hands its bias to the up-sampling kernel (interpolation weights sum to one).  The last layer hands its coarse map to ``upconv`` where that route runs."""

    def __init__(self, pipe, cr, upconv=None):
        self.pipe, self.cr, self.upconv, self.last = pipe, cr, upconv, pipe.model.neck.fusion_stage.layers[-1]
        for layer in pipe.model.neck.fusion_stage.layers:
            layer.forward = lambda hidden_state, residual=None, size=None, layer=layer: self.forward(layer, hidden_state, residual, size)

    def res_unit(self, unit, x, x_relu=None, extra=None, want_relu=False):
        """PreActResidualLayer: conv2(relu(conv1(relu(x)))) + x [then extra + that]; optionally also relu(result)."""
        R, conv_nb = self.cr.R, self.cr.conv_nb
        x = x.contiguous(memory_format=_CL)
        h = torch.relu(x) if x_relu is None else x_relu
        y = R.bias_act(conv_nb(unit.convolution1, h), unit.convolution1.bias, relu=True)
        y = conv_nb(unit.convolution2, y)
        return R.bias_act(y, unit.convolution2.bias, r1=x, r2=extra, want_relu_copy=want_relu)

    def forward(self, layer, hidden_state, residual, size):
        cr, res_unit, up = self.cr, self.res_unit, self.upconv
        fused = cr.f32 and hidden_state.dtype == torch.float32 and hidden_state.shape[1] % 4 == 0
        if residual is not None:
            if hidden_state.shape != residual.shape:
                residual = F.interpolate(residual, size=(hidden_state.shape[2], hidden_state.shape[3]), mode="bilinear", align_corners=False)
            if fused:
                hidden_state, hr = res_unit(layer.residual_layer1, residual, extra=hidden_state.contiguous(memory_format=_CL), want_relu=True)
                hidden_state = res_unit(layer.residual_layer2, hidden_state, x_relu=hr)
            else:
                hidden_state = layer.residual_layer2(hidden_state + layer.residual_layer1(residual))
        else:
            hidden_state = res_unit(layer.residual_layer2, hidden_state) if fused else layer.residual_layer2(hidden_state)
        tgt = (2 * hidden_state.shape[2], 2 * hidden_state.shape[3]) if size is None else tuple(size)
        if cr.sc and not (fused and layer.projection.bias is not None):
            raise NotImplementedError(f"self_contained=True: {cr.names[id(layer)]}: a float32 map with channels in multiples of 4 and a projection with a bias expected")
        if fused and layer is self.last and up is not None and up.armed:
            wb, _ = up.route(tgt)
            if wb is not None:
                up.pending = (hidden_state, tgt, wb)
                return hidden_state   # the residual output on the coarse map: the head runs the composed GEMM and the gather on it
        if fused and layer.projection.bias is not None:
            return cr.R.upsample_bilinear_bias((cr.conv1x1_x3 if cr.sc else cr.conv_nb)(layer.projection, hidden_state), tgt, layer.projection.bias)
        return layer.projection(cr.up(hidden_state, tgt))


class _DaHead:
    """Depth-Anything's DepthEstimationHead in three forms.  With the float32 glue on and a head of the stock shape ([conv 3 x 3, up-sampling, conv 3 x 3 -> 16 / 32 /
    64, ReLU, conv 1 x 1, ReLU] with biases; the metric heads' Sigmoid() * max_depth under self_contained=True only -- without the keyword they route as they always
    did): conv1 bias-free (or the ``upconv`` route's gather on the coarse map the last fusion layer handed through), then either ONE launch for the rest (``fused``,
    in conv or gather form) or the three-launch tail (_ConvRouter.head_tail3).  Anything else: the stock module graph on vd3d_upsample_bilinear_nhwc."""

    def __init__(self, pipe, cr):
        self.pipe, self.cr, self.head, self.tail, self.fused, self.upconv = pipe, cr, pipe.model.head, None, None, None
        head, sc, layers = self.head, pipe.self_contained, pipe.model.neck.fusion_stage.layers
        self.tail_act = "relu" if isinstance(head.activation2, torch.nn.ReLU) else "sigmoid" if sc and isinstance(head.activation2, torch.nn.Sigmoid) else None
        if (cr.f32 and self.tail_act is not None and head.conv2.out_channels in (16, 32, 64) and head.conv3.kernel_size == (1, 1)
                and head.conv2.bias is not None and head.conv3.bias is not None and head.conv1.bias is not None):
            self.tail = _head_tail_operands(head.conv3)
        if sc and self.tail is None:
            raise NotImplementedError(f"self_contained=True: {pipe.name!r}: a depth head other than [conv 3 x 3, up-sampling, conv 3 x 3 -> 16 / 32 / 64, ReLU, conv 1 x 1, "
                                      f"ReLU | Sigmoid] with biases (its last activation is {type(head.activation2).__name__}) -- not built")
        if pipe.gemm == "f32" and pipe.device.type == "cuda" and self.tail is not None:   # (the kernels read device memory: a pipe on the CPU keeps its graph)
            self.fused = _HeadFusedRoute(cr, head, self.tail)
            if head.head_in_index in (-1, len(layers) - 1):
                self.upconv = _UpconvRoute(cr, layers[-1].projection, head.conv1)
        head.forward = self.forward

    def forward(self, hidden_states, patch_height, patch_width):
        head, cr = self.head, self.cr
        x = hidden_states[head.head_in_index]
        size = (int(patch_height * head.patch_size), int(patch_width * head.patch_size))
        pend = self.upconv.take(x) if self.upconv is not None else None
        if self.tail is None or x.dtype != torch.float32:
            h = cr.up(head.conv1(x), size)
            h = head.conv3(head.activation1(head.conv2(h)))
            return (head.activation2(h) * head.max_depth).squeeze(dim=1)
        op = self.fused.route((int(x.shape[2]), int(x.shape[3])) if pend is None else pend[1], size)[0] if self.fused is not None else None
        y1 = self.upconv.run(*pend) if pend is not None else cr.conv_nb(head.conv1, x.contiguous(memory_format=_CL))   # head.conv1 without its bias
        if op is None:
            return cr.head_tail3(y1, head.conv1, head.conv2, size, self.tail, float(head.max_depth), self.tail_act)
        n_out = float(head.conv2.out_channels) * size[0] * size[1]
        self.pipe._count_flops(2.0 * n_out * head.conv2.in_channels * 9 + 2.0 * n_out)   # exactly what conv_nb(head.conv2, .) and head_tail3's tail line add
        return cr.R.dpt_head_conv(y1, head.conv1.bias, size, op[0], head.conv2.bias, *self.tail(), float(head.max_depth), form=op[1])


class DepthPipe:
    """``pipe(images, inference_size=None) -> [{"predicted_depth": Tensor[h, w]}]`` (reference protocol) plus a
    device-resident batch path.  OPT-IN tiled high-resolution depth (the reference's USE_TILED_DEPTH tiler, with a renderer):
    ``infer_tiled_bgr_u8`` (batched equal-shape tiles, Hann blend on the device), ``depth_frames_u8(tiled=True)`` (percentile
    hand-off) and ``call_tiled`` (reference protocol); the defaults are unchanged."""

    def __init__(self, name: str = "depth-anything-v2-small", device="cuda", dtype=torch.float32, seed: int = 0,
                 channels_last: bool = True, renderer=None, fuse_backbone: bool = True, model=None, processor: dict | None = None,
                 tuned_gemm: bool = True, miopen_find: bool | None = None, gemm: str = "f32", conv: str | None = None, self_contained: bool = False,
                 front_end: str = "float", encoders: str | None = None, decoder: str | None = None):
        """``dtype``: float32 (the reference's precision, default) or bfloat16.
        ``front_end``: ``"float"`` (default) -- the network input is the float32 statement of the image processor's antialiased bicubic resize, never
        rounded (``vd3d_depth_preprocess`` with a renderer, ATen otherwise).  ``"pil"`` -- OPT-IN: the input the reference process builds, bit for bit.
        The reference hands its pipeline PIL images, so the optional ``img.resize(inference_size, Image.BICUBIC)`` and the image processor's resize are
        Pillow's 8-bit resampler, which rounds to uint8 after each pass; rescale and normalise are then a table of the byte.  With a renderer this is
        one launch of ``vd3d_depth_preprocess_pil`` (two with an inference size); on the CPU, and for a geometry past the kernel's tap budget, the
        integer statement ``pil_resample.pixel_values`` gives the same values.  ``front_end_route`` ("kernel" | "statement") says which ran last.
        The mode takes uint8 frames only (TypeError otherwise).  Any other value of the keyword raises ValueError.
        DepthPro (``"depth-pro"``, ``DepthProForDepthEstimation``: apple/DepthPro-hf; ``depth_pro.py`` states the geometry as far as it is known here): ``__call__``,
        ``infer_bgr_u8``, ``depth_frames_u8`` and ``at_inference_size`` give what ``pipeline("depth-estimation")`` gives -- the processor's own order (rescale and normalise,
        THEN a bilinear resize without antialias to 1536 x 1536: ``front_end="float"``; ``"pil"`` is refused by name, there is no Pillow pass in this processor), the
        model, and the processor's post-process at the size the pipeline saw: depth x width / focal from the model's field of view, bilinear resize, 1 / clamp(depth,
        1e-4, 1e4).  With a renderer both ends are one launch each (``vd3d_depthpro_preprocess_u8`` for uint8 frames without an ``inference_size`` -- with one, or for
        other frame types, the front end runs as ATen operators and ``front_end_route`` reads "statement" instead of "kernel"; ``vd3d_depthpro_post_f32``, the field of
        view never leaves the device); on the CPU the same arithmetic runs in ATen.  ``raw=True`` returns the MODEL-RESOLUTION inverse depth (scale for the model's width, clamp, reciprocal,
        no resize) -- a deviation: the pipeline resizes before the reciprocal.  A model without the field-of-view branch is not scaled.  The network itself runs its
        stock float32 graph: ``gemm="bf16x3"`` / ``"fp16x2"`` and ``self_contained=True`` refuse DepthPro by name (the rewrite is not built), and so does tiled depth
        (its blend evaluates a bicubic post-process); ``bars=`` consumes the uint8 planes and works unchanged.
        ``encoders`` (DepthPro only; float32 + ``renderer``): ``None`` (default) -- the stock graph, as above.  ``"bf16x3"`` / ``"fp16x2"`` -- OPT-IN: from ``pixel_values``
        to the inputs of ``DepthProNeck`` (and to the input of the field-of-view model's convolution) no vendor-library call is made: the patch pyramid is one launch
        (``vd3d_depthpro_patches_f32``), the patch embeddings are ``vd3d_patchify_f32`` + ``vd3d_gemm_x3``, every ``Dinov2Layer`` of the patch, image and
        field-of-view encoders is a ``vit_blocks._split_block`` in the named arithmetic, the final LayerNorms are ``vd3d_add_layernorm``, the field-of-view ``neck`` Linear is
        ``vd3d_gemm_x3`` and every ``reconstruct_feature_maps`` is ``vd3d_depthpro_merge_f32`` (``_route_depth_pro_encoders``).  The neck, the fusion stage, the head
        and the field-of-view convolutions stay the stock module graph on the float32 library, which is why ``gemm=`` / ``self_contained=True`` keep refusing DepthPro.
        ``decoder`` (DepthPro only; needs ``encoders``, whose mode it may differ from): ``None`` (default) -- the neck, fusion stage, head and field-of-view convolutions
        stay the stock module graph, as above.  ``"bf16x3"`` / ``"fp16x2"`` -- OPT-IN: they run on this project's kernels in the named arithmetic
        (``depth_pro.DecoderRoutes`` lists the route of every module; ``depth_pro.decoder_scope`` refuses, by name and before the module moves, what the routes do not
        take), so that between ``pixel_values`` and ``predicted_depth`` / ``field_of_view`` no convolution, matrix-product or attention operator of ATen is dispatched.
        ``pipe.decoder`` records the mode, ``pipe.decoder_routes`` (module name -> route) where every Conv2d / ConvTranspose2d of the decoder ran in the last forward.
        ``pipe.encoders`` records the mode (or None), ``pipe.encoders_resize`` whether the image / field-of-view encoders read the pyramid's quarter level
        ("pyramid") or resized for themselves ("aten").  Any other model, value or geometry is refused by name at construction.
        ``gemm`` (float32 + ``renderer`` only; round 6): ``"f32"`` (default) -- the four linears of every transformer block are hipBLASLt's float32
        GEMMs and the attention (64-wide heads) is the library's exact-float32 kernel (``vd3d_attention_f32``: both products on the float32-input
        matrix cores, float32 online softmax); ``"bf16x3"`` -- OPT-IN: the library's own split-bf16 GEMM (``vd3d_gemm_x3``: every float32 operand exactly split into three bf16
        terms, six products per MAC on the bf16 matrix cores, float32 accumulation -- float32-faithful, see include/vd3d.h), with the exact GELU
        folded into fc1's epilogue, and the attention in the same arithmetic (``vd3d_attention_x3``: both products split-bf16, float32 online softmax).
        ``"fp16x2"`` -- OPT-IN: the same kernels with every operand as TWO fp16 terms (22 significant bits, round to nearest) and three products per MAC
        -- half the matrix work of bf16x3; weights pre-scaled per row, activations must stay below 65 504 in front of every linear and convolution and q, k, v below 4 094 in front of the
        attention, which scales them by 2^4 before its split (larger values give Inf / NaN, never a finite wrong number: include/vd3d.h).  gfx950 has no TF32 and its float32-input MFMA runs at 1/16 of the bf16 rate, which caps the default mode.
        The split modes cover the DINOv2 family (Depth-Anything V1 / V2, Distill-Any-Depth) and DPT-Large (a plain-ViT ``DPTForDepthEstimation`` with
        readout_type="project"; its readout / 1x1 projections and the transposed convolutions of the reassemble stage go on ``vd3d_gemm_x3`` too, see
        ``_patch_dpt_vit_reassemble_head``) and DPT-Hybrid in its published geometry (``"dpt-hybrid-midas"``, MiDaS 3.0: ViT-B/16 behind a BiT ResNet-50 prefix;
        ``_split_scope`` states the geometry; ``_patch_hybrid_embeddings`` what runs where: the prefix stays the module graph on the float32 library unless
        ``self_contained`` is given).  Anything else -- any other hybrid, BEiT / Swin backbones, ZoeDepth, DepthPro -- raises NotImplementedError; with ``gemm="f32"``
        a DPT model runs its stock module graph unchanged.
        ``conv``: ``None`` (default) -- the 3 x 3 convolutions of the DPT neck / fusion stage / head run as they always did per mode: library float32
        convolutions in ``"f32"`` and ``"bf16x3"``, ``vd3d_conv3x3_x2`` where its rules allow in ``"fp16x2"``.  ``"bf16x3"`` / ``"fp16x2"`` -- OPT-IN, only with
        the ``gemm`` of the same name (else ValueError): the 3 x 3 / stride 1 / padding 1 convolutions of the neck, the fusion stage and the head (DA and DPT-Large
        alike) run on the tile convolution of the mode above a measured launch-size rule, and ``conv_routes`` (module name -> (mode | "library", reason)) records, per
        forward, where each ran and why: ``_ConvRouter``.  The default float32 mode (``gemm="f32"``, hence ``conv=None``; with a renderer) composes three routes of its own, each
        recorded in ``conv_routes`` and each with an A/B switch (``_SWITCHES``): ``_HeadFusedRoute`` ("f32-fused"), ``_PolyRoute`` ("f32-poly"), ``_UpconvRoute`` ("f32-upconv").
        ``renderer``: a ``visiondepth3d_amd.render_3d.Renderer`` on the SAME stream as the network (default stream); when given the
        image-processor front end, the residual-add + LayerNorm pairs and the DPT up-samplings run as fused HIP launches.
        ``model`` / ``processor``: an already constructed Hugging Face depth model and its image-processor constants
        (``from_pretrained``); otherwise the architecture ``name`` is built from MODEL_ZOO with synthetic weights.
        Library selection (the GEMMs / convolutions stay library calls, north_star): ``tuned_gemm`` loads the committed hipBLASLt solution
        table ``tuned/gemm_gfx950.csv`` (PyTorch TunableOp, tuning OFF: a look-up per GEMM shape; written by tools/probe_net_tune.py on an
        MI355X; ignored when its library-version validators do not match; ``VD3D_TUNED_GEMM=0`` disables).  ``miopen_find``: MIOpen
        find mode (``torch.backends.cudnn.benchmark``) -- every convolution shape times its applicable solvers once, ~25 s at the
        first forward of a process, 4.5 % on the 4K float32 forward (profiles/r04_net_library_selection.md); opt-in, bench.py uses it.
        The flag is PyTorch's process-wide one: True / False set it, None (default) leaves it as the caller has it.
        ``self_contained``: ``False`` (default) -- everything above.  ``True`` -- OPT-IN, only with ``gemm="bf16x3"``, ``conv="bf16x3"`` or ``gemm="fp16x2"``, ``conv="fp16x2"``, float32, a renderer on a
        GPU and ``fuse_backbone=True`` (else ValueError naming what is missing), and only for the models of the split modes -- ``DepthAnythingForDepthEstimation`` on
        ``Dinov2Backbone`` whose head ends in ReLU (relative) or Sigmoid (metric: Depth-Anything-V2-Metric-*), and DPT-Large as ``_split_scope`` accepts it
        and DPT-Hybrid likewise (else NotImplementedError naming the model, raised before the renderer or a device is touched): the forward makes NO hipBLASLt / MIOpen / AOTriton call.
        On top of the two split modes every remaining convolution takes a kernel of the mode's pair -- the patch embedding (``_patch_patch_embedding``), the reassemble
        stage (``_self_contained_reassemble``; DPT: ``_patch_dpt_vit_reassemble_head``), ``neck.convs``, the fusion stage and the head at every map size
        (``_ConvRouter``, ``_DaHead``: a metric head's ``Sigmoid() * max_depth`` runs inside the tail launch), DPT-Hybrid's BiT prefix (``_BitPrefix``) -- and a module
        the mode cannot route is refused by name, never handed to a library.  ``conv_routes`` names every routed module and holds no ``"library"`` value; with the
        fp16x2 pair its labels read ``("fp16x2", "self-contained...")`` and the mode's range contract holds in front of every route.  The library selection is skipped:
        TunableOp is not enabled, ``torch.backends.cudnn.benchmark`` is not touched, ``tuned_gemm`` / ``miopen_find`` read False.  Per output element every kernel sums
        in one fixed order and nothing is split along K, so a frame's prediction does not depend on the batch it is in or on the ROCm release's solution tables."""
        self.name, self.device, self.dtype = name, torch.device(device), dtype
        if gemm not in ("f32", "bf16x3", "fp16x2"):
            raise ValueError("gemm must be 'f32', 'bf16x3' or 'fp16x2'")
        if conv not in (None, "bf16x3", "fp16x2"):
            raise ValueError("conv must be None, 'bf16x3' or 'fp16x2'")
        if self_contained:
            # the two pairs of the mode; the bf16x3 pair leads the wording, a half-given bf16x3 pair names its missing half alone
            pair = (gemm, conv) in (("bf16x3", "bf16x3"), ("fp16x2", "fp16x2"))
            missing = [what for what, ok in (("gemm='bf16x3', conv='bf16x3' (or gemm='fp16x2', conv='fp16x2')", pair or gemm == "bf16x3"),
                                             ("conv='bf16x3'", pair or gemm != "bf16x3"), ("dtype=torch.float32", dtype == torch.float32),
                                             ("a renderer on a GPU", renderer is not None and torch.device(device).type == "cuda"),
                                             ("fuse_backbone=True", bool(fuse_backbone)),
                                             ("the neck glue launches (VD3D_NECK_GLUE=0 is set)", _switch("VD3D_NECK_GLUE"))) if not ok]
            if missing:
                raise ValueError("self_contained=True needs " + ", ".join(missing))
        if conv is not None and gemm != conv:
            raise ValueError(f"conv={conv!r} is the convolution half of gemm={conv!r} and needs that mode")
        if gemm != "f32" and (dtype != torch.float32 or renderer is None or torch.device(device).type != "cuda"):
            raise ValueError("gemm='bf16x3' / 'fp16x2' are modes of the float32 pipe on the GPU and need a renderer (the kernels live in libvd3d_hip.so)")
        if front_end not in ("float", "pil"):
            raise ValueError("front_end must be 'float' or 'pil'")
        if encoders not in (None, "bf16x3", "fp16x2"):
            raise ValueError("encoders must be None, 'bf16x3' or 'fp16x2'")
        if encoders is not None and (dtype != torch.float32 or renderer is None or torch.device(device).type != "cuda"):
            raise ValueError("encoders='bf16x3' / 'fp16x2' are modes of the float32 pipe on the GPU and need a renderer (the kernels live in libvd3d_hip.so)")
        if decoder not in (None, "bf16x3", "fp16x2"):
            raise ValueError("decoder must be None, 'bf16x3' or 'fp16x2'")
        if decoder is not None and encoders is None:
            raise ValueError(f"decoder={decoder!r} needs encoders='bf16x3' | 'fp16x2': the patch merges of the routed encoders hand over the NHWC storage the decoder's "
                             "routes read")
        self.encoders, self.encoders_resize = None, {}
        self.decoder, self.decoder_routes = None, {}
        self.front_end, self.front_end_route = front_end, None
        self.gemm, self.conv, self.self_contained = gemm, conv, bool(self_contained)
        self.conv_routes = {}
        self.tuned_gemm = self.miopen_find = False
        self._flop_count = None
        if self.device.type == "cuda" and not self.self_contained:   # self-contained: no library call to select for
            self._library_selection(tuned_gemm, miopen_find)
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("DepthPipe runs in float32 (reference precision) or bfloat16")
        if model is None:
            cfg = build_config(name)
            if MODEL_ZOO[name]["arch"] == "depth_pro":
                from transformers import DepthProForDepthEstimation as Net
            elif MODEL_ZOO[name]["arch"] == "dpt":
                from transformers import DPTForDepthEstimation as Net
            else:
                from transformers import DepthAnythingForDepthEstimation as Net
            model = Net(cfg).eval()
            synthetic_weights_(model, seed)
            processor = processor or PROCESSORS[MODEL_ZOO[name]["arch"]]
        self.arch = {"DepthAnythingForDepthEstimation": "da", "DepthProForDepthEstimation": "depth_pro"}.get(type(model).__name__, "generic")
        if self.arch == "depth_pro":
            if front_end == "pil":   # the processor is no Pillow resize: it normalises first and resizes the FLOAT image (torchvision, no antialias)
                raise NotImplementedError(f"front_end='pil': {name!r} (DepthProForDepthEstimation) -- DepthProImageProcessor rescales and normalises first and resizes the float "
                                          "tensor bilinearly without antialias; there is no 8-bit Pillow pass to reproduce, front_end='float' IS the processor's own order")
            if gemm != "f32" or self_contained:   # refused by name before the renderer or a device is touched
                self.model = model
                self._split_scope(fuse_backbone)
            if processor is None:
                processor = PROCESSORS["depth_pro"]
        if encoders is not None:   # refused by name on the module graph as it was handed in: nothing moved to a device yet
            self.model = model
            enc_plan = self._depth_pro_encoders_scope(encoders, processor)
        if decoder is not None:    # likewise: refused by name before anything moves
            from . import depth_pro
            depth_pro.decoder_scope(model, name, decoder, enc_plan["size"])
        if self.self_contained:   # refused here, by name, on the module graph as it was handed in: no renderer call, nothing moved to a device yet
            self.model = model
            scope = self._split_scope(fuse_backbone)
            if scope == "dpt-hybrid":   # the BiT prefix: every module the mode cannot route is refused by name here
                bit_prefix_plan(model.dpt.embeddings.backbone, {id(m): n for n, m in model.named_modules()})
            if scope == "dinov2":
                bc = model.config.backbone_config
                if not head_geometry_ok(bc.hidden_size, bc.num_attention_heads):
                    raise NotImplementedError(f"self_contained=True: {name!r}: hidden size {bc.hidden_size} with {bc.num_attention_heads} heads -- vd3d_attention_x3 and "
                                              "vd3d_add_layernorm are built for 384 / 768 / 1024 with 64-wide heads; anything else would run library attention")
                act2 = getattr(model.head, "activation2", None)
                if not isinstance(act2, (torch.nn.ReLU, torch.nn.Sigmoid)):
                    raise NotImplementedError(f"self_contained=True: {name!r} ({type(model).__name__}): the depth head ends in {type(act2).__name__} -- the head tail "
                                              "(vd3d_dpt_head_tail_f32 / vd3d_dpt_head_tail_act_f32) is built for ReLU (relative) and Sigmoid (metric) only")
        self.proc = dict(PROCESSORS["da"] if processor is None else processor)
        self.model = model.eval().to(self.device, dtype)
        if channels_last and self.device.type == "cuda":
            self.model = self.model.to(memory_format=torch.channels_last)
        self._names = {id(m): n for n, m in self.model.named_modules()}   # built once, here: every rewrite and every conv_routes key reads it
        self.mean = torch.tensor(self.proc["mean"], device=self.device, dtype=torch.float32).view(1, 3, 1, 1)
        self.std = torch.tensor(self.proc["std"], device=self.device, dtype=torch.float32).view(1, 3, 1, 1)
        self.n_params = sum(p.numel() for p in self.model.parameters())
        self.renderer = renderer if (renderer is not None and self.device.type == "cuda") else None
        dino = self.arch == "da" and type(self.model.backbone).__name__ == "Dinov2Backbone"
        # dpt_vit: DPT-Large's rewrite runs (split modes only; arch stays "generic": gemm="f32" keeps the stock DPT module graph)
        # dpt_hybrid: DPT-Hybrid's rewrite runs (dpt_vit is set too: the ViT half, the reassemble stage, the neck and the head are DPT-Large's rewrite)
        self.dpt_vit = self.dpt_hybrid = False
        scope = self._split_scope(fuse_backbone) if self.gemm != "f32" else None
        if scope == "dpt-vit":
            self._rewrite_dpt_vit()
            if self.self_contained:
                self._patch_patch_embedding(self.model.dpt.embeddings.patch_embeddings)
        elif scope == "dpt-hybrid":
            self.dpt_hybrid = True
            self._rewrite_dpt_vit()
            self._patch_hybrid_embeddings()
        if dino:
            self._cache_position_embeddings()
            if fuse_backbone:
                self._fuse_backbone_layers()
            if self.renderer is not None:
                self._patch_dpt_upsampling()
            if self.self_contained:
                self._patch_patch_embedding(self.model.backbone.embeddings.patch_embeddings)
        if encoders is not None:
            self._route_depth_pro_encoders(encoders, enc_plan)
        if decoder is not None:
            from . import depth_pro
            with torch.no_grad():
                depth_pro.DecoderRoutes(self, decoder)
            self.decoder = decoder

    def _library_selection(self, tuned_gemm: bool, miopen_find):
        if miopen_find is not None:
            torch.backends.cudnn.benchmark = bool(miopen_find)
        self.miopen_find = bool(torch.backends.cudnn.benchmark)
        table = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gemm_gfx950.csv")
        if not tuned_gemm or os.environ.get("VD3D_TUNED_GEMM", "1") == "0" or not os.path.exists(table):
            return
        try:
            import tempfile
            import torch.cuda.tunable as tn
            if tn.is_enabled():       # the caller drives TunableOp itself (tools/probe_net_tune.py, PYTORCH_TUNABLEOP_ENABLED=1)
                return
            tn.enable(True)
            tn.tuning_enable(False)
            # never write into the package.  TunableOp rewrites its results file when the process exits and this build has no switch for that: the
            # file lives in a PRIVATE per-process directory (mkdtemp: mode 0700, unpredictable name -- no race between the ranks of --gpus N, no
            # symlink to clobber in a shared /tmp) that an atexit hook registered BEFORE TunableOp's own write... cannot rely on ordering,
            # so the hook removes what exists and the directory is also swept at the next start-up of the same user (stale entries older than a day)
            tn.set_filename(os.path.join(_tunable_scratch_dir(), "tunableop_results.csv"))
            self.tuned_gemm = bool(tn.read_file(table))
            if not self.tuned_gemm:   # other hipBLASLt / rocBLAS / PyTorch build: the solution indices mean nothing there
                tn.enable(False)
        except Exception:             # TunableOp missing in this build: the heuristic selection is the same math
            self.tuned_gemm = False

    @classmethod
    def from_pretrained(cls, path: str, device="cuda", dtype=torch.float32, **kw) -> "DepthPipe":
        """A local Hugging Face checkpoint folder (config.json + model.safetensors [+ preprocessor_config.json]) -- the reference's
        local-model branch, ``AutoModelForDepthEstimation.from_pretrained(checkpoint)`` + ``AutoProcessor.from_pretrained(checkpoint)``
        (core/render_depth.py:756-760).  DepthAnything / DINOv2 checkpoints (Depth-Anything V1 / V2, Distill-Any-Depth) then get the
        fused-weight rewrites (one QKV GEMM, LayerScale folded into the projections); any other depth architecture
        (DPT / MiDaS 3.0, ZoeDepth ...) runs its stock module graph behind the same protocol -- except that a plain-ViT DPT checkpoint
        (Intel/dpt-large) with ``gemm="bf16x3" / "fp16x2"`` and a renderer in ``kw`` gets the split-mode rewrite (``__init__``)."""
        from transformers import AutoModelForDepthEstimation
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path}: not a local checkpoint folder (this build environment has no network)")
        model = AutoModelForDepthEstimation.from_pretrained(path, local_files_only=True)
        pro = type(model).__name__ == "DepthProForDepthEstimation"
        proc = dict(PROCESSORS["da" if type(model).__name__ == "DepthAnythingForDepthEstimation" else "depth_pro" if pro else "dpt"])
        pc = os.path.join(path, "preprocessor_config.json")
        if os.path.exists(pc):
            with open(pc) as f:
                j = json.load(f)
            sz = j.get("size") or {}
            if isinstance(sz, dict) and "height" in sz:
                proc["size"] = (int(sz["height"]), int(sz["width"]))
            elif isinstance(sz, int):
                proc["size"] = (sz, sz)
            proc["keep_aspect_ratio"] = bool(j.get("keep_aspect_ratio", proc["keep_aspect_ratio"]))
            proc["multiple"] = int(j.get("ensure_multiple_of", proc["multiple"]))
            if j.get("image_mean") is not None:
                proc["mean"] = tuple(float(v) for v in j["image_mean"])
            if j.get("image_std") is not None:
                proc["std"] = tuple(float(v) for v in j["image_std"])
            if pro:   # DepthProImageProcessor: bilinear (PIL resample 2) on the normalised float image, the one processor built with that filter
                if int(j.get("resample", 2)) != 2 or not all(j.get(k, True) for k in ("do_resize", "do_rescale", "do_normalize")):
                    raise NotImplementedError("a DepthPro image processor other than rescale + normalise + bilinear resize (PIL resample 2) is not built")
            elif int(j.get("resample", 3)) != 3:
                raise NotImplementedError("image processors other than bicubic (PIL resample 3) are not built")
        return cls(os.path.basename(os.path.normpath(path)), device=device, dtype=dtype, model=model, processor=proc, **kw)

    def resize_target(self, h: int, w: int):
        return dpt_resize_target(h, w, self.proc["size"], self.proc["multiple"], self.proc["keep_aspect_ratio"])

    def _cache_position_embeddings(self):
        """DINOv2 re-interpolates its position embedding (bicubic 37x37 -> patch grid) on EVERY forward; for a fixed
        frame size the result is a constant, and ATen's bicubic kernel loops the 384-1024 channels serially per output
        pixel (measured 2.9 ms per forward on MI355X, 14 % of the step).  Memoise it per (height, width)."""
        _memoise(self.model.backbone.embeddings, "interpolate_pos_encoding", lambda t, height, width: (int(height), int(width), t.dtype, t.shape[1]))

    def _count_conv(self, m, y):
        """flops_per_frame: a convolution module m that a rewrite runs without calling it adds, for its output y, what the counting hook would have added."""
        self._count_flops(2.0 * y.numel() / y.shape[0] * (m.in_channels // m.groups) * m.kernel_size[0] * m.kernel_size[1])

    def _count_flops(self, n: float):
        """flops_per_frame: ``n`` flops a rewrite executes outside any counted convolution module (the only two places that add to the count: this and _count_conv)."""
        if self._flop_count is not None:
            self._flop_count[0] += n

    def _patch_dpt_upsampling(self):
        """The DPT neck / head between the library convolutions (transformers DepthAnythingReassembleStage / PreActResidualLayer / FeatureFusionLayer /
        DepthEstimationHead; the module graphs are otherwise reproduced verbatim): _ConvRouter (where each convolution runs, per mode), _FusionStage, the head (_DaHead,
        or DPT's in _patch_dpt_vit_reassemble_head) and the reassemble stage (_patch_da_reassemble, or DPT's).  The align_corners=True bilinear up-samplings run on
        vd3d_upsample_bilinear_nhwc.  Same function as the module graph up to float32 association (tests/test_hip_depth_e2e.py: 1e-4 of the range on the prediction,
        identical uint8 planes up to the stated bar).  VD3D_NECK_GLUE is read here, once: "0" is the A/B switch back to the module graph's own passes."""
        cr = _ConvRouter(self, self.dtype == torch.float32 and _switch("VD3D_NECK_GLUE"))
        if self.dpt_vit:
            _FusionStage(self, cr)
            return self._patch_dpt_vit_reassemble_head(cr)
        _FusionStage(self, cr, _DaHead(self, cr).upconv)
        self._patch_da_reassemble(cr)

    def _patch_da_reassemble(self, cr):
        """Depth-Anything's reassemble stage: the token tensor goes to the 1x1 projection as a channels_last VIEW ([B,T,C] minus CLS is NHWC storage) instead of a NCHW copy
        that MIOpen converts back; the up-scaling stages 0 / 1 hand their coarse map to neck.convs[i] where _PolyRoute runs.  self_contained=True: _self_contained_reassemble."""
        neck, stage = self.model.neck, self.model.neck.reassemble_stage
        if self.self_contained:
            stage.forward = self._self_contained_reassemble()
            return
        on = self.gemm == "f32" and cr.f32 and self.device.type == "cuda"
        poly = {i: _PolyRoute(cr, stage.layers[i].resize, neck.convs[i]) for i in (0, 1)
                if on and i < len(stage.layers) and i < len(neck.convs) and isinstance(stage.layers[i].resize, torch.nn.ConvTranspose2d)}

        def reassemble_fwd(hidden_states, patch_height=None, patch_width=None):
            out = []
            for route in poly.values():
                route.pending = None
            for i, hs in enumerate(hidden_states):
                B, _, Cn = hs.shape
                x = hs[:, 1:].reshape(B, patch_height, patch_width, Cn).permute(0, 3, 1, 2)   # NHWC storage, NCHW view: channels_last
                if i in poly:
                    poly[i].pending = poly[i].route(x)[0]
                    if poly[i].pending is not None:
                        out.append(stage.layers[i].projection(x))   # the coarse map; neck.convs[i] is the composed launch
                        continue
                out.append(stage.layers[i](x))
            return out
        stage.forward = reassemble_fwd

    def _self_contained_resize(self, rz, name):
        """The resize module ``rz`` (``name``) of a reassemble layer under self_contained=True -> (kind, operand): ("ct", _ConvTransposeGemm) for a ConvTranspose2d with a
        square kernel == stride, no padding and C_in % 16; ("s2", weight image) for a Conv2d 3 x 3 / stride 2 / padding 1 the stride-2 tile convolution of the mode
        builds (C_in % 16, C_out % 128 up to 1024); ("identity", None).  Anything else is refused by name.  One rule for the DINOv2 stage and DPT's."""
        R, gm = self.renderer, self.gemm
        if isinstance(rz, torch.nn.ConvTranspose2d):
            if not (rz.kernel_size == rz.stride and rz.kernel_size[0] == rz.kernel_size[1] and rz.padding == (0, 0) and rz.output_padding == (0, 0)
                    and rz.dilation == (1, 1) and rz.groups == 1 and rz.in_channels % 16 == 0 and rz.out_channels % 4 == 0):
                raise NotImplementedError(f"self_contained=True: {name}: a ConvTranspose2d with kernel {rz.kernel_size} / stride {rz.stride} / padding "
                                          f"{rz.padding}, {rz.in_channels} -> {rz.out_channels} channels (built: square kernel == stride, no padding, C_in % 16) -- not built")
            return "ct", _ConvTransposeGemm(R, rz, gm)
        if isinstance(rz, torch.nn.Conv2d):
            img = R.conv3x3_tile_pack(rz.weight, gm, 2) if _is_conv(rz, 3, 2, 1) else None
            if img is None:
                raise NotImplementedError(f"self_contained=True: {name}: a Conv2d with kernel {rz.kernel_size} / stride {rz.stride} / padding {rz.padding}, "
                                          f"{rz.in_channels} -> {rz.out_channels} channels (built: 3 x 3 / stride 2 / padding 1, C_in % 16, C_out % 128 up to 1024) -- not built")
            return "s2", img
        if not isinstance(rz, torch.nn.Identity):
            raise NotImplementedError(f"self_contained=True: {name} ({type(rz).__name__}) is no resize module the mode routes -- not built")
        return "identity", None

    def _self_contained_resize_run(self, kind, operand, rz, name, rows, B, gh, gw):
        """Run what ``_self_contained_resize`` prepared on the projected token rows [B, gh gw, C] (NHWC storage of the B x gh x gw map) -> the channels_last
        [B, C', h', w'] map, and record the route.  The caller counts the flops."""
        R, gm = self.renderer, self.gemm
        if kind == "ct":
            self.conv_routes[name] = (gm, "self-contained: vd3d_gemm_x3 + vd3d_depth_to_space_bias_nhwc_f32")
            return operand(rows, B, gh, gw)
        x = rows.view(B, gh, gw, rows.shape[-1]).permute(0, 3, 1, 2)
        if kind == "s2":
            x = R.conv3x3_tile(x, operand, rz.out_channels, gm, 2)
            if rz.bias is not None:
                x = R.bias_act(x, rz.bias)
            self.conv_routes[name] = (gm, "self-contained: vd3d_conv3x3_" + R.TILE_CONVS[gm, 2])
        return x

    def _self_contained_reassemble(self):
        """The DINOv2 reassemble stage without a library call (self_contained=True): per hook, the tokens minus CLS are the rows of the 1 x 1 projection (linear_x3
        with its bias; [B, T-1, C_i] is NHWC storage); ConvTranspose2d (kernel == stride, no padding) is a _ConvTransposeGemm, as on DPT-Large's route
        (_patch_dpt_vit_reassemble_head); Identity stays; the 3 x 3 / stride 2 / padding 1 convolution runs on the stride-2 tile convolution of the mode
        (vd3d_conv3x3_s2_x3 | vd3d_conv3x3_s2_x2) with its bias through bias_act.  Any other resize module is refused by name, here, at construction."""
        R, gm = self.renderer, self.gemm
        stage = self.model.neck.reassemble_stage
        hooks = []
        for lay in stage.layers:
            pm, rz = lay.projection, lay.resize
            if not _is_conv(pm, 1, 1, 0) or pm.in_channels % 16:
                raise NotImplementedError(f"self_contained=True: {self._names[id(pm)]} is not a 1 x 1 convolution with C_in a multiple of 16 -- not built")
            kind, img = self._self_contained_resize(rz, self._names[id(rz)])
            hooks.append(dict(pm=pm, rz=rz, proj=R.gemm_x3_pack(pm.weight.reshape(pm.out_channels, pm.in_channels), gm), kind=kind, img=img))

        def reassemble_fwd(hidden_states, patch_height=None, patch_width=None):
            out = []
            for hk, hs in zip(hooks, hidden_states):
                B, T, _ = hs.shape
                if patch_height is None or patch_width is None:
                    raise ValueError("the DINOv2 reassemble stage needs the patch grid")
                gh, gw = int(patch_height), int(patch_width)
                if gh * gw != T - 1:
                    raise ValueError(f"{T - 1} patch tokens do not form a {gh} x {gw} grid")
                pm, rz = hk["pm"], hk["rz"]
                n = pm.out_channels
                x = R.linear_x3(hs[:, 1:].contiguous(), hk["proj"], n, pm.bias, mode=gm)         # [B, T-1, C_i]: NHWC storage
                self.conv_routes[self._names[id(pm)]] = (gm, "self-contained: vd3d_gemm_x3 over the token rows")
                self._count_conv(pm, x.view(B, gh, gw, n).permute(0, 3, 1, 2))   # the routed modules bypass the counting hooks: the figure equals the library mode's
                x = self._self_contained_resize_run(hk["kind"], hk["img"], rz, self._names[id(rz)], x, B, gh, gw)
                if hk["kind"] != "identity":
                    self._count_conv(rz, x)   # the hook's formula, as the library mode counts these modules
                out.append(x)
            return out
        return reassemble_fwd

    def _patch_patch_embedding(self, pe):
        """Self-contained: the patch-embedding module ``pe`` (Dinov2PatchEmbeddings, DPTViTPatchEmbeddings: ``projection`` = Conv2d(3, C, kernel_size=p, stride=p), whose
        map the module flattens and transposes) as vd3d_patchify_f32 + vd3d_gemm_x3 on the weight reshaped to [C, 3 p^2] and zero-padded to the GEMM's K unit
        (p = 14: 588 -> 592; p = 16: 768, no padding), with its bias: [B, T-1, C] directly.  CLS, the cached position embedding and the final LayerNorm stay ATen
        element-wise / native kernels."""
        m = pe.projection
        name = self._names[id(m)]
        if not patch_embedding_conv_ok(m):
            raise NotImplementedError(f"self_contained=True: {name}: a patch embedding other than Conv2d(3, C, kernel_size=p, stride=p), p <= 64 -- not built")
        rows = patch_embedding_rows(self.renderer, m, self.gemm)

        def patch_fwd(pixel_values):
            if pixel_values.dtype != torch.float32 or pixel_values.shape[1] != 3:
                raise NotImplementedError("self_contained=True: the patch embedding takes a float32 [B, 3, th, tw] image")
            y = rows(pixel_values.contiguous(memory_format=torch.channels_last))   # what depth_preprocess hands over is taken as it is
            self.conv_routes[name] = (self.gemm, "self-contained: vd3d_patchify_f32 + vd3d_gemm_x3")
            self._count_conv(m, y)   # the bypassed Conv2d: 2 (T - 1) C 3 p^2
            return y
        pe.forward = patch_fwd

    def _patch_dpt_vit_reassemble_head(self, cr):
        """DPT-Large's reassemble stage and head on the library path (split modes; called by _patch_dpt_upsampling, whose fusion-stage rewrite DPT shares):
          * per hook, GELU(Linear_2C->C(cat(tokens, CLS))) as one linear_x3 with the GELU epilogue over the [B, T-1, 2C] rows, then the 1x1 projection
            (C -> C_i) as a linear_x3 with its bias on the same rows -- [B, T-1, C_i] is NHWC storage, handed on as a channels_last view;
          * resize: hooks 0 / 1 (ConvTranspose2d, kernel == stride s) as a linear_x3 with the weight permuted to [(i, j, co)][ci] + the scatter / bias
            launch vd3d_depth_to_space_bias_nhwc_f32; hook 2 identity; hook 3 (3 x 3 stride 2) the library convolution -- under self_contained=True the
            stride-2 tile convolution of the mode + bias_act, by the rule of _self_contained_resize, and every module's route goes into conv_routes;
          * head: _ConvRouter.head_tail3 with scale 1 and the head's nn.Upsample(x 2) size (conv2 on vd3d_conv3x3_x2 in fp16x2 where its size rule allows).
        neck.convs (3 x 3, no bias, C_i -> 256) and the fusion stage's 256 -> 256 convolutions have 256 output channels, which vd3d_conv3x3_x2 does not
        build: they stay library float32 convolutions, as for DA-V2-Large -- unless the pipe was built with conv="bf16x3", whose vd3d_conv3x3_x3 builds
        256 output channels and takes them and the head's two 3 x 3 convolutions (the _ConvRouter ``cr``: conv_nb / its neck.convs routing)."""
        R, gm, sc = self.renderer, self.gemm, self.self_contained
        stage, head = self.model.neck.reassemble_stage, self.model.head
        hooks = []
        for i, lay in enumerate(stage.layers):
            if i in stage.neck_ignore_stages:   # DPT-Hybrid's hooks 0 / 1: maps of the BiT prefix, handed to neck.convs as they are
                hooks.append(None)
                continue
            rl, ract = stage.readout_projects[i][0], stage.readout_projects[i][1]
            gelu = isinstance(ract, torch.nn.GELU) and getattr(ract, "approximate", "none") == "none" or type(ract).__name__ == "GELUActivation"
            pw = lay.projection.weight
            hk = dict(readout=(R.gemm_x3_pack(rl.weight, gm), rl.out_features, rl.bias, gelu, ract),
                      proj=(R.gemm_x3_pack(pw.reshape(pw.shape[0], -1), gm), pw.shape[0], lay.projection.bias), resize=lay.resize,
                      ct=_ConvTransposeGemm(R, lay.resize, gm) if isinstance(lay.resize, torch.nn.ConvTranspose2d) and not sc else None)
            if sc:   # no library call: the resize module by the rule of the DINOv2 stage (refused by name here, at construction, if it is not built)
                hk["sc"], hk["pname"] = self._self_contained_resize(lay.resize, self._names[id(lay.resize)]), self._names[id(lay.projection)]
            hooks.append(hk)

        def count_rows(t, n):   # flops_per_frame: the 1x1 projections and transposed convolutions (EXECUTED: P x C_out x C_in) bypass the module hooks;
            self._count_flops(2.0 * t.numel() / t.shape[0] * n)   # the readout Linear is not a convolution (not counted, as in the stock graph)

        def reassemble_fwd(hidden_states, patch_height=None, patch_width=None):
            out = []
            for hk, hs in zip(hooks, hidden_states):
                if hk is None:
                    out.append(hs)
                    continue
                B, T, d = hs.shape
                if patch_height is None or patch_width is None:   # the stock stage's square grid
                    patch_height = patch_width = int((T - 1) ** 0.5)
                gh, gw = int(patch_height), int(patch_width)
                if gh * gw != T - 1:
                    raise ValueError(f"{T - 1} patch tokens do not form a {gh} x {gw} grid")
                img, n, bias, gelu, act = hk["readout"]
                x = torch.cat((hs[:, 1:], hs[:, :1].expand(B, T - 1, d)), -1)
                x = R.linear_x3(x, img, n, bias, gelu=True, mode=gm) if gelu else act(R.linear_x3(x, img, n, bias, mode=gm))
                img, n, bias = hk["proj"]
                count_rows(x, n)
                x = R.linear_x3(x, img, n, bias, mode=gm)                                                       # [B, T-1, C_i]
                if sc:
                    kind, operand = hk["sc"]
                    rz = hk["resize"]
                    self.conv_routes[hk["pname"]] = (gm, "self-contained: vd3d_gemm_x3 over the token rows")
                    if kind == "ct":
                        count_rows(x, operand.n)
                    x = self._self_contained_resize_run(kind, operand, rz, self._names[id(rz)], x, B, gh, gw)
                    if kind == "s2":
                        self._count_conv(rz, x)   # what the module's hook adds without the keyword
                elif hk["ct"] is not None:
                    count_rows(x, hk["ct"].n)
                    x = hk["ct"](x, B, gh, gw)
                else:
                    x = x.view(B, gh, gw, n).permute(0, 3, 1, 2)   # NHWC storage, NCHW view: channels_last
                    x = hk["resize"](x)                             # identity, or the library's 3 x 3 stride-2 convolution
                out.append(x)
            return out
        stage.forward = reassemble_fwd

        if not cr.f32:   # VD3D_NECK_GLUE=0: the head's own module graph
            return
        conv1, _, conv2, _, conv3, _ = list(head.head)
        tail_operands = _head_tail_operands(conv3)
        in_index = self.model.config.head_in_index

        def head_fwd(hidden_states):
            x = hidden_states[in_index].contiguous(memory_format=_CL)
            size = (2 * x.shape[2], 2 * x.shape[3])   # nn.Upsample(scale_factor=2, align_corners=True)
            return cr.head_tail3(cr.conv_nb(conv1, x), conv1, conv2, size, tail_operands, 1.0)
        head.forward = head_fwd

    @torch.no_grad()
    def _fuse_backbone_layers(self):
        """Inference-only rewrite of every Dinov2Layer (same math, fewer launches): q/k/v projections as ONE GEMM
        (N = 3*hidden), LayerScale folded into the output-projection / fc2 weights (lambda * (xW^T + b) == x(lambda*W)^T +
        lambda*b), the attention called directly (float32 with a renderer: vd3d_attention_f32; otherwise SDPA).  Per layer: 4 GEMMs + attention + 2 LN + GELU + 2 adds instead of 6 GEMMs + 13
        smaller kernels.  The block itself is ``vit_blocks``: ``dinov2_operands`` per layer, ``encoder_blocks`` in the pipe's ``gemm``."""
        bb = self.model.backbone
        # query padding is the library back-end's: the split modes are float32 only (the constructor refuses anything else) and the hook pads bf16 alone
        pad_state = query_padding(bb.embeddings, bb.layernorm) if self.device.type == "cuda" and self.gemm == "f32" else None
        layers = list(bb.encoder.layer)
        for layer, blk in zip(layers, encoder_blocks(self.renderer, [dinov2_operands(lay) for lay in layers], self.gemm, pad_state=pad_state)):
            layer.forward = blk

    def _depth_pro_encoders_scope(self, mode, processor):
        """``encoders=``: what the routing needs of the model and its processor, read from the module graph and the configuration only (nothing is moved or
        launched); everything it does not cover is refused by name.  Returns the plan ``_route_depth_pro_encoders`` executes: the processor side, DepthPro's patch
        size, the pyramid levels and the names of the encoders present."""
        from . import depth_pro
        m, tag = self.model, f"encoders={mode!r}"
        what = f"{self.name!r} ({type(m).__name__})"
        if type(m).__name__ != "DepthProForDepthEstimation":
            raise NotImplementedError(f"{tag}: {what} -- the keyword routes the three ViT encoders of DepthProForDepthEstimation; every other model takes gemm= / conv= / "
                                      "self_contained=")
        cfg = m.config
        found = [("patch", m.depth_pro.encoder.patch_encoder), ("image", m.depth_pro.encoder.image_encoder)]
        if m.fov_model is not None:
            found.append(("fov", m.fov_model.fov_encoder))
        for which, enc in found:
            vit = enc.model
            if type(vit).__name__ != "Dinov2Model":
                raise NotImplementedError(f"{tag}: {what}: the {which} encoder is a {type(vit).__name__} -- _split_block is built for Dinov2Model encoders")
            d, nh = int(vit.config.hidden_size), int(vit.config.num_attention_heads)
            if not head_geometry_ok(d, nh):
                raise NotImplementedError(f"{tag}: {what}: the {which} encoder has hidden size {d} with {nh} heads -- vd3d_attention_x3 and vd3d_add_layernorm are "
                                          "built for 384 / 768 / 1024 with 64-wide heads")
            if getattr(vit.config, "use_swiglu_ffn", False):
                raise NotImplementedError(f"{tag}: {what}: the {which} encoder has a SwiGLU feed-forward -- _split_block is built for fc1 / activation / fc2")
            if not patch_embedding_conv_ok(vit.embeddings.patch_embeddings.projection):
                raise NotImplementedError(f"{tag}: {what}: the {which} encoder's patch embedding is not Conv2d(3, C, kernel_size=p, stride=p), p <= 64 -- "
                                          "vd3d_patchify_f32 does not take it")
        ratios = [float(r) for r in cfg.scaled_images_ratios]
        if ratios != [0.25, 0.5, 1.0]:
            raise NotImplementedError(f"{tag}: {what}: scaled_images_ratios={list(cfg.scaled_images_ratios)} -- vd3d_depthpro_patches_f32 builds the pyramid of [0.25, 0.5, 1]")
        size = tuple(int(v) for v in (PROCESSORS["depth_pro"] if processor is None else processor)["size"])
        if size[0] != size[1] or size[0] % 4:
            raise NotImplementedError(f"{tag}: {what}: a processor size of {size} -- the pyramid kernel takes a square side that is a multiple of 4")
        p = int(cfg.patch_size)
        try:
            levels = depth_pro.pyramid_levels(size[0], p, ratios, [float(o) for o in cfg.scaled_images_overlap_ratios])
        except ValueError as e:
            raise NotImplementedError(f"{tag}: {what}: a pyramid vd3d_depthpro_patches_f32 is not built for -- {e}") from None
        if any(stride < 1 for _, _, stride, _ in levels):
            raise NotImplementedError(f"{tag}: {what}: a pyramid vd3d_depthpro_patches_f32 is not built for -- scaled_images_overlap_ratios="
                                      f"{list(cfg.scaled_images_overlap_ratios)} leave a stride below 1")
        return dict(size=size[0], patch=p, ratios=ratios, overlaps=[float(o) for o in cfg.scaled_images_overlap_ratios], which=[w for w, _ in found])

    @torch.no_grad()
    def _route_depth_pro_encoders(self, mode, plan):
        """``encoders=``: the forwards of DepthProPatchEncoder, DepthProImageEncoder and DepthProFovEncoder replaced (``_depth_pro_encoders_scope`` has accepted the
        model), so that between ``pixel_values`` and the inputs of DepthProNeck / ``fov_model.conv`` every launch is one of this project's kernels or an ATen
        element-wise one (the class-token concatenation, the position-embedding add, the last block's residual add) -- no hipBLASLt, MIOpen or AOTriton call:
          * the patch pyramid: one launch of vd3d_depthpro_patches_f32, written in the memory patchify reads;
          * per encoder: vd3d_patchify_f32 + vd3d_gemm_x3 for the patch embedding, the class token and the (memoised) position embedding added, every Dinov2Layer a
            _split_block in ``mode`` (vit_blocks.encoder_blocks: one weight split / pack per encoder, here), the hook layers' residual streams kept, the final LayerNorm as
            add_layernorm(x, None, ln);
          * every reconstruct_feature_maps: vd3d_depthpro_merge_f32, handed on as the [B, C, oh, ow] view of its NHWC storage (channels_last, what the library
            convolutions behind it read);
          * the field-of-view encoder's ``neck`` Linear: vd3d_gemm_x3.
        Where floor(S / 4) is DepthPro's patch size and the image / field-of-view encoder's image_size, that encoder reads the pyramid's quarter level (the last
        patch of the stack: F.interpolate(size=) and F.interpolate(scale_factor=0.25) give the same bits there); otherwise its resize stays an ATen call.
        ``encoders_resize`` says which, per encoder."""
        import math
        from transformers.models.depth_pro.modeling_depth_pro import DepthProOutput
        from . import depth_pro
        R, m = self.renderer, self.model
        cfg = m.config
        p, ratios, overlaps = plan["patch"], plan["ratios"], plan["overlaps"]
        state = {"pixel_values": None, "quarter": None}   # the pyramid's quarter level of the forward in flight, for the image / field-of-view encoders

        def make_encoder(vit):
            emb = vit.embeddings
            rows = patch_embedding_rows(R, emb.patch_embeddings.projection, mode)
            blocks = encoder_blocks(R, [dinov2_operands(lay) for lay in vit.encoder.layer], mode, keyword="encoders")
            pos = {}

            def run(x, hooks=()):
                """[N, 3, h, w] in channels_last memory -> (LayerNorm(last hidden state), {hook: that layer's residual stream})."""
                N, _, h, w = x.shape
                t = torch.cat((emb.cls_token.expand(N, -1, -1), rows(x)), dim=1)
                if (h, w) not in pos:   # a constant of the input size (the parameter itself where the grid is the trained one)
                    pos[(h, w)] = emb.interpolate_pos_encoding(t, h, w).detach()
                t = t + pos[(h, w)]
                kept = {}
                for li, blk in enumerate(blocks):
                    t = blk(t)
                    if li in hooks:
                        kept[li] = t
                return R.add_layernorm(t, None, vit.layernorm)[1], kept
            return run

        def base_size(enc, height, width):   # the lowest-resolution feature size, as the stock forwards compute it
            e = int(math.log2(width / enc.out_size))
            return height // 2 ** e, width // 2 ** e

        def merge(rows, B, padding, oh, ow):
            T = rows.shape[1]
            return R.depthpro_merge(rows.contiguous(), B, int(T ** 0.5), padding, oh, ow).permute(0, 3, 1, 2)

        def own_input(which, enc_cfg, pixel_values):
            """The [B, 3, size, size] input of the image / field-of-view encoder in channels_last memory."""
            size = int(enc_cfg.image_size)
            q = state["quarter"] if state["pixel_values"] is pixel_values else None
            if q is not None and pixel_values.shape[-1] // 4 == size == p and tuple(q.shape[-2:]) == (size, size):
                self.encoders_resize[which] = "pyramid"
                return q
            self.encoders_resize[which] = "aten"
            return F.interpolate(pixel_values, size=(size, size), mode="bilinear", align_corners=False).contiguous(memory_format=torch.channels_last)

        def check(pixel_values):
            if pixel_values.dtype != torch.float32 or pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
                raise NotImplementedError(f"encoders={mode!r}: float32 [B, 3, S, S] pixel values expected -- refusing to fall back silently")

        pe_mod = m.depth_pro.encoder.patch_encoder
        run_patch = make_encoder(pe_mod.model)
        hook_ids = [int(i) for i in pe_mod.intermediate_hook_ids]

        def patch_fwd(pixel_values):
            check(pixel_values)
            B, _, H, W = pixel_values.shape
            if H != W or H % 4:
                raise NotImplementedError(f"encoders={mode!r}: a {H} x {W} input -- the pyramid kernel takes a square side that is a multiple of 4")
            lv = depth_pro.pyramid_levels(H, p, ratios, overlaps)   # low resolution first
            patches = R.depthpro_patches(pixel_values.contiguous(), p, [lv[2][2], lv[1][2], lv[0][2]])
            state["pixel_values"], state["quarter"] = pixel_values, (patches[-B:] if lv[0][3] == 1 else None)
            last, kept = run_patch(patches, set(hook_ids))
            bh, bw = base_size(pe_mod, H, W)
            feats, start = [None] * 3, 0
            for i in (2, 1, 0):   # the stack holds the high-resolution patches first, the features are listed low resolution first
                cnt = lv[i][3] ** 2 * B
                feats[i] = merge(last[start:start + cnt], B, int(pe_mod.merge_padding_value * (1 / ratios[i])), bh * 2 ** i, bw * 2 ** i)
                start += cnt
            for i in hook_ids:
                feats.append(merge(kept[i], B, int(pe_mod.merge_padding_value * (1 / ratios[-1])), bh * 4, bw * 4))
            return feats
        pe_mod.forward = patch_fwd

        ie_mod = m.depth_pro.encoder.image_encoder
        run_image = make_encoder(ie_mod.model)

        def image_fwd(pixel_values, output_attentions=False, output_hidden_states=False, return_dict=True):
            check(pixel_values)
            if output_attentions or output_hidden_states:
                raise NotImplementedError(f"encoders={mode!r}: the routed image encoder keeps no attentions or hidden states")
            B, _, H, W = pixel_values.shape
            last, _ = run_image(own_input("image", cfg.image_model_config, pixel_values))
            feats = merge(last, B, 0, *base_size(ie_mod, H, W))
            return DepthProOutput(last_hidden_state=last, features=feats) if return_dict else (last, feats)
        ie_mod.forward = image_fwd

        if m.fov_model is not None:
            fe_mod = m.fov_model.fov_encoder
            run_fov = make_encoder(fe_mod.model)
            neck = fe_mod.neck
            neck_img = R.gemm_x3_pack(neck.weight, mode)

            def fov_fwd(pixel_values):
                check(pixel_values)
                B, _, H, W = pixel_values.shape
                last, _ = run_fov(own_input("fov", cfg.fov_model_config, pixel_values))
                state["pixel_values"] = state["quarter"] = None   # the last reader of the forward in flight
                return merge(R.linear_x3(last, neck_img, neck.out_features, neck.bias, mode=mode), B, 0, *base_size(fe_mod, H, W))
            fe_mod.forward = fov_fwd
        self.encoders = mode

    def _split_scope(self, fuse_backbone: bool = True) -> str:
        """Which rewrite ``gemm="bf16x3" / "fp16x2"`` applies to this model: "dinov2" (DepthAnythingForDepthEstimation on Dinov2Backbone), "dpt-vit"
        (DPTForDepthEstimation on its plain ViT encoder with readout_type="project": DPT-Large) or "dpt-hybrid" (DPTForDepthEstimation with is_hybrid in the
        published Intel/dpt-hybrid-midas geometry: four hooks, neck_ignore_stages [0, 1], readout_type="project", a BiT bottleneck backbone of three stages and 32
        groups; any other hybrid is refused as "DPT-Hybrid ...").  Everything else raises NotImplementedError naming the model.
        ``self_contained=True`` covers exactly the models of the split modes, so the constructor asks here too; the refusal then names the keyword.  Reads the
        module graph and its configuration only."""
        m, what = self.model, f"{self.name!r} ({type(self.model).__name__}"
        bb = getattr(m, "backbone", None)
        what += f" on {type(bb).__name__})" if self.arch == "da" and bb is not None else ")"
        tag = "self_contained=True" if self.self_contained else f"gemm={self.gemm!r}"
        if self.arch == "da" and type(m.backbone).__name__ == "Dinov2Backbone" and fuse_backbone:
            return "dinov2"
        if type(m).__name__ == "DepthProForDepthEstimation":
            raise NotImplementedError(f"{tag}: {what} -- DepthPro runs its stock float32 graph between the own front end and post-process (gemm='f32'); the split-mode "
                                      "rewrite of its three encoders, neck, fusion stage, head and field-of-view branch is not built -- nothing is substituted "
                                      "silently")
        if type(m).__name__ != "DPTForDepthEstimation" or not fuse_backbone:
            raise NotImplementedError(f"{tag}: {what} -- the split modes rewrite the fused DINOv2 backbone (Depth-Anything V1 / V2, Distill-Any-Depth) and the "
                                      "plain-ViT DPT (DPT-Large), with fuse_backbone=True; this model runs its stock float32 graph -- nothing is substituted silently")
        cfg = m.config

        def refuse(why):
            raise NotImplementedError(f"{tag}: {what}: {why} -- not built in the split modes; gemm='f32' runs the stock float32 graph")
        hybrid = bool(cfg.is_hybrid)
        if hybrid:   # exactly the geometry _rewrite_dpt_hybrid builds: the published Intel/dpt-hybrid-midas one, at the hidden sizes the kernels have
            bc = cfg.backbone_config
            bit = bc is not None and getattr(bc, "model_type", None) == "bit"
            why = (f"{len(cfg.backbone_out_indices)} hooks / {len(cfg.neck_hidden_sizes)} neck stages" if len(cfg.backbone_out_indices) != 4 or len(cfg.neck_hidden_sizes) != 4
                   else f"neck_ignore_stages={cfg.neck_ignore_stages}" if list(cfg.neck_ignore_stages or []) != [0, 1]
                   else f"readout_type={cfg.readout_type!r}" if cfg.readout_type != "project"
                   else "no BiT backbone" if not bit
                   else f"a BiT backbone of layer_type={bc.layer_type!r}" if bc.layer_type != "bottleneck"
                   else f"a BiT backbone with {len(bc.depths)} stages" if len(bc.depths) != 3
                   else f"a BiT backbone with {bc.num_groups} groups" if int(bc.num_groups) != 32 else None)
            if why is not None:
                refuse(f"DPT-Hybrid (MiDaS 3.0 hybrid, Intel/dpt-hybrid-midas) with {why} (built: four hooks, neck_ignore_stages [0, 1], readout_type 'project', a BiT "
                       "bottleneck backbone of three stages and 32 groups; the BiT stem feeds hooks 0 / 1 through an identity readout)")
        else:
            if getattr(m, "backbone", None) is not None or cfg.backbone_config is not None:
                bname = type(m.backbone).__name__ if getattr(m, "backbone", None) is not None else cfg.backbone_config.model_type
                refuse(f"a {bname} backbone (e.g. Intel/dpt-beit-large-512: BEiT's relative position bias has no input in vd3d_attention_x3)")
            if cfg.readout_type != "project":
                refuse(f"readout_type={cfg.readout_type!r} (only 'project' is built)")
            if list(cfg.neck_ignore_stages or []):
                refuse(f"neck_ignore_stages={cfg.neck_ignore_stages}")
        if m.head.projection is not None:
            refuse("a head projection (add_projection=True)")
        if cfg.use_batch_norm_in_fusion_residual:
            refuse("batch norm in the fusion residual units")
        d, nh = int(cfg.hidden_size), int(cfg.num_attention_heads)
        if not head_geometry_ok(d, nh):
            refuse(f"hidden size {d} with {nh} heads (built: 384 / 768 / 1024, 64-wide heads)")
        for lay in m.neck.reassemble_stage.layers:
            r = getattr(lay, "resize", None)   # (DPT-Hybrid's hooks 0 / 1 are nn.Identity layers)
            if isinstance(r, torch.nn.ConvTranspose2d) and not (r.kernel_size == r.stride and r.padding == (0, 0) and r.output_padding == (0, 0)
                                                                 and r.dilation == (1, 1) and r.groups == 1):
                refuse(f"a reassemble ConvTranspose2d with kernel {r.kernel_size} / stride {r.stride} / padding {r.padding} (built: kernel == stride, no padding)")
        hs = list(m.head.head)
        if not (len(hs) == 6 and isinstance(hs[1], torch.nn.Upsample) and isinstance(hs[3], torch.nn.ReLU) and isinstance(hs[5], torch.nn.ReLU)
                and hs[4].kernel_size == (1, 1) and hs[2].out_channels in (16, 32, 64) and hs[1].scale_factor in (2, 2.0) and hs[1].align_corners):
            refuse("a depth head other than DPT's [conv, Upsample x2, conv -> 16 / 32 / 64, ReLU, conv 1x1, ReLU]")
        return "dpt-hybrid" if hybrid else "dpt-vit"

    def _rewrite_dpt_vit(self):
        """The split-mode rewrite of a plain-ViT DPTForDepthEstimation (DPT-Large; _split_scope has accepted it): position embeddings memoised, the ViT
        layers on the split kernels, the reassemble stage, neck and head on the library path (_patch_dpt_upsampling)."""
        self.dpt_vit = True
        self._cache_vit_position_embeddings()
        self._fuse_vit_layers()
        self._patch_dpt_upsampling()

    def _patch_hybrid_embeddings(self):
        """DPT-Hybrid's embeddings (DPTViTHybridEmbeddings; _split_scope has accepted the model) in the split modes: the 1 x 1 projection of the BiT stage-3 map
        (1024 -> hidden) as vd3d_gemm_x3 over its pixel rows, with its bias -- [B, gh gw, hidden] directly, no flatten / transpose copy; CLS and the memoised
        position embedding stay ATen element-wise kernels.  The BiT prefix in front of it: without ``self_contained`` the module graph on the float32 library
        (conv_routes says so for every convolution and normalisation of it, by module name); with it _BitPrefix, on own kernels.  The stage-1 / stage-2 maps go
        on as channels_last [B, C, h, w] tensors: hooks 0 / 1 of the reassemble stage."""
        from transformers.models.dpt.modeling_dpt import BaseModelOutputWithIntermediateActivations as Out
        R, gm, sc = self.renderer, self.gemm, self.self_contained
        emb = self.model.dpt.embeddings
        pm, bb = emb.projection, emb.backbone
        if not _is_conv(pm, 1, 1, 0) or pm.in_channels % 16:
            raise NotImplementedError(f"gemm={gm!r}: {self._names[id(pm)]} is not a 1 x 1 convolution with C_in a multiple of 16 -- not built")
        img = R.gemm_x3_pack(pm.weight.reshape(pm.out_channels, pm.in_channels), gm)
        prefix = _BitPrefix(self, bb, bit_prefix_plan(bb, self._names), self._names) if sc else None
        lib_names = [self._names[id(m)] for m in bb.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.GroupNorm))]

        def emb_fwd(pixel_values, interpolate_pos_encoding=False):
            B, C, H, W = pixel_values.shape
            if C != emb.num_channels:
                raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the configuration.")
            if not interpolate_pos_encoding and (H != emb.image_size[0] or W != emb.image_size[1]):
                raise ValueError(f"Input image size ({H}*{W}) doesn't match model ({emb.image_size[0]}*{emb.image_size[1]}).")
            pos = emb._resize_pos_embed(emb.position_embeddings, H // emb.patch_size, W // emb.patch_size)
            if sc:
                f1, f2, f3 = prefix(pixel_values)
                hooks = [f1.permute(0, 3, 1, 2), f2.permute(0, 3, 1, 2)]
            else:
                maps = bb(pixel_values).feature_maps
                for n in lib_names:
                    self.conv_routes[n] = ("library", "the BiT prefix stays the module graph without self_contained=True")
                hooks, f3 = [maps[i] for i in emb.residual_feature_map_index], maps[-1].permute(0, 2, 3, 1).contiguous()
            tok = R.linear_x3(f3.reshape(B, f3.shape[1] * f3.shape[2], f3.shape[3]), img, pm.out_channels, pm.bias, mode=gm)
            self.conv_routes[self._names[id(pm)]] = (gm, ("self-contained: " if sc else "") + "vd3d_gemm_x3 over the pixel rows")
            self._count_conv(pm, tok)   # the bypassed Conv2d
            x = torch.cat((emb.cls_token.expand(B, -1, -1), tok), dim=1) + pos
            return Out(last_hidden_states=x, intermediate_activations=hooks)
        emb.forward = emb_fwd

    def _cache_vit_position_embeddings(self):
        """DPTViTEmbeddings re-interpolates its position embedding (bilinear, 24 x 24 -> patch grid) on every forward; for a fixed input size the result is a
        constant.  Memoised per (grid height, grid width, dtype), like _cache_position_embeddings for DINOv2."""
        _memoise(self.model.dpt.embeddings, "_resize_pos_embed", lambda t, gh, gw, start_index=1: (int(gh), int(gw), t.dtype, int(start_index)))

    @torch.no_grad()
    def _fuse_vit_layers(self):
        """Every DPTViTLayer (ViT-L/16 of DPT-Large) as a ``vit_blocks._split_block`` -- the same rewrite as _fuse_backbone_layers' split mode, on
        ``dpt_vit_operands``.  The encoder collects each layer's return value at backbone_out_indices: the residual stream, as in the stock graph."""
        layers = list(self.model.dpt.encoder.layer)
        for layer, blk in zip(layers, encoder_blocks(self.renderer, [dpt_vit_operands(lay) for lay in layers], self.gemm)):
            layer.forward = blk

    def _pil_pixel_values(self, frames_bgr: torch.Tensor, inference_size=None) -> torch.Tensor:
        """``front_end="pil"``: the pixel_values the reference's image processor makes of these frames as PIL images (pre-resized to
        ``inference_size`` = (W', H') when given), [B,3,th,tw] of ``self.dtype``, channels_last on the GPU."""
        if frames_bgr.dtype != torch.uint8 or frames_bgr.dim() != 4 or frames_bgr.shape[-1] != 3:
            raise TypeError("front_end='pil' takes uint8 [B,H,W,3] BGR frames (the reference's 8-bit images)")
        H, W = frames_bgr.shape[1:3]
        sh, sw = (H, W) if inference_size is None else (int(inference_size[1]), int(inference_size[0]))
        th, tw = self.resize_target(sh, sw)
        if self.renderer is not None:
            x = self.renderer.depth_preprocess_pil(frames_bgr, th, tw, self.proc["mean"], self.proc["std"], dtype=self.dtype, inference_size=inference_size)
            self.front_end_route = self.renderer.pil_route
            return x
        from . import pil_resample
        x = pil_resample.pixel_values(frames_bgr.to(self.device), th, tw, self.proc["mean"], self.proc["std"], self.dtype, inference_size).permute(0, 3, 1, 2)
        self.front_end_route = "statement"
        return x if self.device.type == "cuda" else x.contiguous()

    @torch.no_grad()
    def infer_bgr_u8(self, frames_bgr: torch.Tensor, inference_size=None, raw: bool = False, at_inference_size: bool = False) -> torch.Tensor:
        """uint8 [B,H,W,3] BGR frames in HBM -> float32 [B,H,W] predicted depth at the frame size (the
        depth-estimation pipeline's post-process: bicubic, align_corners=False).  ``raw=True`` returns the model-resolution
        prediction [B,th,tw] instead, for the fused HIP hand-off (Renderer.depth_handoff).  ``at_inference_size``: with an
        ``inference_size`` (W', H') the prediction is returned at (H', W') -- what the transformers pipeline hands back for the
        pre-resized images of hf_batch_safe_pipe (core/render_depth.py:1113-1116)."""
        B, H, W, _ = frames_bgr.shape
        if at_inference_size and inference_size is not None:
            oH, oW = int(inference_size[1]), int(inference_size[0])
        else:
            oH, oW = H, W
        if self.arch == "depth_pro":
            return self._infer_depth_pro(frames_bgr, inference_size, raw, oH, oW)
        if self.front_end == "pil":
            pred = self.model(pixel_values=self._pil_pixel_values(frames_bgr, inference_size)).predicted_depth
            if raw:
                return pred.float()
            return F.interpolate(pred.float().unsqueeze(1), size=(oH, oW), mode="bicubic", align_corners=False).squeeze(1)
        if self.renderer is not None and inference_size is None and frames_bgr.dtype == torch.uint8:
            th, tw = self.resize_target(H, W)
            x = None
            try:
                x = self.renderer.depth_preprocess(frames_bgr, th, tw, self.proc["mean"], self.proc["std"], dtype=self.dtype)
            except Exception as e:   # down-scale beyond the kernel's tap budget: the ATen path below is the same math
                if getattr(e, "code", None) != -4:
                    raise
            if x is not None:
                pred = self.model(pixel_values=x).predicted_depth
                if raw:
                    return pred.float()
                return F.interpolate(pred.float().unsqueeze(1), size=(H, W), mode="bicubic", align_corners=False).squeeze(1)
        x = frames_bgr.to(self.device).flip(-1).permute(0, 3, 1, 2).float()  # RGB, NCHW
        if inference_size is not None:  # hf_batch_safe_pipe: img.resize(inference_size, BICUBIC) first (:1113-1116)
            x = F.interpolate(x, size=(int(inference_size[1]), int(inference_size[0])), mode="bicubic", antialias=True,
                              align_corners=False).clamp_(0, 255)
        th, tw = self.resize_target(x.shape[2], x.shape[3])
        x = F.interpolate(x, size=(th, tw), mode="bicubic", antialias=True, align_corners=False)
        x = ((x / 255.0) - self.mean) / self.std
        x = x.to(self.dtype)
        if self.device.type == "cuda":
            x = x.contiguous(memory_format=torch.channels_last)
        pred = self.model(pixel_values=x).predicted_depth  # [B, th, tw]
        if raw:
            return pred.float()
        pred = F.interpolate(pred.float().unsqueeze(1), size=(oH, oW), mode="bicubic", align_corners=False).squeeze(1)
        return pred

    def _infer_depth_pro(self, frames_bgr, inference_size, raw, oH, oW):
        """infer_bgr_u8 for DepthProForDepthEstimation: the processor (rescale + normalise, THEN the bilinear resize without antialias to 1536 x 1536), the model,
        and DepthProImageProcessor.post_process_depth_estimation at the size the pipeline saw -- depth * width / focal from the model's field of view (when it has
        that branch), bilinear resize, 1 / clamp(depth, 1e-4, 1e4).  With a renderer the post-process is one launch (vd3d_depthpro_post_f32; the field of
        view stays on the device) and, for uint8 frames without an inference size, so is the front end (vd3d_depthpro_preprocess_u8).  With an ``inference_size`` (the
        pre-resize hands the processor non-integer pixels) or non-uint8 frames the front end is depth_pro.preprocess_statement, the same arithmetic as ATen operators on
        the device, and without a renderer so is the post-process (post_statement).  ``front_end_route`` ("kernel" | "statement") says which front end ran last.
        ``raw``: the model-resolution inverse depth, scaled for the model's own width and not resized (the pipeline resizes BEFORE the reciprocal)."""
        from . import depth_pro
        size = tuple(int(v) for v in self.proc["size"])
        if size[0] != size[1]:
            raise NotImplementedError(f"depth-pro: a processor size of {size} -- DepthPro takes square inputs")
        f = frames_bgr.to(self.device)
        if self.renderer is not None and inference_size is None and f.dtype == torch.uint8:
            x = self.renderer.depthpro_preprocess(f, size[0], self.proc["mean"], self.proc["std"])
            self.front_end_route = "kernel"
        else:
            self.front_end_route = "statement"
            if inference_size is not None:   # hf_batch_safe_pipe: img.resize(inference_size, BICUBIC) first (:1113-1116), in its float statement as for every model
                f = F.interpolate(f.flip(-1).permute(0, 3, 1, 2).float(), size=(int(inference_size[1]), int(inference_size[0])), mode="bicubic", antialias=True,
                                  align_corners=False).clamp_(0, 255).permute(0, 2, 3, 1).flip(-1)
            x = depth_pro.preprocess_statement(f, size, self.proc["mean"], self.proc["std"])
        out = self.model(pixel_values=x.to(self.dtype))
        pred = out.predicted_depth.float().contiguous()
        fov = None if out.field_of_view is None else out.field_of_view.float()
        if raw:
            oH = oW = pred.shape[-1]
        if self.renderer is not None:
            return self.renderer.depthpro_post(pred, fov, oH, oW)
        return depth_pro.post_statement(pred, fov, oH, oW, resize=not raw)

    @torch.no_grad()
    def depth_frames_u8(self, frames_bgr: torch.Tensor, inference_size=None, invert: bool = False, tiled: bool = False, tile: int = 512,
                        pad: int = 32, tile_batch: int = 16, bars=None) -> torch.Tensor:
        """The depth tab's per-frame product (core/render_depth.py:1907-1917) for uint8 [B,H,W,3] BGR frames: the prediction at the size
        the pipeline saw (the frame, or ``inference_size`` = (W', H')) -> ``convert_depth_to_grayscale`` -> optional ``255 -`` ->
        ``cv2.resize(..., (W, H), INTER_CUBIC)``.  Returns uint8 [B,H,W] on the device (what the reference writes to its depth video).
        ``tiled=True`` (OPT-IN, needs a renderer): the reference's USE_TILED_DEPTH product instead -- ``infer_tiled_bgr_u8`` (``tile`` /
        ``pad`` / ``tile_batch``) -> ``_normalize_to_u8``'s 1 % - 99 % percentile normalisation (:173-194, ``Renderer.depth_normalize_pclip``) -> the same
        INTER_CUBIC resize to the frame size.
        ``bars`` (``ignore_letterbox_bars``, :1919-1933; needs a renderer): a (top, bottom) pair or the int32 [B,2] device tensor
        ``letterbox.LetterboxTracker.update`` returns -- every plane is then squeezed into the picture rows and the bars are filled with the
        squeezed plane's median (``Renderer.depth_letterbox_fill``).  ``None``: the planes as they are."""
        u8 = self._depth_frames_u8(frames_bgr, inference_size, invert, tiled, tile, pad, tile_batch)
        if bars is None:
            return u8
        if self.renderer is None:
            raise RuntimeError("depth_frames_u8(bars=...) needs DepthPipe(renderer=...) for the letterbox fill")
        return self.renderer.depth_letterbox_fill(u8, bars)

    def _depth_frames_u8(self, frames_bgr, inference_size, invert, tiled, tile, pad, tile_batch):
        B, H, W, _ = frames_bgr.shape
        if tiled:
            d = self.infer_tiled_bgr_u8(frames_bgr, inference_size, tile=tile, pad=pad, tile_batch=tile_batch)
            u8 = self.renderer.depth_normalize_pclip(d, invert)
        else:
            u8 = depth_to_u8(self.infer_bgr_u8(frames_bgr, inference_size, at_inference_size=True), invert)
        if tuple(u8.shape[-2:]) == (H, W):
            return u8
        if self.renderer is None:
            raise RuntimeError("depth_frames_u8 with an inference size needs DepthPipe(renderer=...) for the uint8 INTER_CUBIC resize")
        out = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        for b in range(B):
            self.renderer.resize_cubic_u8(u8[b], H, W, out=out[b])
        return out

    def _frames_to_inference_size(self, frames: torch.Tensor, tgt_h: int, tgt_w: int) -> torch.Tensor:
        """infer_depth_tile's first step (core/render_depth.py:111-113): INTER_AREA when a side shrinks, INTER_CUBIC otherwise (a copy at
        equal size).  One side shrinking while the other grows is not built."""
        B, H, W, _ = frames.shape
        if (tgt_h, tgt_w) == (H, W):
            return frames
        shrink, grow = tgt_w < W or tgt_h < H, tgt_w > W or tgt_h > H
        if shrink and grow:
            raise NotImplementedError(f"tiled depth: inference size {tgt_w}x{tgt_h} shrinks one side of the {W}x{H} frame and grows the other "
                                      "(INTER_AREA with an up-scaled side) -- this mixed case is not built")
        R = self.renderer
        return torch.stack([R.resize_area_u8(frames[b], tgt_h, tgt_w) if shrink else R.resize_cubic_u8(frames[b], tgt_h, tgt_w) for b in range(B)])

    @torch.no_grad()
    def infer_tiled_bgr_u8(self, frames_bgr: torch.Tensor, inference_size=None, tile: int = 512, pad: int = 32, tile_batch: int = 16,
                           model_call=None) -> torch.Tensor:
        """The reference's tiler (infer_depth_tile, core/render_depth.py:102-170) for uint8 [B,H,W,3] BGR frames, on the device: frames to
        ``inference_size`` = (W', H') (default: the frame size) -> apron crops of every tile, resized to multiples of 14
        (``Renderer.tile_gather_cubic_u8``, one launch per crop shape across the B frames) -> the network on batches of at most
        ``tile_batch`` equal-shape tiles (``infer_bgr_u8(tiles, raw=True)``; the reference runs one tile per forward) -> Hann blend of the
        tile centres (``Renderer.tile_blend``, which also evaluates the pipeline's bicubic post-process of every tile).  Returns float32
        [B,H',W'].  The blend keeps the reference's quirks: pixels only one tile covers (first row / column) carry a degenerate weight and a huge
        value, which the percentile hand-off (``depth_frames_u8(tiled=True)``) clips.
        ``model_call``: a callable uint8 [n,chs,cws,3] BGR tiles -> float32 [n,ph,pw] predictions (one (ph, pw) per tile shape) that
        replaces the network."""
        if self.renderer is None:
            raise RuntimeError("infer_tiled_bgr_u8 needs DepthPipe(renderer=...): the tile gather and blend are HIP kernels")
        if self.arch == "depth_pro" and model_call is None:
            raise NotImplementedError(f"tiled depth: {self.name!r} (DepthProForDepthEstimation) -- the tile blend evaluates the pipeline's BICUBIC post-process of every tile; "
                                      "DepthPro's is a bilinear resize followed by a reciprocal -- not built")
        from .depth_tiles import tile_plan
        R = self.renderer
        f = frames_bgr.to(self.device)
        if f.dim() == 3:
            f = f[None]
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3:
            raise TypeError("infer_tiled_bgr_u8 takes uint8 [B,H,W,3] BGR frames")
        B, H, W, _ = f.shape
        tgt_w, tgt_h = (W, H) if inference_size is None else (int(inference_size[0]), int(inference_size[1]))
        img = self._frames_to_inference_size(f, tgt_h, tgt_w)
        plan = tile_plan(tgt_h, tgt_w, int(tile), int(pad), 14)
        cache = self.__dict__.setdefault("_tile_tables", {})
        key = (plan, B)
        if key not in cache:   # static per geometry: uploaded once
            cache[key] = dict(origins=[torch.from_numpy(plan.gather_origins(g, B)).to(self.device) for g in plan.groups],
                              w_pool=torch.from_numpy(plan.weight_pool()).to(self.device), blend={})
        tabs = cache[key]
        call = model_call if model_call is not None else (lambda t: self.infer_bgr_u8(t, raw=True))
        step = max(1, int(tile_batch))
        preds, shapes = [], []
        for g, org in zip(plan.groups, tabs["origins"]):
            tiles = R.tile_gather_cubic_u8(img, org, g.ch, g.cw, g.chs, g.cws)
            shape = None
            for i in range(0, tiles.shape[0], step):
                p = call(tiles[i:i + step])
                if not isinstance(p, torch.Tensor) or p.dim() != 3 or p.shape[0] != min(step, tiles.shape[0] - i) or (shape or tuple(p.shape[1:])) != tuple(p.shape[1:]):
                    raise ValueError("tiled depth: the model call returns a float32 [n,ph,pw] tensor, one (ph, pw) per tile shape")
                shape = tuple(p.shape[1:])
                preds.append(p.to(self.device, torch.float32).reshape(-1))
            shapes.append(shape)
        bkey = tuple(shapes)
        if bkey not in tabs["blend"]:
            tab, off, total = plan.blend_tables(B, shapes)
            tabs["blend"][bkey] = (torch.from_numpy(tab).to(self.device), torch.from_numpy(off).to(self.device), total)
        tab, off, total = tabs["blend"][bkey]
        pool = torch.cat(preds)
        assert pool.numel() == total
        return R.tile_blend(pool, off, tab, tabs["w_pool"], B, tgt_h, tgt_w, int(tile), int(pad))

    def call_tiled(self, images, inference_size=None, tile: int = 512, pad: int = 32):
        """The USE_TILED_DEPTH branch of _run_pipe_or_tile (core/render_depth.py:242-250) behind the reference protocol: list of PIL images (or
        HxWx3 uint8 RGB arrays) -> list of ``{"predicted_depth": float32 [H', W']}`` at the inference size (the frame size by default)."""
        single = not isinstance(images, (list, tuple))
        outs = []
        for im in ([images] if single else list(images)):
            a = np.asarray(im.convert("RGB") if hasattr(im, "convert") else im)
            bgr = torch.from_numpy(np.ascontiguousarray(a[..., ::-1]))[None]
            outs.append({"predicted_depth": self.infer_tiled_bgr_u8(bgr, inference_size, tile=tile, pad=pad)[0]})
        return outs

    def __call__(self, images, inference_size=None):
        """Reference protocol: list of PIL images (or HxWx3 uint8 RGB arrays) -> list of dicts; ``predicted_depth`` has the size
        of the image the pipeline saw (the frame, or ``inference_size`` when given -- the caller then resizes the uint8 map back
        with cv2.INTER_CUBIC, core/render_depth.py:1914-1917)."""
        single = not isinstance(images, (list, tuple))
        imgs = [images] if single else list(images)
        outs = []
        for im in imgs:
            a = np.asarray(im.convert("RGB") if hasattr(im, "convert") else im)
            bgr = torch.from_numpy(np.ascontiguousarray(a[..., ::-1]))[None]
            outs.append({"predicted_depth": self.infer_bgr_u8(bgr, inference_size, at_inference_size=True)[0]})
        return outs

    def flops_per_frame(self, h: int, w: int) -> float:
        """Dense-GEMM flop estimate for MFMA accounting: 2*params_linear*tokens + 4*T^2*d per layer
        for the backbone, the EXECUTED convolution flops of the DPT neck / head counted during one forward."""
        if self.arch == "depth_pro":
            raise NotImplementedError(f"flops_per_frame: {self.name!r} (DepthProForDepthEstimation) -- the estimate is not built for the three-encoder patch pyramid")
        th, tw = self.resize_target(h, w)
        bcfg = getattr(self.model.config, "backbone_config", None) or self.model.config
        if not hasattr(bcfg, "patch_size"):   # DPT-Hybrid: the backbone configuration is the BiT prefix's; the transformer is the model's own
            bcfg = self.model.config
        ps = int(bcfg.patch_size)
        T = (th // ps) * (tw // ps) + 1
        d, L = int(bcfg.hidden_size), int(bcfg.num_hidden_layers)
        lin = L * (4 * d * d + 8 * d * d)  # qkv+proj, mlp 4x
        backbone = 2.0 * lin * T + 4.0 * T * T * d * L
        total = [0.0]

        # the hook is registered on the convolution modules only; total is self._flop_count while they run
        hs = [m.register_forward_hook(lambda mod, inp, out: self._count_conv(mod, out)) for m in self.model.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
        self._flop_count = total   # the bias-free convolution calls of the rewritten neck / head count themselves (EXECUTED flops: the
        try:                       # fusion layers' projections run before their up-samplings, at a quarter of the pixels)
            with torch.no_grad():
                x = torch.zeros(1, 3, th, tw, device=self.device, dtype=self.dtype)
                if self.device.type == "cuda":
                    x = x.contiguous(memory_format=torch.channels_last)
                self.model(pixel_values=x)
        finally:
            self._flop_count = None
            for hnd in hs:
                hnd.remove()
        return backbone + total[0]
