"""DepthPro (``apple/DepthPro-hf``, ``DepthProForDepthEstimation``) behind DepthPipe: the published geometry; the image processor and its post-process stated
in torch (what the two kernels of csrc/vd3d_depthpro.hip are held to, and what runs where there is no renderer); and the model's patch order and merge geometry
stated in NumPy: ``patches_statement`` and ``merge_statement`` are what the two kernels of csrc/vd3d_depthpro_pyramid.hip (``vd3d_depthpro_patches_f32``,
``vd3d_depthpro_merge_f32``) give bit for bit (tests/test_hip_depth_pro_pyramid.py).  Those kernels run under ``DepthPipe(encoders="bf16x3" | "fp16x2")``, which
routes the three encoders (``DepthPipe._route_depth_pro_encoders``); by default the network is the stock module graph and no kernel runs them.

Line numbers are those of the installed transformers: ``models/depth_pro/modeling_depth_pro.py`` (M), ``models/depth_pro/image_processing_depth_pro.py`` (P)
and ``image_processing_backends.py`` (B).

The geometry below is the published one AS FAR AS IT IS KNOWN HERE: no copy of the checkpoint's config.json was at hand when this was written, so nothing has
confirmed it against the file.  A checkpoint loads with whatever geometry its own config.json states (``DepthPipe.from_pretrained``)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

# every encoder (image, patch, field of view): a Dinov2Model, ViT-L/16 at 384 x 384, no mask token
ENCODER = dict(model_type="dinov2", hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, image_size=384, patch_size=16, use_mask_token=False)
GEOMETRY = dict(patch_size=384, fusion_hidden_size=256, intermediate_hook_ids=[11, 5], intermediate_feature_dims=[256, 256],
                scaled_images_ratios=[0.25, 0.5, 1], scaled_images_overlap_ratios=[0.0, 0.5, 0.25], scaled_images_feature_dims=[1024, 1024, 512],
                merge_padding_value=3, use_fov_model=True, num_fov_head_layers=2)
# DepthProImageProcessor (P:46-53): 1536 x 1536, no aspect keeping, PIL resample 2 (bilinear), mean = std = 0.5; rescale + normalise BEFORE the resize (P:70-80)
PROCESSOR = dict(size=(1536, 1536), keep_aspect_ratio=False, multiple=1, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), resample=2)


def config(**over):
    """DepthProConfig of the published geometry (see the module docstring for what "published" means here); ``over`` replaces top-level fields."""
    from transformers import DepthProConfig
    kw = dict(GEOMETRY, image_model_config=dict(ENCODER), patch_model_config=dict(ENCODER), fov_model_config=dict(ENCODER))
    kw.update(over)
    return DepthProConfig(**kw)


# ---------------------------------------------------------------------------------------------------------------- the image processor
def normalize_table(mean, std) -> torch.Tensor:
    """The processor's fused rescale + normalise (B:297-337) as a table of the byte, float32 [3, 256] in R, G, B order: mean and std are multiplied by
    1 / rescale_factor = 1 / (1 / 255) as float32 tensors, then (float32(byte) - mean') / std' -- a subtraction and a division, each rounded once."""
    k = 1.0 / (1 / 255)
    m = torch.tensor(mean, dtype=torch.float32) * k
    s = torch.tensor(std, dtype=torch.float32) * k
    return (torch.arange(256, dtype=torch.float32)[None, :] - m[:, None]) / s[:, None]


def preprocess_statement(frames_bgr: torch.Tensor, size, mean, std) -> torch.Tensor:
    """uint8 BGR [B, H, W, 3] -> pixel_values float32 [B, 3, S, S] as DepthProImageProcessor._preprocess makes them (P:70-80): rescale and normalise
    first, then torchvision's resize of the float tensor -- ``F.interpolate(mode="bilinear", align_corners=False, antialias=False)``."""
    rgb = frames_bgr.flip(-1).permute(0, 3, 1, 2).to(torch.float32)
    k = 1.0 / (1 / 255)
    m = (torch.tensor(mean, dtype=torch.float32) * k).to(rgb.device).view(1, 3, 1, 1)
    s = (torch.tensor(std, dtype=torch.float32) * k).to(rgb.device).view(1, 3, 1, 1)
    return F.interpolate((rgb - m) / s, size=(int(size[0]), int(size[1])), mode="bilinear", align_corners=False, antialias=False)


def post_statement(pred: torch.Tensor, fov, oH: int, oW: int, resize: bool = True) -> torch.Tensor:
    """post_process_depth_estimation (P:102-116) for a batch: float32 [B, S, S] and the field of view [B] (degrees) or None -> inverse depth [B, oH, oW]:
    depth * width / focal with focal = 0.5 width / tan(0.5 deg2rad(fov)), the bilinear resize to the target size, then 1 / clamp(depth, 1e-4, 1e4).
    ``resize=False``: the raw form, no interpolation (the target width still scales the depth)."""
    outs = []
    for b in range(pred.shape[0]):
        depth = pred[b]
        if fov is not None:
            focal = 0.5 * oW / torch.tan(0.5 * torch.deg2rad(fov[b]))
            depth = depth * oW / focal
        if resize:
            depth = F.interpolate(depth[None, None], size=(int(oH), int(oW)), mode="bilinear")[0, 0]
        outs.append(1.0 / torch.clamp(depth, min=1e-4, max=1e4))
    return torch.stack(outs)


# ---------------------------------------------------------------------------------------------------------------- the patch pyramid
def pyramid_levels(S: int, p: int, ratios=(0.25, 0.5, 1), overlaps=(0.0, 0.5, 0.25)):
    """[(ratio, side of the scaled image, stride, patches per side)] in the configuration's order (low resolution first): ``F.interpolate(scale_factor=r)`` gives
    floor(S r) (M:254-262), split_to_patches strides by int(p (1 - overlap)) and leaves an image of exactly one patch alone (M:78-84)."""
    out = []
    for r, o in zip(ratios, overlaps):
        s = int(np.floor(S * r))
        if s < p:
            raise ValueError(f"depth-pro: a {S} x {S} image scaled by {r} is smaller than the {p} x {p} patch")
        stride = p if s == p else int(p * (1 - o))
        out.append((r, s, stride, 1 if s == p else (s - p) // stride + 1))
    return out


def _half(x):
    """F.interpolate(scale_factor=0.5, bilinear, align_corners=False) on even sides: both weights of both axes are exactly 0.5, every product is exact, so the
    value is 0.25 ((top-left + top-right) + (bottom-left + bottom-right)) with the three sums rounded in that order."""
    a, b, c, d = x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]
    return np.float32(0.25) * ((a + b) + (c + d))


def _quarter(x):
    """scale_factor=0.25: source coordinate 4 d + 1.5 -- the 2 x 2 centre of every 4 x 4 cell, in the same order."""
    a, b, c, d = x[..., 1::4, 1::4], x[..., 1::4, 2::4], x[..., 2::4, 1::4], x[..., 2::4, 2::4]
    return np.float32(0.25) * ((a + b) + (c + d))


def patches_statement(x: np.ndarray, p: int, overlaps=(0.0, 0.5, 0.25)) -> np.ndarray:
    """float32 [B, 3, S, S] (S a multiple of 4) -> the stack DepthProPatchEncoder hands its ViT (M:251-273), [(n1 + n2 + n4) B, 3, p, p]: the full-resolution
    patches first, then the half, then the quarter; inside a level patch-major, batch-minor (index l B + b, l = row-major patch position)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, C, S, _ = x.shape
    lv = pyramid_levels(S, p, (0.25, 0.5, 1), overlaps)
    out = []
    for img, (_, s, stride, n) in ((x, lv[2]), (_half(x), lv[1]), (_quarter(x), lv[0])):
        assert img.shape[-1] == s
        for py in range(n):
            for px in range(n):
                out.append(img[:, :, py * stride:py * stride + p, px * stride:px * stride + p])
    return np.stack(out).reshape(-1, C, p, p)   # [patch position over the three levels, B, ...]: a level's patches are complete before the next level starts


# ---------------------------------------------------------------------------------------------------------------- the patch merge
def merge_geometry(n: int, g: int, padding: int):
    """merge_patches' own rules (M:103-126) for n sequences per frame on a g x g token grid -> (side, pad, merged size): side = int(sqrt(n)) patches per
    side (the sequences past side^2 are not used: 35 -> 25), pad = min(g // 4, padding), forced to 0 below four patches; one sequence is left as it is."""
    if n == 1:
        return 1, 0, g
    side = int(n ** 0.5)
    pad = min(g // 4, 0 if n < 4 else int(padding))
    return side, pad, side * g - 2 * pad * (side - 1)


def merge_index(side: int, g: int, pad: int):
    """Per merged coordinate (one axis): (patch index, token index).  Padding is trimmed only on edges that meet another patch (M:153-170)."""
    h, t = [], []
    for k in range(side):
        lo, hi = (pad if k else 0), (g - pad if k != side - 1 else g)
        h += [k] * (hi - lo)
        t += list(range(lo, hi))
    return np.asarray(h, np.int64), np.asarray(t, np.int64)


def aten_linear_taps(inp: int, out: int):
    """ATen's bilinear taps of one axis without antialias, align_corners=False, no scale factor given (UpSampleKernel.cpp, compute_source_index_and_lambda),
    in float32 -> (i0, i1, lambda0, lambda1): equal sizes are the identity (i1 = i0, weights 1 and 0); otherwise scale = float32(in) / out,
    src = max(scale (d + 0.5) - 0.5, 0), i0 = min(floor(src), in - 1), lambda1 = clamp(src - i0, 0, 1), i1 = i0 + (i0 < in - 1), lambda0 = 1 - lambda1."""
    d = np.arange(out, dtype=np.float32)
    if inp == out:
        i0 = np.arange(out, dtype=np.int64)
        return i0, i0.copy(), np.ones(out, np.float32), np.zeros(out, np.float32)
    scale = np.float32(inp) / np.float32(out)
    src = np.maximum(scale * (d + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), inp - 1)
    l1 = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    i1 = i0 + (i0 < inp - 1)
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def merge_statement(rows: np.ndarray, B: int, g: int, padding: int, oh: int, ow: int) -> np.ndarray:
    """reconstruct_feature_maps (M:181-217) in NHWC: token rows float32 [n B, T, C] (T >= g^2: the leading T - g^2 tokens -- the class token -- are dropped)
    -> [B, oh, ow, C].  The bilinear resize is skipped where the merged size is the output size (ATen's weights are exactly 1 and 0 there); elsewhere
    out = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), every operation rounded to float32 on its own."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    nB, T, C = rows.shape
    n = nB // B
    side, pad, M = merge_geometry(n, g, padding)
    h, t = merge_index(side, g, pad)
    tok = rows[:, T - g * g:, :].reshape(n, B, g, g, C)
    seq = h[:, None] * side + h[None, :]                                      # [M, M] patch position l
    merged = tok[seq, :, t[:, None], t[None, :], :].transpose(2, 0, 1, 3)     # [B, M, M, C]
    if (M, M) == (oh, ow):
        return np.ascontiguousarray(merged)
    y0, y1, ly0, ly1 = aten_linear_taps(M, oh)
    x0, x1, lx0, lx1 = aten_linear_taps(M, ow)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    top = lx0 * merged[:, y0][:, :, x0] + lx1 * merged[:, y0][:, :, x1]
    bot = lx0 * merged[:, y1][:, :, x0] + lx1 * merged[:, y1][:, :, x1]
    return (ly0[None, :, None, None] * top + ly1[None, :, None, None] * bot).astype(np.float32)
