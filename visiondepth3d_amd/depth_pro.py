"""DepthPro (``apple/DepthPro-hf``, ``DepthProForDepthEstimation``) behind DepthPipe: the published geometry; the image processor and its post-process stated
in torch (what the two kernels of csrc/vd3d_depthpro.hip are held to, and what runs where there is no renderer); and the model's patch order and merge geometry
stated in NumPy: ``patches_statement`` and ``merge_statement`` are what the two kernels of csrc/vd3d_depthpro_pyramid.hip (``vd3d_depthpro_patches_f32``,
``vd3d_depthpro_merge_f32``) give bit for bit (tests/test_hip_depth_pro_pyramid.py).  Those kernels run under ``DepthPipe(encoders="bf16x3" | "fp16x2")``, which
routes the three encoders (``encoders_scope``, ``EncoderRoutes``); by default the network is the stock module graph and no kernel runs them.
``DepthPipe(encoders=..., decoder="bf16x3" | "fp16x2")`` routes the neck, the fusion stage, the head and the field-of-view convolutions as well: the last sections
hold the float64 statements of the two composed weights (``deconv_projection_compose``; ``head_poly_statement`` with ``head_poly_table``, what
csrc/vd3d_depthpro_head.hip computes), the scope check ``decoder_scope`` and the routes themselves, ``DecoderRoutes``.

Line numbers are those of the installed transformers: ``models/depth_pro/modeling_depth_pro.py`` (M), ``models/depth_pro/image_processing_depth_pro.py`` (P)
and ``image_processing_backends.py`` (B).

The geometry below is the published one AS FAR AS IT IS KNOWN HERE: no copy of the checkpoint's config.json was at hand when this was written, so nothing has
confirmed it against the file.  A checkpoint loads with whatever geometry its own config.json states (``DepthPipe.from_pretrained``)."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from .depth_compose import im2col_gemm_weight, neck_poly_compose, neck_poly_offsets, patch_embedding_conv_ok
from .depth_routes import _ConvTransposeGemm, _head_tail_operands, patch_embedding_rows
from .vit_blocks import dinov2_operands, encoder_blocks, head_geometry_ok

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


# ---------------------------------------------------------------------------------------------------------------- the decoder: composed weights, stated in float64
def deconv_projection_compose(deconv_w: torch.Tensor, proj_w: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """DepthProFeatureFusionLayer's bias-free ``deconv`` (ConvTranspose2d weight [C_in, C, s, s], kernel == stride) followed by its 1 x 1 ``projection`` (weight
    [C_out, C, 1, 1] or [C_out, C]) is one transposed convolution: W'[ci, co, i, j] = sum_c deconv_w[ci, c, i, j] proj_w[co, c] -- nothing non-linear sits between
    them and the projection acts per pixel.  Composed in float64, rounded once to ``dtype``; the projection's bias is added behind it (depth-to-space)."""
    if deconv_w.dim() != 4 or deconv_w.shape[2] != deconv_w.shape[3] or proj_w.dim() not in (2, 4) or (proj_w.dim() == 4 and tuple(proj_w.shape[2:]) != (1, 1)):
        raise ValueError(f"deconv_projection: weights {tuple(deconv_w.shape)} / {tuple(proj_w.shape)} are not [C_in, C, s, s] and [C_out, C, 1, 1]")
    P = proj_w.detach().to(torch.float64).reshape(proj_w.shape[0], -1)
    if P.shape[1] != deconv_w.shape[1]:
        raise ValueError(f"deconv_projection: the projection reads {P.shape[1]} channels, the transposed convolution writes {deconv_w.shape[1]}")
    return torch.einsum("icyx,oc->ioyx", deconv_w.detach().to(torch.float64), P).to(dtype).contiguous()


def head_poly_table(bt: torch.Tensor, w3: torch.Tensor, b2: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """The constant term of conv3x3(ConvTranspose2d(x) + bt) + b2 per border class, [3, 3, C_out] indexed by (first / interior / last fine row, likewise the
    column): T = b2 + sum of W3[:, :, dy, dx] @ bt over the taps (dy, dx) whose fine pixel lies inside the map -- the convolution pads the FINE map with zeros,
    not with bt (``neck_poly_compose``'s docstring), so the first row loses dy = -1 and the last dy = +1.  A transposed convolution with stride 2 gives at least
    two fine rows and columns: first and last never coincide.  Float64, rounded once to ``dtype``."""
    s = torch.einsum("ocyx,c->oyx", w3.detach().to(torch.float64), bt.detach().to(torch.float64))
    keep = ((1, 2), (0, 1, 2), (0, 1))
    T = torch.zeros(3, 3, w3.shape[0], dtype=torch.float64, device=w3.device)
    for ry in range(3):
        for rx in range(3):
            T[ry, rx] = b2.detach().to(torch.float64) + sum(s[:, ky, kx] for ky in keep[ry] for kx in keep[rx])
    return T.to(dtype).contiguous()


def head_poly_statement(x: torch.Tensor, wt: torch.Tensor, bt: torch.Tensor, w3: torch.Tensor, b2: torch.Tensor, w1: torch.Tensor, b3, operands=torch.float64):
    """What vd3d_depthpro_head computes, in float64: [B, C, h, w] -> [B, 2h, 2w] =
        relu(conv1x1(relu(conv3x3(ConvTranspose2d_k2s2(x; wt) + bt; w3) + b2); w1) + b3)
    as the 16 composed blocks of ``neck_poly_compose(wt, None, w3, 2)`` on the coarse grid -- output phase (pa, pb), four taps at coarse offsets (pa - 1 | pa,
    pb - 1 | pb), pixels outside the map contributing nothing -- plus ``head_poly_table``'s border-class constant, ReLU, the 32-term dot product with ``w1``
    ([1, 32, 1, 1] or [32]), ``b3``, ReLU.  ``operands``: the dtype the blocks and the table are rounded to once (float32: the kernel's operands)."""
    Wc, _ = neck_poly_compose(wt, None, w3, 2, dtype=operands)
    T = head_poly_table(bt, w3, b2, dtype=operands).to(torch.float64)
    Wc, x = Wc.to(torch.float64), x.detach().to(torch.float64)
    B, _, h, w = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    v = torch.zeros(B, w3.shape[0], 2 * h, 2 * w, dtype=torch.float64, device=x.device)
    for k, (pa, pb, di, dj) in enumerate(neck_poly_offsets(2)):
        v[:, :, pa::2, pb::2] += torch.einsum("oc,bchw->bohw", Wc[k], xp[:, :, 1 + di:1 + di + h, 1 + dj:1 + dj + w])
    ry = torch.tensor([0] + [1] * (2 * h - 2) + [2], device=x.device)
    rx = torch.tensor([0] + [1] * (2 * w - 2) + [2], device=x.device)
    u = torch.relu(v + T[ry][:, rx].permute(2, 0, 1))
    d = torch.einsum("o,bohw->bhw", w1.detach().to(torch.float64).reshape(-1), u)
    return torch.relu(d + float(b3))


# ---------------------------------------------------------------------------------------------------------------- the encoders on own kernels: DepthPipe(encoders=...)
def encoders_scope(model, name: str, mode, processor) -> dict:
    """``encoders=``: what the routing needs of the model and its processor, read from the module graph and the configuration only (nothing is moved or
    launched); everything it does not cover is refused by name.  Returns the plan ``EncoderRoutes`` executes: the processor side, DepthPro's patch size, the
    pyramid levels and the names of the encoders present."""
    m, tag = model, f"encoders={mode!r}"
    what = f"{name!r} ({type(m).__name__})"
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
    size = tuple(int(v) for v in (PROCESSOR if processor is None else processor)["size"])
    if size[0] != size[1] or size[0] % 4:
        raise NotImplementedError(f"{tag}: {what}: a processor size of {size} -- the pyramid kernel takes a square side that is a multiple of 4")
    p = int(cfg.patch_size)
    try:
        levels = pyramid_levels(size[0], p, ratios, [float(o) for o in cfg.scaled_images_overlap_ratios])
    except ValueError as e:
        raise NotImplementedError(f"{tag}: {what}: a pyramid vd3d_depthpro_patches_f32 is not built for -- {e}") from None
    if any(stride < 1 for _, _, stride, _ in levels):
        raise NotImplementedError(f"{tag}: {what}: a pyramid vd3d_depthpro_patches_f32 is not built for -- scaled_images_overlap_ratios="
                                  f"{list(cfg.scaled_images_overlap_ratios)} leave a stride below 1")
    return dict(size=size[0], patch=p, ratios=ratios, overlaps=[float(o) for o in cfg.scaled_images_overlap_ratios], which=[w for w, _ in found])


class EncoderRoutes:
    """``DepthPipe(encoders=mode)``: the forwards of DepthProPatchEncoder, DepthProImageEncoder and DepthProFovEncoder replaced (``encoders_scope`` has accepted the
    model; ``plan`` is what it returned), so that between ``pixel_values`` and the inputs of DepthProNeck / ``fov_model.conv`` every launch is one of this
    project's kernels or an ATen element-wise one (the class-token concatenation, the position-embedding add, the last block's residual add) -- no hipBLASLt,
    MIOpen or AOTriton call:
      * the patch pyramid: one launch of vd3d_depthpro_patches_f32, written in the memory patchify reads;
      * per encoder (``make_encoder``): vd3d_patchify_f32 + vd3d_gemm_x3 for the patch embedding, the class token and the (memoised) position embedding added, every
        Dinov2Layer a _split_block in ``mode`` (vit_blocks.encoder_blocks: one weight split / pack per encoder, here), the hook layers' residual streams kept, the
        final LayerNorm as add_layernorm(x, None, ln);
      * every reconstruct_feature_maps (``merge``): vd3d_depthpro_merge_f32, handed on as the [B, C, oh, ow] view of its NHWC storage (channels_last, what the
        library convolutions behind it read);
      * the field-of-view encoder's ``neck`` Linear: vd3d_gemm_x3.
    Where floor(S / 4) is DepthPro's patch size and the image / field-of-view encoder's image_size, that encoder reads the pyramid's quarter level (the last
    patch of the stack: F.interpolate(size=) and F.interpolate(scale_factor=0.25) give the same bits there); otherwise its resize stays an ATen call (``own_input``;
    ``pipe.encoders_resize`` says which).  ``pixel_values`` / ``quarter``: the forward in flight and its quarter level, from the patch encoder's call to the last reader's."""

    def __init__(self, pipe, mode: str, plan: dict):
        from transformers.models.depth_pro.modeling_depth_pro import DepthProOutput
        self.pipe, self.R, self.mode, self.plan, self.Out = pipe, pipe.renderer, mode, plan, DepthProOutput
        self.pixel_values = self.quarter = None
        m = pipe.model
        self.pe_mod, self.ie_mod = m.depth_pro.encoder.patch_encoder, m.depth_pro.encoder.image_encoder
        self.run_patch, self.run_image = self.make_encoder(self.pe_mod.model), self.make_encoder(self.ie_mod.model)
        self.hook_ids = [int(i) for i in self.pe_mod.intermediate_hook_ids]
        self.pe_mod.forward, self.ie_mod.forward = self.patch_forward, self.image_forward
        if m.fov_model is not None:
            self.fe_mod = m.fov_model.fov_encoder
            self.run_fov = self.make_encoder(self.fe_mod.model)
            self.neck_img = self.R.gemm_x3_pack(self.fe_mod.neck.weight, mode)
            self.fe_mod.forward = self.fov_forward

    def make_encoder(self, vit):
        R, emb = self.R, vit.embeddings
        rows = patch_embedding_rows(R, emb.patch_embeddings.projection, self.mode)
        blocks = encoder_blocks(R, [dinov2_operands(lay) for lay in vit.encoder.layer], self.mode, keyword="encoders")
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

    @staticmethod
    def base_size(enc, height, width):   # the lowest-resolution feature size, as the stock forwards compute it
        e = int(math.log2(width / enc.out_size))
        return height // 2 ** e, width // 2 ** e

    def merge(self, rows, B, padding, oh, ow):
        return self.R.depthpro_merge(rows.contiguous(), B, int(rows.shape[1] ** 0.5), padding, oh, ow).permute(0, 3, 1, 2)

    def own_input(self, which, enc_cfg, pixel_values):
        """The [B, 3, size, size] input of the image / field-of-view encoder in channels_last memory."""
        size = int(enc_cfg.image_size)
        q = self.quarter if self.pixel_values is pixel_values else None
        if q is not None and pixel_values.shape[-1] // 4 == size == self.plan["patch"] and tuple(q.shape[-2:]) == (size, size):
            self.pipe.encoders_resize[which] = "pyramid"
            return q
        self.pipe.encoders_resize[which] = "aten"
        return F.interpolate(pixel_values, size=(size, size), mode="bilinear", align_corners=False).contiguous(memory_format=torch.channels_last)

    def check(self, pixel_values):
        if pixel_values.dtype != torch.float32 or pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
            raise NotImplementedError(f"encoders={self.mode!r}: float32 [B, 3, S, S] pixel values expected -- refusing to fall back silently")

    def patch_forward(self, pixel_values):
        self.check(pixel_values)
        pe_mod, p, ratios = self.pe_mod, self.plan["patch"], self.plan["ratios"]
        B, _, H, W = pixel_values.shape
        if H != W or H % 4:
            raise NotImplementedError(f"encoders={self.mode!r}: a {H} x {W} input -- the pyramid kernel takes a square side that is a multiple of 4")
        lv = pyramid_levels(H, p, ratios, self.plan["overlaps"])   # low resolution first
        patches = self.R.depthpro_patches(pixel_values.contiguous(), p, [lv[2][2], lv[1][2], lv[0][2]])
        self.pixel_values, self.quarter = pixel_values, (patches[-B:] if lv[0][3] == 1 else None)
        last, kept = self.run_patch(patches, set(self.hook_ids))
        bh, bw = self.base_size(pe_mod, H, W)
        feats, start = [None] * 3, 0
        for i in (2, 1, 0):   # the stack holds the high-resolution patches first, the features are listed low resolution first
            cnt = lv[i][3] ** 2 * B
            feats[i] = self.merge(last[start:start + cnt], B, int(pe_mod.merge_padding_value * (1 / ratios[i])), bh * 2 ** i, bw * 2 ** i)
            start += cnt
        for i in self.hook_ids:
            feats.append(self.merge(kept[i], B, int(pe_mod.merge_padding_value * (1 / ratios[-1])), bh * 4, bw * 4))
        return feats

    def image_forward(self, pixel_values, output_attentions=False, output_hidden_states=False, return_dict=True):
        self.check(pixel_values)
        if output_attentions or output_hidden_states:
            raise NotImplementedError(f"encoders={self.mode!r}: the routed image encoder keeps no attentions or hidden states")
        B, _, H, W = pixel_values.shape
        last, _ = self.run_image(self.own_input("image", self.pipe.model.config.image_model_config, pixel_values))
        feats = self.merge(last, B, 0, *self.base_size(self.ie_mod, H, W))
        return self.Out(last_hidden_state=last, features=feats) if return_dict else (last, feats)

    def fov_forward(self, pixel_values):
        self.check(pixel_values)
        B, _, H, W = pixel_values.shape
        neck = self.fe_mod.neck
        last, _ = self.run_fov(self.own_input("fov", self.pipe.model.config.fov_model_config, pixel_values))
        self.pixel_values = self.quarter = None   # the last reader of the forward in flight
        return self.merge(self.R.linear_x3(last, self.neck_img, neck.out_features, neck.bias, mode=self.mode), B, 0, *self.base_size(self.fe_mod, H, W))


# ---------------------------------------------------------------------------------------------------------------- the decoder on own kernels: DepthPipe(decoder=...)
# The argument sets of vd3d_conv3x3_epi the decoder uses: a residual unit's first convolution (ReLU in front, bias + ReLU behind), its second one (bias + the
# unit's input, and in residual_layer1 the fusion layer's running state as well), and head.layers.0 (bias alone).
DECODER_EPI_SETS = ("relu_in+bias+relu", "bias+r1", "bias+r1+r2", "bias")
DECODER_EPI_BUILT = tuple((mode, s) for mode in ("bf16x3", "fp16x2") for s in DECODER_EPI_SETS)
# ... and those routed by default: the (mode, argument set) pairs whose fused launch beat bias-free convolution + vd3d_nhwc_bias_act_f32 by more than the rounds'
# spread at 256 -> 256 channels (profiles/r29_depth_pro_decoder.md); VD3D_DEPTHPRO_RES_EPI=1 routes every built pair, =0 none.
DECODER_EPI_ROUTED = tuple((mode, s) for mode in ("bf16x3", "fp16x2") for s in ("relu_in+bias+relu", "bias"))
DECODER_HEAD_POLY_BUILT = ("bf16x3", "fp16x2")     # modes of vd3d_depthpro_head
DECODER_HEAD_POLY_ROUTED = DECODER_HEAD_POLY_BUILT   # ... routed by default (the same profile); VD3D_DEPTHPRO_HEAD_POLY=1 / =0 as above


# The A/B switches of the two new kernels (environment variables, read per forward; depth_routes._SWITCHES' convention): unset, the ROUTED tables above decide; "1"
# routes every built form; "0" puts the residual units back on bias-free convolution + vd3d_nhwc_bias_act_f32 | the head on GEMM + depth-to-space + tile
# convolution + vd3d_dpt_head_tail_f32.
IM2COL_KERNELS = (1, 3, 7)   # the window sizes vd3d_im2col_nhwc_f32 builds
DECODER_SWITCHES = ("VD3D_DEPTHPRO_RES_EPI", "VD3D_DEPTHPRO_HEAD_POLY")


def decoder_switch(name: str):
    """The switch ``name`` of DECODER_SWITCHES as it stands in the environment NOW: False for "0", True for "1", None (the tables decide) otherwise."""
    import os
    if name not in DECODER_SWITCHES:
        raise KeyError(name)
    return {"0": False, "1": True}.get(os.environ.get(name))


def _conv_is(m, k, s, p):
    return (isinstance(m, torch.nn.Conv2d) and m.kernel_size == (k, k) and m.stride == (s, s) and m.padding == (p, p) and m.dilation == (1, 1) and m.groups == 1
            and m.padding_mode == "zeros")


def _deconv_is_k2s2(m):
    return (isinstance(m, torch.nn.ConvTranspose2d) and m.kernel_size == (2, 2) and m.stride == (2, 2) and m.padding == (0, 0) and m.output_padding == (0, 0)
            and m.dilation == (1, 1) and m.groups == 1)


def decoder_scope(model, name: str, mode, size: int):
    """``decoder=``: what the routes need of the module graph, read from the modules and the configuration only (nothing is moved or launched); whatever they do
    not take is refused by name.  ``size``: the processor's square side.  Returns the list of (module name, module) the routes cover."""
    tag, what = f"decoder={mode!r}", f"{name!r} ({type(model).__name__})"
    if type(model).__name__ != "DepthProForDepthEstimation":
        raise NotImplementedError(f"{tag}: {what} -- the keyword routes the neck, the fusion stage, the head and the field-of-view convolutions of "
                                  "DepthProForDepthEstimation; every other model takes gemm= / conv= / self_contained=")
    cfg, names = model.config, {id(m): n for n, m in model.named_modules()}
    if getattr(cfg, "use_batch_norm_in_fusion_residual", False):
        raise NotImplementedError(f"{tag}: {what}: use_batch_norm_in_fusion_residual=True -- the residual units' epilogue (vd3d_conv3x3_epi) is bias, residual and ReLU; "
                                  "a BatchNorm2d between the convolutions is not built")
    Fh = int(cfg.fusion_hidden_size)
    if Fh not in (64, 128, 256):
        raise NotImplementedError(f"{tag}: {what}: fusion_hidden_size={Fh} -- the tile convolution writes 32 / 64 / 128 / 256 channels and the head halves the width: "
                                  "64, 128 and 256 are built")
    covered = []

    def need(ok, m, expect):
        if not ok:
            raise NotImplementedError(f"{tag}: {what}: {names[id(m)]} is not {expect} -- not built")
        covered.append((names[id(m)], m))

    def tile_ok(m):
        return m.in_channels % 16 == 0 and m.out_channels in (32, 64, 128, 256)
    neck = model.depth_pro.neck
    up = neck.feature_upsample
    for block, lead_proj in [(up.image_block, False)] + [(b, True) for b in list(up.scaled_images) + list(up.intermediate)]:
        layers = list(block.layers)
        if lead_proj:
            need(_conv_is(layers[0], 1, 1, 0) and layers[0].in_channels % 16 == 0, layers[0], "a 1 x 1 convolution with C_in a multiple of 16")
            layers = layers[1:]
        for m in layers:
            need(_deconv_is_k2s2(m) and m.in_channels % 16 == 0, m, "a ConvTranspose2d with kernel = stride = 2 and C_in a multiple of 16")
    need(_conv_is(neck.fuse_image_with_low_res, 1, 1, 0) and neck.fuse_image_with_low_res.in_channels % 16 == 0, neck.fuse_image_with_low_res,
         "a 1 x 1 convolution with C_in a multiple of 16")
    for m in neck.feature_projection.projections:
        if not isinstance(m, torch.nn.Identity):
            need(_conv_is(m, 3, 1, 1) and m.bias is None and tile_ok(m), m, "a bias-free 3 x 3 / stride 1 / padding 1 convolution the tile kernel builds")
    for layer in list(model.fusion_stage.intermediate) + [model.fusion_stage.final]:
        for unit in (layer.residual_layer1, layer.residual_layer2):
            for m in (unit.convolution1, unit.convolution2):
                need(_conv_is(m, 3, 1, 1) and tile_ok(m), m, "a 3 x 3 / stride 1 / padding 1 convolution the tile kernel builds")
        if layer.use_deconv:
            need(_deconv_is_k2s2(layer.deconv) and layer.deconv.bias is None and layer.deconv.in_channels % 16 == 0, layer.deconv,
                 "a bias-free ConvTranspose2d with kernel = stride = 2")
        need(_conv_is(layer.projection, 1, 1, 0) and layer.projection.in_channels % 16 == 0, layer.projection, "a 1 x 1 convolution with C_in a multiple of 16")
    hl = list(model.head.layers)
    shape_ok = (len(hl) == 6 and isinstance(hl[3], torch.nn.ReLU) and isinstance(hl[5], torch.nn.ReLU) and isinstance(hl[2], torch.nn.Conv2d)
                and isinstance(hl[4], torch.nn.Conv2d))
    if not shape_ok:
        raise NotImplementedError(f"{tag}: {what}: a head other than [conv 3 x 3, ConvTranspose2d 2 x 2 / 2, conv 3 x 3, ReLU, conv 1 x 1, ReLU] -- not built")
    if hl[2].out_channels != 32:
        raise NotImplementedError(f"{tag}: {what}: head.layers.2 writes {hl[2].out_channels} channels -- vd3d_depthpro_head and vd3d_dpt_head_tail_f32 behind the "
                                  "head's last 3 x 3 convolution are built for 32")
    need(_conv_is(hl[0], 3, 1, 1) and hl[0].bias is not None and tile_ok(hl[0]), hl[0], "a biased 3 x 3 / stride 1 / padding 1 convolution the tile kernel builds")
    need(_deconv_is_k2s2(hl[1]) and hl[1].bias is not None and hl[1].in_channels % 16 == 0 and hl[1].out_channels == hl[1].in_channels, hl[1],
         "a biased ConvTranspose2d(C, C) with kernel = stride = 2 and C a multiple of 16")
    need(_conv_is(hl[2], 3, 1, 1) and hl[2].bias is not None and hl[2].in_channels % 16 == 0, hl[2], "a biased 3 x 3 / stride 1 / padding 1 convolution")
    need(_conv_is(hl[4], 1, 1, 0) and hl[4].out_channels == 1 and hl[4].bias is not None, hl[4], "a biased 1 x 1 convolution to one channel")
    fov = model.fov_model
    if fov is not None:   # use_fov_model=False: nothing to route there
        import math
        out_size = int(fov.head.out_size)
        base = int(size) // 2 ** int(math.log2(int(size) / fov.fov_encoder.out_size))
        conv_out = ((base * 2) + 1) // 2
        if base != out_size or conv_out != out_size:
            raise NotImplementedError(f"{tag}: {what}: at a {size} x {size} input the field-of-view head resizes its {base} x {base} features to {out_size} x {out_size} "
                                      "(F.interpolate) -- only the identity is built")
        need(_conv_is(fov.conv, 3, 2, 1) and fov.conv.bias is not None and fov.conv.in_channels % 16 == 0, fov.conv, "a biased 3 x 3 / stride 2 / padding 1 convolution")
        convs = [m for m in fov.head.layers if not isinstance(m, torch.nn.ReLU)]
        for m in convs[:-1]:
            need(_conv_is(m, 3, 2, 1) and m.bias is not None, m, "a biased 3 x 3 / stride 2 / padding 1 convolution")
        last, side = convs[-1], out_size
        for _ in convs[:-1]:
            side = (side + 1) // 2
        if isinstance(last, torch.nn.Conv2d) and last.kernel_size[0] not in IM2COL_KERNELS and last.kernel_size != (side, side):
            raise NotImplementedError(f"{tag}: {what}: {names[id(last)]} has a {last.kernel_size[0]} x {last.kernel_size[1]} window on a {side} x {side} map -- "
                                      f"vd3d_im2col_nhwc_f32 builds kernels of {' | '.join(map(str, IM2COL_KERNELS))}, and only a window that is the whole map needs none")
        need(isinstance(last, torch.nn.Conv2d) and last.kernel_size[0] == last.kernel_size[1] and last.stride == (1, 1) and last.padding == (0, 0)
             and last.dilation == (1, 1) and last.groups == 1 and last.bias is not None, last, "a biased k x k / stride 1 / padding 0 convolution")
    return covered


class DecoderRoutes:
    """``DepthPipe("depth-pro", encoders=M1, decoder=mode)``: the forwards of DepthProNeck, DepthProFeatureFusionStage, DepthProDepthEstimationHead and
    DepthProFovModel replaced (``decoder_scope`` has accepted the model) so that every Conv2d / ConvTranspose2d between the encoders' merges and
    ``predicted_depth`` / ``field_of_view`` is one of this project's kernels in ``mode``; what is left to ATen is element-wise (ReLU, add), ``cat``, views and
    copies.  All maps are float32 NHWC (channels_last [B, C, h, w] tensors); every weight is packed once, here.
      * 1 x 1 convolutions: vd3d_gemm_x3 over the pixel rows (the NHWC storage is the row matrix); ``fuse_image_with_low_res`` over the concatenated rows.
      * kernel = stride = 2 transposed convolutions: depth_routes._ConvTransposeGemm (GEMM + vd3d_depth_to_space_bias_nhwc_f32).
      * ``feature_projection.projections``: the tile convolution, bare.
      * residual units: vd3d_conv3x3_epi per argument set (DECODER_EPI_ROUTED, VD3D_DEPTHPRO_RES_EPI), else bias-free tile convolution + vd3d_nhwc_bias_act_f32 --
        the same bits either way.
      * a fusion layer's ``deconv`` + ``projection``: ONE GEMM with the two weights composed (``deconv_projection_compose``), depth-to-space with the projection's
        bias; ``final.projection``: vd3d_gemm_x3.
      * ``head.layers.0``: vd3d_conv3x3_epi with a bias only; ``head.layers.1 .. 5``: vd3d_depthpro_head (DECODER_HEAD_POLY_ROUTED, VD3D_DEPTHPRO_HEAD_POLY), else
        GEMM + depth-to-space, bias-free tile convolution, vd3d_dpt_head_tail_f32.
      * ``fov_model.conv``: the stride-2 tile convolution where it builds the shape (C_out a multiple of 128) + bias_act, else vd3d_im2col_nhwc_f32 + vd3d_gemm_x3;
        ``fov_model.head.layers``: vd3d_im2col_nhwc_f32 + vd3d_gemm_x3 (K and N zero-padded to multiples of 16).
    ``pipe.decoder_routes`` (module name -> route) says, per forward, where each module ran and in which form."""

    def __init__(self, pipe, mode: str):
        import types
        self.pipe, self.R, self.mode, self.names = pipe, pipe.renderer, mode, pipe._names
        R, m = self.R, pipe.model
        self.routes = pipe.decoder_routes
        self._g1, self._ct, self._tile = {}, {}, {}
        neck = m.depth_pro.neck
        up = neck.feature_upsample
        for block in [up.image_block] + list(up.scaled_images) + list(up.intermediate):
            for lay in block.layers:
                if isinstance(lay, torch.nn.ConvTranspose2d):
                    self._ct[id(lay)] = _ConvTransposeGemm(R, lay, mode)
                else:
                    self._g1[id(lay)] = R.gemm_x3_pack(lay.weight.reshape(lay.out_channels, lay.in_channels), mode)
        self._g1[id(neck.fuse_image_with_low_res)] = R.gemm_x3_pack(neck.fuse_image_with_low_res.weight.reshape(neck.fuse_image_with_low_res.out_channels, -1), mode)
        for pj in neck.feature_projection.projections:
            if not isinstance(pj, torch.nn.Identity):
                self._tile[id(pj)] = R.conv3x3_tile_pack(pj.weight, mode, 1)
        for layer in list(m.fusion_stage.intermediate) + [m.fusion_stage.final]:
            for unit in (layer.residual_layer1, layer.residual_layer2):
                for cv in (unit.convolution1, unit.convolution2):
                    self._tile[id(cv)] = R.conv3x3_tile_pack(cv.weight, mode, 1)
            pj = layer.projection
            if layer.use_deconv:
                w = deconv_projection_compose(layer.deconv.weight, pj.weight)
                self._ct[id(layer)] = _ConvTransposeGemm(R, types.SimpleNamespace(weight=w, bias=pj.bias, kernel_size=(2, 2), out_channels=pj.out_channels), mode)
            else:
                self._g1[id(pj)] = R.gemm_x3_pack(pj.weight.reshape(pj.out_channels, pj.in_channels), mode)
        hl = m.head.layers
        self._tile[id(hl[0])] = R.conv3x3_tile_pack(hl[0].weight, mode, 1)
        self._head_poly = R.depthpro_head_pack(neck_poly_compose(hl[1].weight, None, hl[2].weight, 2)[0], mode)
        self._head_T = head_poly_table(hl[1].bias, hl[2].weight, hl[2].bias).to(pipe.device)
        self._head_b2 = hl[2].bias.detach().clone().contiguous()
        self._head_tail = _head_tail_operands(hl[4])
        self._ct[id(hl[1])] = _ConvTransposeGemm(R, hl[1], mode)
        self._tile[id(hl[2])] = R.conv3x3_tile_pack(hl[2].weight, mode, 1)   # None where the fallback's 3 x 3 is not built (C_in % 16 has been checked: never)
        if any(v is None for v in self._tile.values()) or self._head_poly is None:
            raise NotImplementedError(f"decoder={mode!r}: a weight image was refused by the library although decoder_scope accepted the module -- not built")
        self._im2col = {}
        fov = m.fov_model
        if fov is not None:
            self._fov_s2 = R.conv3x3_tile_pack(fov.conv.weight, mode, 2)   # None: C_out is no multiple of 128 (or C_in % 16)
            for cv in [fov.conv] + [c for c in fov.head.layers if isinstance(c, torch.nn.Conv2d)]:
                n, npad = cv.out_channels, (cv.out_channels + 15) // 16 * 16
                w = F.pad(im2col_gemm_weight(cv.weight), (0, 0, 0, npad - n))
                self._im2col[id(cv)] = (R.gemm_x3_pack(w, mode), npad, F.pad(cv.bias.detach(), (0, npad - n)).contiguous())
            fov.forward = self.fov_forward
        neck.forward = self.neck_forward
        m.fusion_stage.forward = self.fusion_forward
        m.head.forward = self.head_forward

    # ---- pieces
    def _note(self, m, route):
        self.routes[self.names[id(m)]] = route

    @staticmethod
    def _rows(x):   # channels_last [B, C, h, w] -> its NHWC rows [B, h, w, C] (a view of the same storage where x is channels_last)
        return x.permute(0, 2, 3, 1).contiguous()

    def conv1x1(self, m, rows):
        self._note(m, "vd3d_gemm_x3")
        return self.R.linear_x3(rows, self._g1[id(m)], m.out_channels, m.bias, mode=self.mode)

    def deconv(self, m, rows):
        B, h, w, _ = rows.shape
        self._note(m, "vd3d_gemm_x3 + vd3d_depth_to_space_bias_nhwc_f32")
        return self._ct[id(m)](rows, B, h, w)

    def tile(self, m, x, note=True):
        if note:
            self._note(m, f"vd3d_conv3x3_{self.R.TILE_CONVS[self.mode, 1]}")
        return self.R.conv3x3_tile(x.contiguous(memory_format=torch.channels_last), self._tile[id(m)], m.out_channels, self.mode, 1)

    def _epi_on(self, arg_set):
        sw = decoder_switch("VD3D_DEPTHPRO_RES_EPI")
        if sw is False:
            return False, "VD3D_DEPTHPRO_RES_EPI=0"
        return (self.mode, arg_set) in (DECODER_EPI_BUILT if sw else DECODER_EPI_ROUTED), "not routed: profiles/r29_depth_pro_decoder.md"

    def conv_epi(self, m, x, arg_set, r1=None, r2=None):
        """m's 3 x 3 convolution with its glue (``arg_set`` of DECODER_EPI_SETS): one vd3d_conv3x3_epi launch, or [ReLU ->] bias-free convolution ->
        vd3d_nhwc_bias_act_f32 -- the same bits."""
        R, relu = self.R, arg_set == "relu_in+bias+relu"
        x = x.contiguous(memory_format=torch.channels_last)
        on, why = self._epi_on(arg_set)
        fam = R.TILE_CONVS[self.mode, 1]
        if on:
            self._note(m, f"vd3d_conv3x3_epi ({arg_set})")
            return R.conv3x3_epi(x, self._tile[id(m)], m.out_channels, self.mode, bias=m.bias, r1=r1, r2=r2, relu_in=relu, relu=relu)
        self._note(m, f"vd3d_conv3x3_{fam} + vd3d_nhwc_bias_act_f32 ({why})")
        return R.bias_act(self.tile(m, torch.relu(x) if relu else x, note=False), m.bias, r1=r1, r2=r2, relu=relu)

    def res_unit(self, unit, x, extra=None):
        """DepthProPreActResidualLayer: conv2(relu(conv1(relu(x)))) + x [then extra + that]."""
        x = x.contiguous(memory_format=torch.channels_last)
        y = self.conv_epi(unit.convolution1, x, "relu_in+bias+relu")
        return self.conv_epi(unit.convolution2, y, "bias+r1" if extra is None else "bias+r1+r2", r1=x,
                             r2=None if extra is None else extra.contiguous(memory_format=torch.channels_last))

    # ---- the four forwards
    def neck_forward(self, features):
        f, up, neck = list(features), self.pipe.model.depth_pro.neck.feature_upsample, self.pipe.model.depth_pro.neck

        def block(b, x):
            for lay in b.layers:
                rows = self._rows(x)
                x = self.deconv(lay, rows) if isinstance(lay, torch.nn.ConvTranspose2d) else self.conv1x1(lay, rows).permute(0, 3, 1, 2)
            return x
        f[0] = block(up.image_block, f[0])
        for i, b in enumerate(up.scaled_images):
            f[i + 1] = block(b, f[i + 1])
        n = len(up.scaled_images)
        for i, b in enumerate(up.intermediate):
            f[n + i + 1] = block(b, f[n + i + 1])
        g = self.conv1x1(neck.fuse_image_with_low_res, torch.cat((self._rows(f[1]), self._rows(f[0])), dim=-1)).permute(0, 3, 1, 2)
        out = []
        for pj, x in zip(neck.feature_projection.projections, [g, *f[2:]]):
            out.append(x if isinstance(pj, torch.nn.Identity) else self.tile(pj, x))
        return out

    def fusion_layer(self, layer, hidden, residual=None):
        if residual is not None:
            hidden = self.res_unit(layer.residual_layer1, residual, extra=hidden)
        else:   # the first fusion layer: the module graph never calls its residual_layer1 either
            self._note(layer.residual_layer1.convolution1, "not run (the first fusion layer has no residual input)")
            self._note(layer.residual_layer1.convolution2, "not run (the first fusion layer has no residual input)")
        hidden = self.res_unit(layer.residual_layer2, hidden)
        rows = self._rows(hidden)
        if layer.use_deconv:
            B, h, w, _ = rows.shape
            route = "vd3d_gemm_x3 (deconv and projection composed) + vd3d_depth_to_space_bias_nhwc_f32"
            self._note(layer.deconv, route)
            self._note(layer.projection, route)
            return self._ct[id(layer)](rows, B, h, w)
        return self.conv1x1(layer.projection, rows).permute(0, 3, 1, 2)

    def fusion_forward(self, hidden_states):
        stage = self.pipe.model.fusion_stage
        if stage.num_layers != len(hidden_states):
            raise ValueError(f"num_layers={stage.num_layers} in DepthProFeatureFusionStage does not match len(hidden_states)={len(hidden_states)}")
        fused, outs = None, []
        for hs, layer in zip(hidden_states[:-1], stage.intermediate):
            fused = self.fusion_layer(layer, hs) if fused is None else self.fusion_layer(layer, fused, hs)
            outs.append(fused)
        outs.append(self.fusion_layer(stage.final, fused, hidden_states[-1]))
        return outs

    def head_forward(self, hidden_states):
        R, hl = self.R, self.pipe.model.head.layers
        y0 = self.conv_epi(hl[0], hidden_states, "bias")
        w3, b3 = self._head_tail()
        sw = decoder_switch("VD3D_DEPTHPRO_HEAD_POLY")
        if sw is not False and self.mode in (DECODER_HEAD_POLY_BUILT if sw else DECODER_HEAD_POLY_ROUTED):
            for lay in (hl[1], hl[2], hl[4]):
                self._note(lay, "vd3d_depthpro_head")
            return R.depthpro_head(y0, self._head_poly, self._head_T, w3, b3, self.mode)
        why = "VD3D_DEPTHPRO_HEAD_POLY=0" if sw is False else "not routed: profiles/r29_depth_pro_decoder.md"
        fine = self.deconv(hl[1], self._rows(y0))
        y = self.tile(hl[2], fine)
        self._note(hl[2], f"vd3d_conv3x3_{R.TILE_CONVS[self.mode, 1]} ({why})")
        self._note(hl[4], "vd3d_dpt_head_tail_f32")
        return R.dpt_head_tail(y, self._head_b2, w3, b3, 1.0)

    def conv_im2col(self, cv, rows, relu):
        """A k x k convolution as vd3d_im2col_nhwc_f32 + vd3d_gemm_x3 with the bias: NHWC rows in, NHWC rows out."""
        img, npad, bias = self._im2col[id(cv)]
        p, k = cv.padding[0], cv.kernel_size[0]
        if k in IM2COL_KERNELS:
            cols = self.R.im2col(rows, k, cv.stride[0], (p, p, p, p))
            self._note(cv, "vd3d_im2col_nhwc_f32 + vd3d_gemm_x3")
        else:   # decoder_scope: the window is the whole map, without padding -- the map's NHWC storage IS the one im2col row (ky, kx, c), zero-padded to 16 n
            B = rows.shape[0]
            cols = rows.reshape(B, 1, 1, -1)
            cols = F.pad(cols, (0, (-cols.shape[-1]) % 16)).contiguous()
            self._note(cv, "vd3d_gemm_x3 (the window is the whole map: its NHWC storage is the im2col row)")
        y = self.R.linear_x3(cols, img, npad, bias, mode=self.mode)
        y = y[..., :cv.out_channels]
        return (torch.relu(y) if relu else y).contiguous()

    def fov_forward(self, pixel_values, global_features):
        fov, R = self.pipe.model.fov_model, self.R
        feats = fov.fov_encoder(pixel_values)
        if self._fov_s2 is not None:
            g = R.conv3x3_tile(global_features.contiguous(memory_format=torch.channels_last), self._fov_s2, fov.conv.out_channels, self.mode, 2)
            g = self._rows(R.bias_act(g, fov.conv.bias, relu=True))
            self._note(fov.conv, f"vd3d_conv3x3_{R.TILE_CONVS[self.mode, 2]} + vd3d_nhwc_bias_act_f32")
        else:
            g = self.conv_im2col(fov.conv, self._rows(global_features), True)
        x = self._rows(feats) + g
        if tuple(x.shape[1:3]) != (fov.head.out_size, fov.head.out_size):
            raise NotImplementedError(f"decoder={self.mode!r}: the field-of-view head would resize {tuple(x.shape[1:3])} features to {fov.head.out_size} x {fov.head.out_size} -- "
                                      "only the identity is built")
        convs = [c for c in fov.head.layers if isinstance(c, torch.nn.Conv2d)]
        for i, cv in enumerate(convs):
            x = self.conv_im2col(cv, x, i + 1 < len(convs))
        return x.flatten()
