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

from . import depth_pro, zoedepth
# the names below that this module does not use itself are re-exported: tests, tools and bench.py import them from here (tests/test_depth_layout.py lists them)
from .depth_compose import (HEAD_CONV2_GATHER_BUILT, HEAD_CONV2_GATHER_ROUTED, HEAD_UPCONV_BUILT, bit_standardized_weight, conv_transpose_gemm_weight,  # noqa: F401
                            depth_to_u8, dpt_resize_target, head_conv2_compose, head_upconv_compose, im2col_gemm_weight, neck_poly_compose, neck_poly_offsets,
                            patch_embedding_gemm_weight, same_padding)
from .depth_routes import (CONV_X2_MIN_TILES, CONV_X3_MIN_TILES, _SWITCHES, _BitPrefix, _ConvRouter, _DaHead, _DaReassemble, _DptHead, _FusionStage,  # noqa: F401
                           _HybridEmbeddings, _memoise, _PatchEmbedding, _PerVersion, _RowReassemble, _switch, bit_prefix_plan, fuse_dinov2_layers,
                           fuse_dpt_vit_layers, patch_embedding_rows)
from .vit_blocks import head_geometry_ok

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
    # Intel/zoedepth-nyu-kitti (ZoeDepthForDepthEstimation): BEiT-L/16 at 384 behind a DPT neck, a relative head and the two-domain metric bin head; zoedepth.py states
    # the geometry (as far as it is known here), the processor and the composed head
    "zoedepth-nyu-kitti": dict(arch="zoedepth", hidden=1024, layers=24, heads=16, fusion=256),
}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
# image-processor constants (preprocessor_config.json of the checkpoints): DA = DPTImageProcessor(size 518, keep_aspect_ratio,
# ensure_multiple_of 14, bicubic, ImageNet mean/std); DPT-Large = 384 x 384, no aspect keeping, mean = std = 0.5
PROCESSORS = {
    "da": dict(size=(518, 518), keep_aspect_ratio=True, multiple=14, mean=IMAGENET_MEAN, std=IMAGENET_STD),
    "dpt": dict(size=(384, 384), keep_aspect_ratio=False, multiple=1, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)),
    # DepthProImageProcessor: 1536 x 1536, no aspect keeping, BILINEAR (PIL resample 2) without antialias AFTER rescale + normalise, mean = std = 0.5
    "depth_pro": dict(size=(1536, 1536), keep_aspect_ratio=False, multiple=1, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), resample=2),
    # ZoeDepthImageProcessor: rescale, REFLECT padding by int(sqrt(side / 2) * 3), BILINEAR (PIL resample 2) with align_corners=True to 384 x 512 keeping the aspect
    # ratio, normalise last, mean = std = 0.5.  multiple 32: the checkpoint's value as far as it is known here, unconfirmed (the class default is 1 / 32)
    "zoedepth": dict(zoedepth.PROCESSOR),
}


def build_config(name: str):
    from transformers import DepthAnythingConfig, Dinov2Config
    z = MODEL_ZOO[name]
    if z["arch"] == "depth_pro":
        return depth_pro.config()
    if z["arch"] == "zoedepth":
        return zoedepth.config(name)
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
        ZoeDepth (``"zoedepth-nyu-kitti"``, ``ZoeDepthForDepthEstimation``: Intel/zoedepth-nyu-kitti; ``zoedepth.py`` states the geometry as far as it is known here):
        ``__call__``, ``infer_bgr_u8``, ``depth_frames_u8`` and ``at_inference_size`` give what ``pipeline("depth-estimation")`` gives -- ZoeDepthImageProcessor's own order
        (rescale, REFLECT padding by int(sqrt(side / 2) * 3), a bilinear resize with align_corners=True to 384 x 512 keeping the aspect ratio at a multiple of 32, normalise
        last: ``front_end="float"``; ``"pil"`` is refused by name), the model, and the processor's post-process at the size the pipeline saw: the bicubic resize to that
        size plus its padding, with the padding cut off.  With a renderer both ends are one launch each (``vd3d_zoedepth_preprocess_u8`` for uint8 frames without an
        ``inference_size`` -- otherwise ATen operators, ``front_end_route`` reads "statement"; ``vd3d_zoedepth_post_f32``); on the CPU the same arithmetic runs in ATen.
        ``raw=True`` returns the model-resolution prediction, padding included.  The BEiT backbone, the neck and the relative head run their stock float32 graph
        (``gemm=`` / ``conv=`` / ``self_contained=True`` / ``encoders=`` / ``decoder=``, tiled depth and ``flops_per_frame`` refuse the model by name).  The metric bin
        head runs on two own kernels in float32 with a renderer (``zoedepth.MetricHeadRoute``: ``vd3d_zoedepth_attractor_f32`` per attractor layer and
        ``vd3d_zoedepth_bins_f32`` for the log-binomial tail, no [B, 64, H, W] tensor, no ``.item()`` on the multi-head model's domain vote); ``pipe.zoe_routes`` says
        which form runs, ``pipe.zoe_domain`` holds the vote's device index of the last forward, ``VD3D_ZOE_HEAD=0`` puts the stock head back, and whatever
        ``zoedepth.head_scope`` does not take (``bin_centers_type="normed"``, ...) keeps the stock head with the reason in ``zoe_routes``.  The multi-head model votes
        over the BATCH (``domain_logits.sum(0)``), as the module does: a frame's prediction depends on the batch it is in, by the model's design.
        ``encoders`` (DepthPro only; float32 + ``renderer``): ``None`` (default) -- the stock graph, as above.  ``"bf16x3"`` / ``"fp16x2"`` -- OPT-IN: from ``pixel_values``
        to the inputs of ``DepthProNeck`` (and to the input of the field-of-view model's convolution) no vendor-library call is made: the patch pyramid is one launch
        (``vd3d_depthpro_patches_f32``), the patch embeddings are ``vd3d_patchify_f32`` + ``vd3d_gemm_x3``, every ``Dinov2Layer`` of the patch, image and
        field-of-view encoders is a ``vit_blocks._split_block`` in the named arithmetic, the final LayerNorms are ``vd3d_add_layernorm``, the field-of-view ``neck`` Linear is
        ``vd3d_gemm_x3`` and every ``reconstruct_feature_maps`` is ``vd3d_depthpro_merge_f32`` (``depth_pro.EncoderRoutes``).  The neck, the fusion stage, the head
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
        ``depth_routes._RowReassemble``) and DPT-Hybrid in its published geometry (``"dpt-hybrid-midas"``, MiDaS 3.0: ViT-B/16 behind a BiT ResNet-50 prefix;
        ``_split_scope`` states the geometry; ``depth_routes._HybridEmbeddings`` what runs where: the prefix stays the module graph on the float32 library unless
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
        On top of the two split modes every remaining convolution takes a kernel of the mode's pair -- the patch embedding (``_PatchEmbedding``), the reassemble
        stage (``_RowReassemble``, DINOv2's and DPT's alike), ``neck.convs``, the fusion stage and the head at every map size
        (``_ConvRouter``, ``_DaHead``: a metric head's ``Sigmoid() * max_depth`` runs inside the tail launch), DPT-Hybrid's BiT prefix (``_BitPrefix``) -- and a module
        the mode cannot route is refused by name, never handed to a library.  ``conv_routes`` names every routed module and holds no ``"library"`` value; with the
        fp16x2 pair its labels read ``("fp16x2", "self-contained...")`` and the mode's range contract holds in front of every route.  The library selection is skipped:
        TunableOp is not enabled, ``torch.backends.cudnn.benchmark`` is not touched, ``tuned_gemm`` / ``miopen_find`` read False.  Per output element every kernel sums
        in one fixed order and nothing is split along K, so a frame's prediction does not depend on the batch it is in or on the ROCm release's solution tables."""
        # 1. the keywords: refusals that touch nothing
        if gemm not in ("f32", "bf16x3", "fp16x2"):
            raise ValueError("gemm must be 'f32', 'bf16x3' or 'fp16x2'")
        if conv not in (None, "bf16x3", "fp16x2"):
            raise ValueError("conv must be None, 'bf16x3' or 'fp16x2'")
        if getattr(renderer, "_private", False):
            # nothing here calls ordered_after(): the renderer's launches and the network's ATen operators are ordered by sharing one stream
            raise ValueError("DepthPipe needs a renderer on the SAME stream as the network: Renderer(private_stream=True) enqueues on a stream of its own, "
                             "pass a default Renderer (it follows torch's current stream)")
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
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("DepthPipe runs in float32 (reference precision) or bfloat16")
        self.name, self.device, self.dtype = name, torch.device(device), dtype
        self.encoders, self.encoders_resize = None, {}
        self.decoder, self.decoder_routes = None, {}
        self.front_end, self.front_end_route = front_end, None
        self.gemm, self.conv, self.self_contained = gemm, conv, bool(self_contained)
        self.conv_routes = {}
        self.tuned_gemm = self.miopen_find = False
        self._flop_count = None
        if self.device.type == "cuda" and not self.self_contained:   # self-contained: no library call to select for
            self._library_selection(tuned_gemm, miopen_find)
        # 2. the model, built or accepted, and the scope checks on its module graph as handed in: what a mode does not build is refused by name, before anything moves
        if model is None:
            cfg = build_config(name)
            if MODEL_ZOO[name]["arch"] == "depth_pro":
                from transformers import DepthProForDepthEstimation as Net
            elif MODEL_ZOO[name]["arch"] == "zoedepth":
                from transformers import ZoeDepthForDepthEstimation as Net
            elif MODEL_ZOO[name]["arch"] == "dpt":
                from transformers import DPTForDepthEstimation as Net
            else:
                from transformers import DepthAnythingForDepthEstimation as Net
            model = Net(cfg).eval()
            synthetic_weights_(model, seed)
            processor = processor or PROCESSORS[MODEL_ZOO[name]["arch"]]
        self.model = model
        self.arch = {"DepthAnythingForDepthEstimation": "da", "DepthProForDepthEstimation": "depth_pro", "ZoeDepthForDepthEstimation": "zoedepth"}.get(type(model).__name__, "generic")
        if self.arch == "depth_pro":
            if front_end == "pil":   # the processor is no Pillow resize: it normalises first and resizes the FLOAT image (torchvision, no antialias)
                raise NotImplementedError(f"front_end='pil': {name!r} (DepthProForDepthEstimation) -- DepthProImageProcessor rescales and normalises first and resizes the float "
                                          "tensor bilinearly without antialias; there is no 8-bit Pillow pass to reproduce, front_end='float' IS the processor's own order")
            if gemm != "f32" or self_contained:
                self._split_scope(fuse_backbone)
            if processor is None:
                processor = PROCESSORS["depth_pro"]
        if self.arch == "zoedepth":
            if front_end == "pil":   # the processor pads and resizes the rescaled FLOAT image (F.interpolate, align_corners=True)
                raise NotImplementedError(f"front_end='pil': {name!r} (ZoeDepthForDepthEstimation) -- ZoeDepthImageProcessor rescales, pads by reflection and resizes the float "
                                          "tensor bilinearly with align_corners=True; there is no 8-bit Pillow pass to reproduce, front_end='float' IS the processor's own order")
            if gemm != "f32" or self_contained:
                self._split_scope(fuse_backbone)
            if processor is None:
                processor = PROCESSORS["zoedepth"]
        if encoders is not None:
            enc_plan = depth_pro.encoders_scope(model, name, encoders, processor)
        if decoder is not None:
            depth_pro.decoder_scope(model, name, decoder, enc_plan["size"])
        if self.self_contained:
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
        # 3. the model on its device and the rewrites, in this order
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
                _PatchEmbedding(self, self.model.dpt.embeddings.patch_embeddings)
        elif scope == "dpt-hybrid":
            self.dpt_hybrid = True
            self._rewrite_dpt_vit()
            _HybridEmbeddings(self)
        if dino:
            # DINOv2 re-interpolates its position embedding (bicubic 37x37 -> patch grid) on EVERY forward; for a fixed frame size it is a constant, and ATen's bicubic
            # kernel loops the 384-1024 channels serially per output pixel (measured 2.9 ms per forward on MI355X, 14 % of the step): memoised per (height, width)
            _memoise(self.model.backbone.embeddings, "interpolate_pos_encoding", lambda t, height, width: (int(height), int(width), t.dtype, t.shape[1]))
            if fuse_backbone:
                fuse_dinov2_layers(self)
            if self.renderer is not None:
                self._patch_dpt_upsampling()
            if self.self_contained:
                _PatchEmbedding(self, self.model.backbone.embeddings.patch_embeddings)
        if self.arch == "zoedepth":
            self._zoe_table = zoedepth.rescale_table().to(self.device)
            with torch.no_grad():
                zoedepth.route_head(self)
        if encoders is not None:
            with torch.no_grad():
                depth_pro.EncoderRoutes(self, encoders, enc_plan)
            self.encoders = encoders
        if decoder is not None:
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
        (DPT / MiDaS 3.0 ...) runs its stock module graph behind the same protocol; a ZoeDepth checkpoint runs behind ITS processor (``resample: 2`` is accepted for
        that class -- and DepthPro -- only; ``zoedepth.preprocessor_from_json`` reads do_pad, keep_aspect_ratio, ensure_multiple_of, size, mean and std and refuses
        any other ZoeDepth processor by name) -- except that a plain-ViT DPT checkpoint
        (Intel/dpt-large) with ``gemm="bf16x3" / "fp16x2"`` and a renderer in ``kw`` gets the split-mode rewrite (``__init__``)."""
        from transformers import AutoModelForDepthEstimation
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path}: not a local checkpoint folder (this build environment has no network)")
        model = AutoModelForDepthEstimation.from_pretrained(path, local_files_only=True)
        pro = type(model).__name__ == "DepthProForDepthEstimation"
        if type(model).__name__ == "ZoeDepthForDepthEstimation":   # the one class whose processor is bilinear with align_corners=True behind a reflect padding
            pc = os.path.join(path, "preprocessor_config.json")
            proc = dict(PROCESSORS["zoedepth"])
            if os.path.exists(pc):
                with open(pc) as f:
                    proc = zoedepth.preprocessor_from_json(json.load(f))
            return cls(os.path.basename(os.path.normpath(path)), device=device, dtype=dtype, model=model, processor=proc, **kw)
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
        if self.arch == "zoedepth":   # (of the image the resize sees: the frame plus its reflect padding)
            return zoedepth.resize_target(h, w, self.proc["size"], self.proc["multiple"], self.proc["keep_aspect_ratio"])
        return dpt_resize_target(h, w, self.proc["size"], self.proc["multiple"], self.proc["keep_aspect_ratio"])

    def _count_conv(self, m, y):
        """flops_per_frame: a convolution module m that a rewrite runs without calling it adds, for its output y, what the counting hook would have added."""
        self._count_flops(2.0 * y.numel() / y.shape[0] * (m.in_channels // m.groups) * m.kernel_size[0] * m.kernel_size[1])

    def _count_flops(self, n: float):
        """flops_per_frame: ``n`` flops a rewrite executes outside any counted convolution module (the only two places that add to the count: this and _count_conv)."""
        if self._flop_count is not None:
            self._flop_count[0] += n

    def _patch_dpt_upsampling(self):
        """The DPT neck / head between the library convolutions (transformers DepthAnythingReassembleStage / PreActResidualLayer / FeatureFusionLayer /
        DepthEstimationHead; the module graphs are otherwise reproduced verbatim), as the objects of depth_routes.py: _ConvRouter (where each convolution runs, per mode),
        _FusionStage, the head (_DaHead | _DptHead) and the reassemble stage (_DaReassemble on the library path; _RowReassemble for the DINOv2 stage under
        self_contained=True and for DPT, which differ in the grid fall-back and the flop count alone).  The align_corners=True bilinear up-samplings run on
        vd3d_upsample_bilinear_nhwc.  Same function as the module graph up to float32 association (tests/test_hip_depth_e2e.py: 1e-4 of the range on the prediction,
        identical uint8 planes up to the stated bar).  VD3D_NECK_GLUE is read here, once: "0" is the A/B switch back to the module graph's own passes."""
        cr = _ConvRouter(self, self.dtype == torch.float32 and _switch("VD3D_NECK_GLUE"))
        if self.dpt_vit:
            _FusionStage(self, cr)
            _RowReassemble(self, self.model.neck.reassemble_stage.readout_projects, square_grid=True, count_executed=True)
            if cr.f32:   # (VD3D_NECK_GLUE=0 keeps the head's own module graph)
                _DptHead(self, cr)
            return
        _FusionStage(self, cr, _DaHead(self, cr).upconv)
        _RowReassemble(self) if self.self_contained else _DaReassemble(self, cr)

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
        if type(m).__name__ == "ZoeDepthForDepthEstimation":
            raise NotImplementedError(f"{tag}: {what} -- ZoeDepth runs its stock float32 graph between the own front end, metric bin head and post-process (gemm='f32'): "
                                      "BEiT's relative position bias has no input in vd3d_attention_x3 and the split-mode rewrite of its backbone, neck and relative head "
                                      "is not built -- nothing is substituted silently")
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
        # DPTViTEmbeddings re-interpolates its position embedding (bilinear, 24 x 24 -> patch grid) on every forward: a constant of the input size, like DINOv2's
        _memoise(self.model.dpt.embeddings, "_resize_pos_embed", lambda t, gh, gw, start_index=1: (int(gh), int(gw), t.dtype, int(start_index)))
        fuse_dpt_vit_layers(self)
        self._patch_dpt_upsampling()

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
        if self.arch == "zoedepth":
            return self._infer_zoedepth(frames_bgr, inference_size, raw, oH, oW)
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

    def _infer_zoedepth(self, frames_bgr, inference_size, raw, oH, oW):
        """infer_bgr_u8 for ZoeDepthForDepthEstimation: the processor (rescale, reflect padding, the align_corners=True bilinear resize, normalise), the model, and
        ZoeDepthImageProcessor.post_process_depth_estimation as the pipeline calls it, with the size it saw as ``source_sizes``: the bicubic resize of the prediction to
        that size plus its padding, with the padding cut off.  With a renderer the post-process is one launch (vd3d_zoedepth_post_f32) and, for uint8 frames without an
        inference size, so is the front end (vd3d_zoedepth_preprocess_u8: no padded image exists).  With an ``inference_size`` (the pre-resize hands the processor
        non-integer pixels) or non-uint8 frames the front end is zoedepth.preprocess_statement, the same arithmetic as ATen operators, and without a renderer so is
        the post-process (post_statement).  ``front_end_route`` ("kernel" | "statement") says which front end ran last.  ``raw``: the model-resolution prediction,
        padding included."""
        f, proc = frames_bgr.to(self.device), self.proc
        if self.renderer is not None and inference_size is None and f.dtype == torch.uint8:
            H, W = f.shape[1:3]
            ph, pw = zoedepth.pad_amounts(H, W) if proc.get("pad", True) else (0, 0)
            target = zoedepth.resize_target(H + 2 * ph, W + 2 * pw, proc["size"], proc["multiple"], proc["keep_aspect_ratio"])
            x = self.renderer.zoedepth_preprocess(f, (ph, pw), target, proc["mean"], proc["std"], self._zoe_table)
            self.front_end_route = "kernel"
        else:
            self.front_end_route = "statement"
            if inference_size is not None:   # hf_batch_safe_pipe: img.resize(inference_size, BICUBIC) first (:1113-1116), in its float statement as for every model
                f = F.interpolate(f.flip(-1).permute(0, 3, 1, 2).float(), size=(int(inference_size[1]), int(inference_size[0])), mode="bicubic", antialias=True,
                                  align_corners=False).clamp_(0, 255).permute(0, 2, 3, 1).flip(-1)
            x = zoedepth.preprocess_statement(f, proc)
            if self.device.type == "cuda":
                x = x.contiguous(memory_format=torch.channels_last)
        pred = self.model(pixel_values=x.to(self.dtype)).predicted_depth.float().contiguous()
        if raw:
            return pred
        if self.renderer is not None:
            return self.renderer.zoedepth_post(pred, oH, oW, zoedepth.pad_amounts(oH, oW) if proc.get("pad", True) else (0, 0))
        return zoedepth.post_statement(pred, oH, oW, proc.get("pad", True))

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
        if self.arch == "zoedepth" and model_call is None:
            raise NotImplementedError(f"tiled depth: {self.name!r} (ZoeDepthForDepthEstimation) -- the tile blend evaluates the pipeline's plain bicubic post-process of every "
                                      "tile; ZoeDepth's removes the processor's reflect padding -- not built")
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
        if self.arch == "zoedepth":
            raise NotImplementedError(f"flops_per_frame: {self.name!r} (ZoeDepthForDepthEstimation) -- the estimate is not built for the padded front end and the bin head")
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
