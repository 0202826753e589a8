"""Everything that replaces a module's ``forward`` for the DINOv2 / DPT families of DepthPipe (depth.py), and the helpers those replacements share with
depth_pro.py.  Every object takes the pipe and reads ``pipe.renderer`` / ``pipe.gemm`` when it is CONSTRUCTED (DepthPipe._patch_dpt_upsampling and its
neighbours), never earlier: tests put a CPU double in the renderer's place first.  Imports depth_compose and vit_blocks; knows neither depth.py nor depth_pro.py."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from .depth_compose import (HEAD_CONV2_GATHER_BUILT, HEAD_CONV2_GATHER_ROUTED, HEAD_UPCONV_BUILT, _is_conv, bit_standardized_weight, conv_transpose_gemm_weight,
                            head_conv2_compose, head_upconv_compose, im2col_gemm_weight, neck_poly_compose, neck_poly_offsets, patch_embedding_conv_ok,
                            patch_embedding_gemm_weight, same_padding)
from .vit_blocks import dinov2_operands, dpt_vit_operands, encoder_blocks, query_padding

_CL = torch.channels_last


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


class _DaReassemble:
    """Depth-Anything's reassemble stage on the library path: the token tensor goes to the 1x1 projection as a channels_last VIEW ([B,T,C] minus CLS is NHWC storage)
    instead of a NCHW copy that MIOpen converts back; the up-scaling stages 0 / 1 hand their coarse map to neck.convs[i] where _PolyRoute runs (``pending``)."""

    def __init__(self, pipe, cr):
        neck, self.stage = pipe.model.neck, pipe.model.neck.reassemble_stage
        on = pipe.gemm == "f32" and cr.f32 and pipe.device.type == "cuda"
        self.poly = {i: _PolyRoute(cr, self.stage.layers[i].resize, neck.convs[i]) for i in (0, 1)
                     if on and i < len(self.stage.layers) and i < len(neck.convs) and isinstance(self.stage.layers[i].resize, torch.nn.ConvTranspose2d)}
        self.stage.forward = self.forward

    def forward(self, hidden_states, patch_height=None, patch_width=None):
        stage, poly, out = self.stage, self.poly, []
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


class _RowReassemble:
    """A reassemble stage whose 1 x 1 projections are GEMMs over the token rows: the DINOv2 stage under self_contained=True, and DPT-Large's / DPT-Hybrid's with and
    without it.  Per hook: the readout where the stage has one (``readouts`` = its readout_projects: GELU(Linear_2C->C(cat(tokens, CLS))) as one linear_x3 with the
    GELU epilogue over the [B, T-1, 2C] rows, or linear_x3 and the module's own activation); the projection as linear_x3 with its bias ([B, T-1, C_i] is NHWC
    storage); the resize -- self_contained=True: ``resize_rule``, every route recorded in conv_routes, no library call; without it a ConvTranspose2d (kernel ==
    stride, _split_scope has checked) is a _ConvTransposeGemm and anything else the module's own call.  Hooks in the stage's neck_ignore_stages (DPT-Hybrid's BiT
    maps) pass through.  The two families differ in two ways, on purpose:
      * ``square_grid``: DPT falls back to the stock stage's square grid where the caller names none; DINOv2 requires patch_height / patch_width;
      * ``count_executed``: what a transposed convolution adds to flops_per_frame -- DPT the EXECUTED GEMM (P x s s C_out x C_in), the DINOv2 stage the module
        hook's formula, so that the figure equals the library mode's.  (The readout Linear is not a convolution: not counted, as in the stock graph.)"""

    def __init__(self, pipe, readouts=None, square_grid=False, count_executed=False):
        self.pipe, self.square_grid, self.count_executed = pipe, square_grid, count_executed
        R, gm, sc, names = pipe.renderer, pipe.gemm, pipe.self_contained, pipe._names
        stage, self.hooks = pipe.model.neck.reassemble_stage, []
        for i, lay in enumerate(stage.layers):
            if i in getattr(stage, "neck_ignore_stages", ()):
                self.hooks.append(None)
                continue
            pm, rz, hk = lay.projection, lay.resize, {}
            if sc and (not _is_conv(pm, 1, 1, 0) or pm.in_channels % 16):
                raise NotImplementedError(f"self_contained=True: {names[id(pm)]} is not a 1 x 1 convolution with C_in a multiple of 16 -- not built")
            if readouts is not None:
                rl, act = readouts[i][0], readouts[i][1]
                gelu = isinstance(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none" or type(act).__name__ == "GELUActivation"
                hk["readout"] = (R.gemm_x3_pack(rl.weight, gm), rl.out_features, rl.bias, gelu, act)
            hk.update(pm=pm, rz=rz, proj=R.gemm_x3_pack(pm.weight.reshape(pm.weight.shape[0], -1), gm))
            hk["kind"], hk["operand"] = (self.resize_rule(rz, names[id(rz)]) if sc else ("ct", _ConvTransposeGemm(R, rz, gm)) if isinstance(rz, torch.nn.ConvTranspose2d)
                                         else ("module", None))
            self.hooks.append(hk)
        stage.forward = self.forward

    def resize_rule(self, rz, name):
        """The resize module ``rz`` (``name``) of a reassemble layer under self_contained=True -> (kind, operand): ("ct", _ConvTransposeGemm) for a ConvTranspose2d with a
        square kernel == stride, no padding and C_in % 16; ("s2", weight image) for a Conv2d 3 x 3 / stride 2 / padding 1 the stride-2 tile convolution of the mode
        builds (C_in % 16, C_out % 128 up to 1024); ("identity", None).  Anything else is refused by name.  One rule for the DINOv2 stage and DPT's."""
        R, gm = self.pipe.renderer, self.pipe.gemm
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

    def count_rows(self, t, n):   # flops_per_frame: a GEMM of t's rows to n columns that bypasses the module hooks (for a 1 x 1 convolution: the hook's formula)
        self.pipe._count_flops(2.0 * t.numel() / t.shape[0] * n)

    def resize(self, hk, rows, B, gh, gw):
        """The hook's resize on the projected token rows [B, gh gw, C] (NHWC storage of the B x gh x gw map) -> the channels_last [B, C', h', w'] map, counted, recorded."""
        pipe, R, gm, names = self.pipe, self.pipe.renderer, self.pipe.gemm, self.pipe._names
        kind, operand, rz = hk["kind"], hk["operand"], hk["rz"]
        if kind == "ct":
            if pipe.self_contained:
                pipe.conv_routes[names[id(rz)]] = (gm, "self-contained: vd3d_gemm_x3 + vd3d_depth_to_space_bias_nhwc_f32")
            x = operand(rows, B, gh, gw)
            self.count_rows(rows, operand.n) if self.count_executed else pipe._count_conv(rz, x)   # the executed GEMM | the module hook's formula
            return x
        x = rows.view(B, gh, gw, rows.shape[-1]).permute(0, 3, 1, 2)   # NHWC storage, NCHW view: channels_last
        if kind == "module":
            return rz(x)   # identity, or the library's 3 x 3 stride-2 convolution (its hook counts it)
        if kind == "s2":
            x = R.conv3x3_tile(x, operand, rz.out_channels, gm, 2)
            if rz.bias is not None:
                x = R.bias_act(x, rz.bias)
            pipe.conv_routes[names[id(rz)]] = (gm, "self-contained: vd3d_conv3x3_" + R.TILE_CONVS[gm, 2])
            pipe._count_conv(rz, x)   # what the module's hook adds without the keyword
        return x

    def forward(self, hidden_states, patch_height=None, patch_width=None):
        pipe, R, gm, out = self.pipe, self.pipe.renderer, self.pipe.gemm, []
        for hk, hs in zip(self.hooks, hidden_states):
            if hk is None:
                out.append(hs)
                continue
            B, T, d = hs.shape
            if patch_height is None or patch_width is None:
                if not self.square_grid:
                    raise ValueError("the DINOv2 reassemble stage needs the patch grid")
                patch_height = patch_width = int((T - 1) ** 0.5)   # the stock stage's square grid
            gh, gw = int(patch_height), int(patch_width)
            if gh * gw != T - 1:
                raise ValueError(f"{T - 1} patch tokens do not form a {gh} x {gw} grid")
            if "readout" in hk:
                img, n, bias, gelu, act = hk["readout"]
                x = torch.cat((hs[:, 1:], hs[:, :1].expand(B, T - 1, d)), -1)
                x = R.linear_x3(x, img, n, bias, gelu=True, mode=gm) if gelu else act(R.linear_x3(x, img, n, bias, mode=gm))
            else:
                x = hs[:, 1:].contiguous()
            pm = hk["pm"]
            self.count_rows(x, pm.out_channels)
            x = R.linear_x3(x, hk["proj"], pm.out_channels, pm.bias, mode=gm)   # [B, T-1, C_i]: NHWC storage
            if pipe.self_contained:
                pipe.conv_routes[pipe._names[id(pm)]] = (gm, "self-contained: vd3d_gemm_x3 over the token rows")
            out.append(self.resize(hk, x, B, gh, gw))
        return out


class _DptHead:
    """DPT's head (split modes, float32 glue on): _ConvRouter.head_tail3 with scale 1 and the head's nn.Upsample(x 2) size (conv2 on vd3d_conv3x3_x2 in fp16x2 where
    its size rule allows, on the tile convolution with ``conv=``)."""

    def __init__(self, pipe, cr):
        self.cr, self.in_index = cr, pipe.model.config.head_in_index
        self.conv1, _, self.conv2, _, conv3, _ = list(pipe.model.head.head)
        self.tail = _head_tail_operands(conv3)
        pipe.model.head.forward = self.forward

    def forward(self, hidden_states):
        x = hidden_states[self.in_index].contiguous(memory_format=_CL)
        size = (2 * x.shape[2], 2 * x.shape[3])   # nn.Upsample(scale_factor=2, align_corners=True)
        return self.cr.head_tail3(self.cr.conv_nb(self.conv1, x), self.conv1, self.conv2, size, self.tail, 1.0)


class _PatchEmbedding:
    """Self-contained: the patch-embedding module ``pe`` (Dinov2PatchEmbeddings, DPTViTPatchEmbeddings: ``projection`` = Conv2d(3, C, kernel_size=p, stride=p), whose
    map the module flattens and transposes) as vd3d_patchify_f32 + vd3d_gemm_x3 on the weight reshaped to [C, 3 p^2] and zero-padded to the GEMM's K unit
    (p = 14: 588 -> 592; p = 16: 768, no padding), with its bias: [B, T-1, C] directly.  CLS, the cached position embedding and the final LayerNorm stay ATen
    element-wise / native kernels."""

    def __init__(self, pipe, pe):
        self.pipe, self.m, self.name = pipe, pe.projection, pipe._names[id(pe.projection)]
        if not patch_embedding_conv_ok(self.m):
            raise NotImplementedError(f"self_contained=True: {self.name}: a patch embedding other than Conv2d(3, C, kernel_size=p, stride=p), p <= 64 -- not built")
        self.rows = patch_embedding_rows(pipe.renderer, self.m, pipe.gemm)
        pe.forward = self.forward

    def forward(self, pixel_values):
        if pixel_values.dtype != torch.float32 or pixel_values.shape[1] != 3:
            raise NotImplementedError("self_contained=True: the patch embedding takes a float32 [B, 3, th, tw] image")
        y = self.rows(pixel_values.contiguous(memory_format=_CL))   # what depth_preprocess hands over is taken as it is
        self.pipe.conv_routes[self.name] = (self.pipe.gemm, "self-contained: vd3d_patchify_f32 + vd3d_gemm_x3")
        self.pipe._count_conv(self.m, y)   # the bypassed Conv2d: 2 (T - 1) C 3 p^2
        return y


class _HybridEmbeddings:
    """DPT-Hybrid's embeddings (DPTViTHybridEmbeddings; _split_scope has accepted the model) in the split modes: the 1 x 1 projection of the BiT stage-3 map
    (1024 -> hidden) as vd3d_gemm_x3 over its pixel rows, with its bias -- [B, gh gw, hidden] directly, no flatten / transpose copy; CLS and the memoised
    position embedding stay ATen element-wise kernels.  The BiT prefix in front of it: without ``self_contained`` the module graph on the float32 library
    (conv_routes says so for every convolution and normalisation of it, by module name); with it _BitPrefix, on own kernels.  The stage-1 / stage-2 maps go
    on as channels_last [B, C, h, w] tensors: hooks 0 / 1 of the reassemble stage."""

    def __init__(self, pipe):
        from transformers.models.dpt.modeling_dpt import BaseModelOutputWithIntermediateActivations
        self.pipe, self.Out, self.emb = pipe, BaseModelOutputWithIntermediateActivations, pipe.model.dpt.embeddings
        names, pm, bb = pipe._names, self.emb.projection, self.emb.backbone
        if not _is_conv(pm, 1, 1, 0) or pm.in_channels % 16:
            raise NotImplementedError(f"gemm={pipe.gemm!r}: {names[id(pm)]} is not a 1 x 1 convolution with C_in a multiple of 16 -- not built")
        self.img = pipe.renderer.gemm_x3_pack(pm.weight.reshape(pm.out_channels, pm.in_channels), pipe.gemm)
        self.prefix = _BitPrefix(pipe, bb, bit_prefix_plan(bb, names), names) if pipe.self_contained else None
        self.lib_names = [names[id(m)] for m in bb.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.GroupNorm))]
        self.emb.forward = self.forward

    def forward(self, pixel_values, interpolate_pos_encoding=False):
        pipe, emb, pm, gm = self.pipe, self.emb, self.emb.projection, self.pipe.gemm
        B, C, H, W = pixel_values.shape
        if C != emb.num_channels:
            raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the configuration.")
        if not interpolate_pos_encoding and (H != emb.image_size[0] or W != emb.image_size[1]):
            raise ValueError(f"Input image size ({H}*{W}) doesn't match model ({emb.image_size[0]}*{emb.image_size[1]}).")
        pos = emb._resize_pos_embed(emb.position_embeddings, H // emb.patch_size, W // emb.patch_size)
        if self.prefix is not None:
            f1, f2, f3 = self.prefix(pixel_values)
            hooks = [f1.permute(0, 3, 1, 2), f2.permute(0, 3, 1, 2)]
        else:
            maps = emb.backbone(pixel_values).feature_maps
            for n in self.lib_names:
                pipe.conv_routes[n] = ("library", "the BiT prefix stays the module graph without self_contained=True")
            hooks, f3 = [maps[i] for i in emb.residual_feature_map_index], maps[-1].permute(0, 2, 3, 1).contiguous()
        tok = pipe.renderer.linear_x3(f3.reshape(B, f3.shape[1] * f3.shape[2], f3.shape[3]), self.img, pm.out_channels, pm.bias, mode=gm)
        pipe.conv_routes[pipe._names[id(pm)]] = (gm, ("self-contained: " if self.prefix is not None else "") + "vd3d_gemm_x3 over the pixel rows")
        pipe._count_conv(pm, tok)   # the bypassed Conv2d
        x = torch.cat((emb.cls_token.expand(B, -1, -1), tok), dim=1) + pos
        return self.Out(last_hidden_states=x, intermediate_activations=hooks)


@torch.no_grad()
def fuse_dinov2_layers(pipe):
    """Inference-only rewrite of every Dinov2Layer of the backbone (same math, fewer launches): q/k/v projections as ONE GEMM (N = 3*hidden), LayerScale folded into
    the output-projection / fc2 weights (lambda * (xW^T + b) == x(lambda*W)^T + lambda*b), the attention called directly (float32 with a renderer: vd3d_attention_f32;
    otherwise SDPA).  Per layer: 4 GEMMs + attention + 2 LN + GELU + 2 adds instead of 6 GEMMs + 13 smaller kernels.  The block is ``vit_blocks.encoder_blocks``."""
    bb = pipe.model.backbone
    # query padding is the library back-end's: the split modes are float32 only (the constructor refuses anything else) and the hook pads bf16 alone
    pad_state = query_padding(bb.embeddings, bb.layernorm) if pipe.device.type == "cuda" and pipe.gemm == "f32" else None
    layers = list(bb.encoder.layer)
    for layer, blk in zip(layers, encoder_blocks(pipe.renderer, [dinov2_operands(lay) for lay in layers], pipe.gemm, pad_state=pad_state)):
        layer.forward = blk


@torch.no_grad()
def fuse_dpt_vit_layers(pipe):
    """Every DPTViTLayer (ViT-L/16 of DPT-Large) as a ``vit_blocks._split_block`` -- the same rewrite as fuse_dinov2_layers' split mode, on ``dpt_vit_operands``.
    The encoder collects each layer's return value at backbone_out_indices: the residual stream, as in the stock graph."""
    layers = list(pipe.model.dpt.encoder.layer)
    for layer, blk in zip(layers, encoder_blocks(pipe.renderer, [dpt_vit_operands(lay) for lay in layers], pipe.gemm)):
        layer.forward = blk
