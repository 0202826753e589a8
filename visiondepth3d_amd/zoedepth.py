"""ZoeDepth (``Intel/zoedepth-nyu-kitti``, ``ZoeDepthForDepthEstimation``) behind DepthPipe: the published geometry; the image processor's two ends stated in torch
(``preprocess_statement``, ``post_statement``: what vd3d_zoedepth_preprocess_u8 / vd3d_zoedepth_post_f32 are held to, and what runs where there is no renderer); the
metric bin head in its composed form (``head_statement`` with ``attractor_statement`` and ``bins_statement``: what vd3d_zoedepth_attractor_f32 and
vd3d_zoedepth_bins_f32 compute); the scope check ``head_scope`` and the route ``MetricHeadRoute`` that puts the head on those two kernels.

The network itself -- the BEiT backbone, the neck, the relative head -- runs its stock float32 module graph: BEiT's relative position bias has no input in the
split kernels, so ``gemm=`` / ``conv=`` / ``self_contained=True`` refuse the model by name.

Line numbers are those of the installed transformers: ``models/zoedepth/modeling_zoedepth.py`` (M) and ``models/zoedepth/image_processing_pil_zoedepth.py`` (P).

The geometry below is the published one AS FAR AS IT IS KNOWN HERE: no copy of the checkpoint's config.json or preprocessor_config.json was at hand when this was
written, so nothing has confirmed it against the files (in particular ``ensure_multiple_of`` 32).  A checkpoint loads with whatever its own files state
(``DepthPipe.from_pretrained``).

The composed head.  ZoeDepthConditionalLogBinomialSoftmax starts with a 1 x 1 convolution of cat(last, up(e)): last is the relative head's 32-channel map (33 with
the relative depth in the single-head model), up(e) the align_corners=True up-sampling of the last bin embedding.  A 1 x 1 convolution and a bilinear up-sampling
commute, so W1 . cat(last, up(e)) = W1_last . last + up(W1_e . e): the 128-channel embedding is projected on the COARSE map and only Ch = 40 / 80 channels are
sampled per fine pixel; the 64 bin centres are sampled per fine pixel as well and nothing of size [B, 64, H, W] is ever written.  ``inv_attractor`` is called with
its defaults (alpha = 300, gamma = 2: M:551; ``config.attractor_alpha`` / ``attractor_gamma`` are never passed) and the statement follows the code.
``log_binom(k_minus_1, k_idx)`` (M:376-380, 420) is evaluated on integer buffers plus a Python float, so it is float32 whatever the model's dtype: the table is taken
as the module computes it, never recomputed."""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn.functional as F

# BEiT-L/16 at 384 with relative position bias and no absolute embeddings; hooks after layers 6 / 12 / 18 / 24
BACKBONE = dict(model_type="beit", image_size=384, patch_size=16, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                use_relative_position_bias=True, use_absolute_position_embeddings=False, reshape_hidden_states=False,
                out_features=["stage6", "stage12", "stage18", "stage24"])
GEOMETRY = dict(neck_hidden_sizes=[256, 512, 1024, 1024], fusion_hidden_size=256, bottleneck_features=256, num_relative_features=32, bin_embedding_dim=128,
                num_attractors=[16, 8, 4, 1], bin_centers_type="softplus", attractor_kind="mean", readout_type="project", reassemble_factors=[4, 2, 1, 0.5])
BIN_CONFIGURATIONS = {
    "zoedepth-nyu-kitti": [dict(name="nyu", n_bins=64, min_depth=1e-3, max_depth=10.0), dict(name="kitti", n_bins=64, min_depth=1e-3, max_depth=80.0)],
    "zoedepth-nyu": [dict(n_bins=64, min_depth=1e-3, max_depth=10.0)],
    "zoedepth-kitti": [dict(n_bins=64, min_depth=1e-3, max_depth=80.0)],
}
PATCH_TRANSFORMER = dict(num_patch_transformer_layers=4, patch_transformer_hidden_size=128, patch_transformer_intermediate_size=1024,
                         patch_transformer_num_attention_heads=4)
# ZoeDepthImageProcessor (P:113-124): 384 x 512, keep_aspect_ratio, PIL resample 2 (bilinear, align_corners=True), reflect padding, mean = std = 0.5.  multiple: 32 is
# the checkpoint's value as far as it is known here (unconfirmed); the CLASS default is 1 / 32 (sic), which is what a preprocessor_config.json without the key gives
PROCESSOR = dict(size=(384, 512), keep_aspect_ratio=True, multiple=32, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), resample=2, pad=True)
CLASS_DEFAULT_MULTIPLE = 1 / 32

# what the two head kernels take (include/vd3d.h)
KERNEL_LAST, KERNEL_MAX_HIDDEN, KERNEL_MAX_BINS, KERNEL_MAX_ATTRACTORS = 32, 128, 256, 16

# The A/B switch of the head route (an environment variable, read at construction; depth_routes._SWITCHES' convention): unset, HEAD_ROUTED decides; "1" routes the head
# on the two kernels; "0" puts the stock metric head back.
ZOE_SWITCHES = ("VD3D_ZOE_HEAD",)
HEAD_ROUTED = True   # profiles/r32_zoedepth.md


def zoe_switch(name: str):
    """The switch ``name`` of ZOE_SWITCHES as it stands in the environment NOW: False for "0", True for "1", None (HEAD_ROUTED decides) otherwise."""
    if name not in ZOE_SWITCHES:
        raise KeyError(name)
    return {"0": False, "1": True}.get(os.environ.get(name))


def config(name: str = "zoedepth-nyu-kitti", **over):
    """ZoeDepthConfig of the published geometry (UNCONFIRMED against the checkpoint's config.json, see the module docstring): BEiT-L/16 at 384 with relative position
    bias, stages 6 / 12 / 18 / 24, neck 256 / 512 / 1024 / 1024, fusion = bottleneck 256, 32 relative features, bin embedding 128, attractors 16 / 8 / 4 / 1,
    softplus bin centres; ``"zoedepth-nyu-kitti"`` has two bin configurations (nyu 1e-3 .. 10, kitti 1e-3 .. 80, 64 bins each) and the patch transformer (4 layers,
    128 / 1024, 4 heads).  ``over`` replaces top-level fields."""
    from transformers import ZoeDepthConfig
    bins = [dict(c) for c in BIN_CONFIGURATIONS[name]]
    kw = dict(GEOMETRY, backbone_config=dict(BACKBONE), bin_configurations=bins)
    if len(bins) > 1:
        kw.update(PATCH_TRANSFORMER)
    kw.update(over)
    return ZoeDepthConfig(**kw)


# ---------------------------------------------------------------------------------------------------------------- the image processor
def resize_target(h: int, w: int, size=(384, 512), multiple=32, keep_aspect_ratio: bool = True):
    """get_resize_output_image_size (P:72-108) for any positive multiple, fractions included: "scale as little as possible", then np.round(v / m) * m, truncated."""
    sh, sw = size[0] / h, size[1] / w
    if keep_aspect_ratio:
        if abs(1 - sw) < abs(1 - sh):
            sh = sw
        else:
            sw = sh
    return int((np.round(sh * h / multiple) * multiple).astype(int)), int((np.round(sw * w / multiple) * multiple).astype(int))


def pad_amounts(h: int, w: int):
    """pad_image's reflect padding per side (P:192-193; the post-process removes the same, P:314-315): int(sqrt(side / 2) * 3)."""
    return int(np.sqrt(h / 2) * 3), int(np.sqrt(w / 2) * 3)


def rescale_table() -> torch.Tensor:
    """The class's own rescale (image_transforms.rescale) of every byte, float32 [256]: float32(float64(v) * (1 / 255)).  float32(v) * float32(1 / 255) differs in
    the last bit on some bytes."""
    return torch.from_numpy((np.arange(256, dtype=np.uint8).astype(np.float64) * (1 / 255)).astype(np.float32))


def preprocess_statement(frames_bgr: torch.Tensor, proc: dict, table=None, target=None) -> torch.Tensor:
    """uint8 BGR [B, H, W, 3] -> pixel_values float32 [B, 3, th, tw] as ZoeDepthImageProcessor._preprocess makes them (P:220-230): rescale (the table of the byte),
    reflect padding, the bilinear resize with align_corners=True, then (x - mean) / std.  ``proc``: size, multiple, keep_aspect_ratio, mean, std, pad.  ``table`` /
    ``target``: another table of the byte / another (th, tw) than the processor's own (the kernel tests)."""
    rgb = frames_bgr.flip(-1).permute(0, 3, 1, 2)
    if frames_bgr.dtype == torch.uint8:
        x = (rescale_table() if table is None else table).to(frames_bgr.device)[rgb.long()]
    else:   # non-integer pixels (a pre-resized frame): the same rescale, float32(float64(v) * (1 / 255))
        x = (rgb.to(torch.float64) * (1 / 255)).to(torch.float32)
    if proc.get("pad", True):
        ph, pw = pad_amounts(x.shape[2], x.shape[3])
        x = F.pad(x, (pw, pw, ph, ph), mode="reflect")
    th, tw = resize_target(x.shape[2], x.shape[3], proc["size"], proc["multiple"], proc["keep_aspect_ratio"]) if target is None else target
    x = F.interpolate(x, size=(th, tw), mode="bilinear", align_corners=True)
    m = torch.tensor(proc["mean"], dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    s = torch.tensor(proc["std"], dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    return (x - m) / s


def post_statement(pred: torch.Tensor, H: int, W: int, pad: bool = True) -> torch.Tensor:
    """post_process_depth_estimation (P:308-339) as the depth-estimation pipeline calls it -- source_sizes = the frame size, target_sizes None -- for a batch:
    float32 [B, th, tw] -> [B, H, W], per frame the bicubic resize (torchvision's of a float tensor: F.interpolate(mode="bicubic", align_corners=False,
    antialias=False)) to (H + 2 pad_h, W + 2 pad_w) and the padding cut off."""
    outs = []
    ph, pw = pad_amounts(H, W) if pad else (0, 0)
    for depth in pred.unsqueeze(1):
        depth = F.interpolate(depth[None], size=(int(H) + 2 * ph, int(W) + 2 * pw), mode="bicubic", align_corners=False, antialias=False)[0]
        if ph > 0:
            depth = depth[:, ph:-ph, :]
        if pw > 0:
            depth = depth[:, :, pw:-pw]
        outs.append(depth.squeeze(0))
    return torch.stack(outs)


# ---------------------------------------------------------------------------------------------------------------- the metric bin head, composed
def _up(x, size):
    return F.interpolate(x, size=tuple(int(v) for v in size), mode="bilinear", align_corners=True)


def attractor_statement(a: torch.Tensor, prev: torch.Tensor, kind: str = "mean") -> torch.Tensor:
    """ZoeDepthAttractorLayerUnnormed behind its MLP (M:726-746), NCHW: attractor points [B, nA, h, w] (after softplus) and previous bins [B, nb, hp, wp] -> new bins
    [B, nb, h, w]: the module's own loop in the module's own order."""
    c = _up(prev, a.shape[-2:])
    delta = torch.zeros_like(c)
    for i in range(a.shape[1]):
        dx = a[:, i:i + 1] - c
        delta = delta + dx / (1 + 300 * (dx * dx))
    if kind == "mean":
        delta = delta / a.shape[1]
    return c + delta


def bins_statement(last, rel, wrel, P, bins, w1_last, b1, w2, b2, table, min_temp, max_temp) -> torch.Tensor:
    """The conditional log-binomial tail (M:477-491, 417-424) and the expectation behind it (M:1101), NCHW, in the operands' dtype: last [B, 32, H, W], the optional
    relative-depth plane rel [B, H, W] with its weight column wrel [Ch], P = W1_e . e [B, Ch, hc, wc] and bins [B, nb, hc, wc] on the coarse map, w1_last [Ch, 32],
    b1 [Ch], w2 [4, Ch], b2 [4], table [nb] (float32 in the module) -> [B, H, W]."""
    size = last.shape[-2:]
    hid = torch.einsum("ck,bkhw->bchw", w1_last, last)
    if rel is not None:
        hid = hid + wrel.view(1, -1, 1, 1) * rel.unsqueeze(1)
    hid = hid + _up(P, size) + b1.view(1, -1, 1, 1)
    o = F.softplus(torch.einsum("mc,bchw->bmhw", w2, F.gelu(hid)) + b2.view(1, -1, 1, 1)) + 1e-4
    p = o[:, 0] / (o[:, 0] + o[:, 1])
    temp = ((max_temp - min_temp) * (o[:, 2] / (o[:, 2] + o[:, 3])) + min_temp).unsqueeze(1)
    q1, p1 = (1 - p).clamp(min=1e-4, max=1.0).unsqueeze(1), p.clamp(min=1e-4, max=1.0).unsqueeze(1)
    nb = table.numel()
    k = torch.arange(nb, device=last.device).view(1, -1, 1, 1)
    y = table.view(1, -1, 1, 1) + k * torch.log(p1) + (nb - 1 - k) * torch.log(q1)
    return torch.sum(torch.softmax(y / temp, dim=1) * _up(bins, size), dim=1)


def _conv(x, conv, weight=None, bias=None):
    return F.conv2d(x, conv.weight if weight is None else weight, conv.bias if bias is None else bias)


def _mlp_params(*convs):
    return [t for c in convs for t in (c.weight, c.bias)]


class _HeadWeights:
    """The per-configuration tensors of a metric head -- the seed regressor, the four attractor MLPs, the log-binomial MLP with its first weight split into the
    ``last`` columns, the relative-depth column and the embedding columns, and the module's float32 log-binomial table -- as one list per configuration; the
    multi-head class stacks them so that a DEVICE index picks a configuration (``pick``)."""

    def __init__(self, head):
        from transformers.models.zoedepth.modeling_zoedepth import log_binom
        self.multi = hasattr(head, "mlp_classifier")
        if self.multi:
            names = [c["name"] for c in head.bin_configurations]
            parts = [(head.seed_bin_regressors[n], head.attractors[n], head.conditional_log_binomial[n]) for n in names]
        else:
            parts = [(head.seed_bin_regressor, head.attractors, head.conditional_log_binomial)]
        self.n_layers = len(parts[0][1])
        per = []
        for seed, atts, clb in parts:
            lbt = clb.log_binomial_transform
            w1 = clb.mlp[0].weight.detach()[:, :, 0, 0]
            cl = w1.shape[1] - atts[0].conv1.in_channels   # the columns in front of the embedding's: 32, or 33 with the relative depth
            ts = _mlp_params(seed.conv1, seed.conv2) + [t for a in atts for t in _mlp_params(a.conv1, a.conv2)]
            ts += [w1[:, :KERNEL_LAST].contiguous(), (w1[:, KERNEL_LAST] if cl > KERNEL_LAST else w1[:, :0]).contiguous(), w1[:, cl:, None, None].contiguous(),
                   clb.mlp[0].bias, clb.mlp[2].weight[:, :, 0, 0].contiguous(), clb.mlp[2].bias]
            ts = [t.detach() for t in ts]
            ts.append(log_binom(lbt.k_minus_1, lbt.k_idx).reshape(-1).detach())   # float32 in the module whatever its dtype: taken as it is
            per.append(ts)
        self.has_rel = per[0][5 + 4 * self.n_layers].numel() > 0
        self.tensors = [torch.stack(ts) for ts in zip(*per)] if self.multi else per[0]

    def pick(self, index=None):
        """The tensors of configuration ``index`` (a one-element int64 DEVICE tensor: index_select, no host synchronisation), or of the only one."""
        ts = [t.index_select(0, index)[0] for t in self.tensors] if self.multi else self.tensors
        n = self.n_layers
        return dict(seed=ts[0:4], attractors=[ts[4 + 4 * i:8 + 4 * i] for i in range(n)], w1_last=ts[4 + 4 * n], wrel=ts[5 + 4 * n] if self.has_rel else None,
                    w1_e=ts[6 + 4 * n], b1=ts[7 + 4 * n], w2=ts[8 + 4 * n], b2=ts[9 + 4 * n], table=ts[10 + 4 * n])


def _nhwc(x):
    """[B, C, H, W] -> contiguous [B, H, W, C] (no copy where x is channels_last)."""
    return x.permute(0, 2, 3, 1).contiguous()


def head_forward(head, weights: _HeadWeights, outconv_activation, bottleneck, feature_blocks, relative_depth, R=None, min_temp=None, max_temp=None):
    """The forward of ZoeDepthMetricDepthEstimationHead (M:1166-1200) / ZoeDepthMultipleMetricDepthEstimationHeads (M:1054-1103) in the composed form of the module
    docstring -> (metric depth [B, 1, H, W], domain_logits | None, domain index | None).  ``R`` None: the attractor step and the tail are ``attractor_statement`` /
    ``bins_statement`` in ATen, in the inputs' dtype; a Renderer: they are vd3d_zoedepth_attractor_f32 / vd3d_zoedepth_bins_f32 (float32 on the GPU).  ``conv2``, the seed
    regressor, the projectors, the attractor MLPs and W1_e . e are F.conv2d either way; the embedding sum in front of an attractor MLP (up-sampling + add), the ReLUs and
    the softplus are ATen element-wise launches.
    Multi-head: the patch transformer and the classifier are the stock modules; the vote is ``domain_logits.sum(0)`` over the BATCH, as in the module (M:1063) -- a
    frame's prediction depends on the batch it is in, by the model's design -- and the winning configuration's weights are picked by a device index: no ``.item()``."""
    x = head.conv2(bottleneck)
    logits = index = None
    if weights.multi:
        logits = head.mlp_classifier(head.patch_transformer(x)[:, 0, :])
        index = torch.argmax(torch.softmax(logits.sum(dim=0, keepdim=True), dim=-1), dim=-1).reshape(1)
    w = weights.pick(index)
    kind = (head.attractors[head.bin_configurations[0]["name"]] if weights.multi else head.attractors)[0].kind
    s = w["seed"]
    prev_bin = F.softplus(F.conv2d(F.relu(F.conv2d(x, s[0], s[1])), s[2], s[3]))
    prev_emb = head.seed_projector(x)
    if R is not None:
        prev_bin = _nhwc(prev_bin)
    for proj, a, feat in zip(head.projectors, w["attractors"], feature_blocks):
        emb = proj(feat)
        e = emb + _up(prev_emb, emb.shape[-2:])
        pts = F.softplus(F.conv2d(F.relu(F.conv2d(e, a[0], a[1])), a[2], a[3]))
        prev_bin = R.zoedepth_attractor(_nhwc(pts), prev_bin, kind) if R is not None else attractor_statement(pts, prev_bin, kind)
        prev_emb = emb
    last = outconv_activation
    rel = None
    if w["wrel"] is not None:
        rel = relative_depth if relative_depth.shape[-2:] == last.shape[-2:] else _up(relative_depth.unsqueeze(1), last.shape[-2:]).squeeze(1)
    P = F.conv2d(prev_emb, w["w1_e"])
    clb = head.conditional_log_binomial[head.bin_configurations[0]["name"]] if weights.multi else head.conditional_log_binomial   # (one config.min_temp / max_temp)
    min_temp, max_temp = (clb.min_temp if min_temp is None else min_temp), (clb.max_temp if max_temp is None else max_temp)
    if R is not None:
        out = R.zoedepth_bins(_nhwc(last), None if rel is None else rel.contiguous(), w["wrel"], _nhwc(P), prev_bin, w["w1_last"], w["b1"], w["w2"], w["b2"],
                              w["table"], min_temp, max_temp)
    else:
        out = bins_statement(last, rel, w["wrel"], P, prev_bin, w["w1_last"], w["b1"], w["w2"], w["b2"], w["table"], min_temp, max_temp)
    return out.unsqueeze(1), logits, index


@torch.no_grad()
def head_statement(head, outconv_activation, bottleneck, feature_blocks, relative_depth, operands=torch.float64):
    """The metric head in the composed form, everything in ``operands`` (float64 for the tests; float32 gives the kernels' operands) except the float32 log-binomial
    table, which is the module's -> (metric depth [B, 1, H, W], domain_logits | None).  Covers both head classes.  The module itself is not changed: its stock
    sub-modules (conv2, projectors, patch transformer, classifier) are called on a copy in ``operands``."""
    import copy
    h = copy.deepcopy(head).to(operands)
    cast = lambda t: None if t is None else t.to(operands)   # noqa: E731
    out, logits, _ = head_forward(h, _HeadWeights(h), cast(outconv_activation), cast(bottleneck), [cast(f) for f in feature_blocks], cast(relative_depth))
    return out, logits


# ---------------------------------------------------------------------------------------------------------------- the head on own kernels
def head_scope(model, name: str) -> None:
    """What ``MetricHeadRoute`` needs of the model, read from the module graph and the configuration only (nothing is moved or launched); everything it does not cover
    is refused by name -- the caller then keeps the stock head, nothing is substituted silently."""
    what = f"{name!r} ({type(model).__name__})"
    if type(model).__name__ != "ZoeDepthForDepthEstimation":
        raise NotImplementedError(f"zoedepth head route: {what} -- the route replaces the metric head of ZoeDepthForDepthEstimation")
    cfg, head = model.config, model.metric_head

    def refuse(why):
        raise NotImplementedError(f"zoedepth head route: {what}: {why} -- not built; the stock metric head runs (VD3D_ZOE_HEAD=0)")
    if cfg.bin_centers_type != "softplus":
        refuse(f"bin_centers_type={cfg.bin_centers_type!r} (ZoeDepthAttractorLayer sorts and clips the bins; only 'softplus', ZoeDepthAttractorLayerUnnormed, is built)")
    if cfg.attractor_kind not in ("mean", "sum"):
        refuse(f"attractor_kind={cfg.attractor_kind!r} (built: 'mean', 'sum')")
    bins = [int(c["n_bins"]) for c in cfg.bin_configurations]
    if len(set(bins)) != 1:
        refuse(f"bin configurations of {bins} bins (one bin count is built: the configurations' weights are stacked)")
    if bins[0] % 4 or not 4 <= bins[0] <= KERNEL_MAX_BINS:
        refuse(f"{bins[0]} bins (built: a multiple of 4 up to {KERNEL_MAX_BINS})")
    if int(cfg.num_relative_features) != KERNEL_LAST:
        refuse(f"num_relative_features={cfg.num_relative_features} (vd3d_zoedepth_bins_f32 reads a {KERNEL_LAST}-channel feature map)")
    if any(not 1 <= int(n) <= KERNEL_MAX_ATTRACTORS for n in cfg.num_attractors):
        refuse(f"num_attractors={list(cfg.num_attractors)} (built: 1 .. {KERNEL_MAX_ATTRACTORS} per layer)")
    clbs = list(head.conditional_log_binomial.values()) if hasattr(head, "mlp_classifier") else [head.conditional_log_binomial]
    for clb in clbs:
        ch = clb.mlp[0].out_channels
        if ch % 4 or not 4 <= ch <= KERNEL_MAX_HIDDEN or clb.mlp[2].out_channels != 4:
            refuse(f"a log-binomial MLP of {ch} hidden channels and {clb.mlp[2].out_channels} outputs (built: a multiple of 4 up to {KERNEL_MAX_HIDDEN}, 4 outputs)")
        if not isinstance(clb.mlp[1], torch.nn.GELU) or clb.mlp[1].approximate != "none" or not isinstance(clb.mlp[3], torch.nn.Softplus) \
                or clb.mlp[3].beta != 1 or clb.mlp[3].threshold != 20:
            refuse("a log-binomial MLP other than [conv 1x1, exact GELU, conv 1x1, Softplus(beta 1, threshold 20)]")
    if not (float(cfg.min_temp) > 0 and float(cfg.max_temp) >= float(cfg.min_temp)):
        refuse(f"temperatures {cfg.min_temp} .. {cfg.max_temp}")


class MetricHeadRoute:
    """``metric_head.forward`` replaced (``head_scope`` has accepted the model): ``head_forward`` with the pipe's renderer -- per forward four launches of
    vd3d_zoedepth_attractor_f32 and one of vd3d_zoedepth_bins_f32 instead of the module's per-attractor loop (about five element-wise launches for each of the
    16 + 8 + 4 + 1 attractors) and its [B, 64, H, W] tail; the multi-head model's ``.item()`` on the domain vote is gone, ``pipe.zoe_domain`` holds the vote's DEVICE
    index of the last forward (None for the single-head model).  ``pipe.zoe_routes`` says which form runs: {"metric_head": "kernels"}."""

    def __init__(self, pipe):
        self.pipe, self.R, self.head = pipe, pipe.renderer, pipe.model.metric_head
        self.weights = _HeadWeights(self.head)
        pipe.zoe_routes["metric_head"] = "kernels"
        self.head.forward = self.forward

    def forward(self, outconv_activation, bottleneck, feature_blocks, relative_depth):
        out, logits, index = head_forward(self.head, self.weights, outconv_activation, bottleneck, feature_blocks, relative_depth, R=self.R)
        self.pipe.zoe_domain = index
        return out, logits


def route_head(pipe) -> None:
    """DepthPipe's one call: the head route where it applies -- a renderer, float32, ``head_scope`` accepts the model, and the switch (VD3D_ZOE_HEAD, else
    HEAD_ROUTED) says so -- else the stock head, with the reason in ``pipe.zoe_routes``."""
    pipe.zoe_routes, pipe.zoe_domain = {}, None
    sw = zoe_switch("VD3D_ZOE_HEAD")
    if pipe.renderer is None or pipe.dtype != torch.float32:
        pipe.zoe_routes["metric_head"] = "stock: the route needs a renderer and float32"
    elif sw is False or (sw is None and not HEAD_ROUTED):
        pipe.zoe_routes["metric_head"] = "stock: VD3D_ZOE_HEAD=0" if sw is False else "stock: not routed (profiles/r32_zoedepth.md)"
    else:
        try:
            head_scope(pipe.model, pipe.name)
        except NotImplementedError as e:
            pipe.zoe_routes["metric_head"] = f"stock: {e}"
            return
        MetricHeadRoute(pipe)


def preprocessor_from_json(j: dict) -> dict:
    """The processor constants of a ZoeDepth preprocessor_config.json: size, keep_aspect_ratio, ensure_multiple_of (the class default 1 / 32 when the file gives none),
    do_pad, mean and std.  Anything but rescale + [pad] + bilinear resize (PIL resample 2) + normalise is refused by name."""
    if int(j.get("resample", 2)) != 2 or not all(j.get(k, True) for k in ("do_resize", "do_rescale", "do_normalize")):
        raise NotImplementedError("a ZoeDepth image processor other than rescale + reflect padding + bilinear resize (PIL resample 2, align_corners=True) + normalise is "
                                  "not built")
    if j.get("rescale_factor") is not None and float(j["rescale_factor"]) != 1 / 255:
        raise NotImplementedError(f"a ZoeDepth image processor with rescale_factor={j['rescale_factor']} is not built (1 / 255)")
    proc = dict(PROCESSOR, multiple=CLASS_DEFAULT_MULTIPLE)
    sz = j.get("size") or {}
    if isinstance(sz, dict) and "height" in sz:
        proc["size"] = (int(sz["height"]), int(sz["width"]))
    elif isinstance(sz, int):
        proc["size"] = (sz, sz)
    proc["keep_aspect_ratio"] = bool(j.get("keep_aspect_ratio", True))
    if j.get("ensure_multiple_of") is not None:
        m = j["ensure_multiple_of"]
        if not (isinstance(m, (int, float)) and math.isfinite(m) and m > 0):
            raise NotImplementedError(f"a ZoeDepth image processor with ensure_multiple_of={m!r} is not built (a positive number)")
        proc["multiple"] = int(m) if float(m).is_integer() else float(m)
    proc["pad"] = bool(j.get("do_pad", True))
    if j.get("image_mean") is not None:
        proc["mean"] = tuple(float(v) for v in j["image_mean"])
    if j.get("image_std") is not None:
        proc["std"] = tuple(float(v) for v in j["image_std"])
    return proc
