"""Shared by the ZoeDepth tests (host and GPU): tiny ZoeDepthForDepthEstimation models in the multi-head and the single-head form, structured uint8 frames, the
image processor and its post-process restated in torch operation for operation (the class's post-process needs torchvision, which is not assumed), and the derivations
of the bounds the GPU tests use."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24   # unit round-off of float32


def tiny_config(multi: bool, **over):
    """BEiT hidden 64, 4 layers, 2 heads, stages 1 - 4, neck 16 / 32 / 64 / 64, fusion = bottleneck 32, bin embedding 32, 64 bins, attractors 16 / 8 / 4 / 1.  The
    classifier of the multi-head model reads 128 features whatever the configuration (modeling_zoedepth.py:985), so the patch transformer keeps hidden size 128."""
    from transformers import ZoeDepthConfig
    bb = dict(model_type="beit", image_size=64, patch_size=16, hidden_size=64, num_hidden_layers=4, num_attention_heads=2, intermediate_size=128,
              use_relative_position_bias=True, use_absolute_position_embeddings=False, reshape_hidden_states=False, out_features=["stage1", "stage2", "stage3", "stage4"])
    bins = [dict(name="nyu", n_bins=64, min_depth=1e-3, max_depth=10.0), dict(name="kitti", n_bins=64, min_depth=1e-3, max_depth=80.0)] if multi else \
        [dict(n_bins=64, min_depth=1e-3, max_depth=10.0)]
    kw = dict(backbone_config=bb, neck_hidden_sizes=[16, 32, 64, 64], fusion_hidden_size=32, bottleneck_features=32, num_relative_features=32, bin_embedding_dim=32,
              num_attractors=[16, 8, 4, 1], bin_centers_type="softplus", bin_configurations=bins)
    if multi:
        kw.update(num_patch_transformer_layers=4, patch_transformer_hidden_size=128, patch_transformer_intermediate_size=64, patch_transformer_num_attention_heads=2)
    kw.update(over)
    return ZoeDepthConfig(**kw)


def tiny_model(multi: bool, seed: int = 0, synthetic: bool = True, **over):
    """With transformers' default initialisation every prediction is the constant log 2 (the MLP outputs vanish): ``synthetic`` plants the project's weights."""
    from transformers import ZoeDepthForDepthEstimation
    from visiondepth3d_amd.depth import synthetic_weights_
    torch.manual_seed(1234 + seed)
    m = ZoeDepthForDepthEstimation(tiny_config(multi, **over)).eval()
    if synthetic:
        synthetic_weights_(m, seed)
    return m


# (the sides are multiples of 32 = patch 16 x the 0.5 reassemble factor: only then has the prediction the size of pixel_values)
TINY_PROCESSOR = dict(size=(64, 96), keep_aspect_ratio=True, multiple=32, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), resample=2, pad=True)


def force_domain(model, which: int):
    """Make the multi-head model vote for configuration ``which`` whatever the input: the classifier's last bias."""
    with torch.no_grad():
        b = model.metric_head.mlp_classifier.linear2.bias
        b.zero_()
        b[which] = 100.0


def frames(B: int, H: int, W: int, seed: int = 0) -> torch.Tensor:
    """Structured uint8 BGR frames: gradients, a checker and noise, with 0 and 255 present."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    f = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        f[b, ..., 0] = (x * 255 // max(W - 1, 1) + 17 * b) % 256
        f[b, ..., 1] = ((y * 3 + x * 5 + 40 * b) % 256)
        f[b, ..., 2] = np.where(((y // 3) + (x // 4)) % 2 == 0, 255, 0) ^ rng.integers(0, 32, (H, W))
    f[:, 0, 0], f[:, -1, -1] = 0, 255
    return torch.from_numpy(f)


def processor_in_class(frames_bgr: torch.Tensor, proc: dict) -> torch.Tensor:
    """ZoeDepthImageProcessorPil itself (it runs without torchvision) on the frames as RGB arrays -> float32 [B, 3, th, tw]."""
    from transformers.models.zoedepth.image_processing_pil_zoedepth import ZoeDepthImageProcessorPil
    P = ZoeDepthImageProcessorPil(size=dict(height=proc["size"][0], width=proc["size"][1]), keep_aspect_ratio=proc["keep_aspect_ratio"],
                                  ensure_multiple_of=proc["multiple"], image_mean=list(proc["mean"]), image_std=list(proc["std"]), do_pad=proc.get("pad", True))
    out = P(images=[np.ascontiguousarray(f.numpy()[..., ::-1]) for f in frames_bgr], return_tensors="pt")
    return out["pixel_values"]


def post_process_in_torch(pred: torch.Tensor, source_sizes, do_remove_padding: bool = True):
    """The loop body of ZoeDepthImageProcessor.post_process_depth_estimation (image_processing_pil_zoedepth.py:303-339) with target_sizes None and no flipped outputs,
    operation for operation; torchvision's resize of a float tensor (BICUBIC, antialias=False) is F.interpolate(mode="bicubic", align_corners=False,
    antialias=False) on the tensor with a batch axis."""
    results = []
    for depth, source_size in zip(pred.unsqueeze(1), source_sizes):
        pad_h = pad_w = 0
        if do_remove_padding:
            pad_h = int(np.sqrt(source_size[0] / 2) * 3)
            pad_w = int(np.sqrt(source_size[1] / 2) * 3)
        depth = F.interpolate(depth[None], size=[source_size[0] + 2 * pad_h, source_size[1] + 2 * pad_w], mode="bicubic", align_corners=False, antialias=False)[0]
        if pad_h > 0:
            depth = depth[:, pad_h:-pad_h, :]
        if pad_w > 0:
            depth = depth[:, :, pad_w:-pad_w]
        results.append(depth.squeeze(0))
    return results


def front_end_bound(in_h: int, in_w: int) -> float:
    """Bound on |kernel - statement| of the front end, two float32 evaluations of rescale table -> reflect gather -> align_corners=True bilinear -> (v - 0.5) / 0.5 on the
    same bytes, one with every operation rounded on its own (the kernel), the other ATen's CPU kernel (possibly contracted, possibly another association of the
    blend).  The table values lie in [0, 1]: A = 1, and neighbouring taps differ by at most D = 1.
      1. source coordinate src = scale d: scale = fl((in - 1) / (out - 1)) is the same float in both; the product is one rounding in both (there is nothing to
         contract it with) -- ATen's CPU kernel computes the same float.  Allowed for anyway: a coordinate difference of U in moves the piecewise linear interpolant
         by at most U in D per axis: U (in_h + in_w) D.
      2. lambda1 = src - floor(src) is exact; lambda0 = fl(1 - lambda1) errs by <= U / 2 in each evaluation: <= U A per axis for the pair, 2 U A.
      3. the blend, four operations deep on partial results of magnitude <= (1 + U)^2 A: each evaluation within 4 U A (1 + 3 U) of the exact blend of its weights,
         the pair within 9 U A.
      4. (v - 0.5) / 0.5: the subtraction rounds once (<= U / 2 on a result of magnitude <= 0.5), the division by 0.5 is exact; it doubles what came before:
         2 (11 U A + U (in_h + in_w) D) + 2 U.
    Total: U (24 + 2 (in_h + in_w))."""
    return U * (24.0 + 2.0 * (in_h + in_w))


def bicubic_bound(A, in_h: int, in_w: int, D):
    """Bound on |kernel - statement| of the post-process: two float32 evaluations of ATen's bicubic (A = -0.75, align_corners=False) on the same data, one with
    every operation rounded on its own (the kernel), the other possibly with multiply-adds contracted (ATen's CPU build).  ``A``: max |v| over the taps'
    neighbourhood, ``D``: max - min over it (tensors, per output pixel).
      1. source coordinate src = scale (d + 0.5) - 0.5, scale the same float in both: the unfused form rounds the product (<= U in) and the difference (<= U in), a
         fused one the difference alone -- the coordinates differ by at most 2 U in per axis.  The interpolant is C1 in src; d/dt sum_k w_k(t) v_k =
         sum_k w_k'(t) (v_k - mean) with |w_1'|, |w_2'| <= 1.5 and |w_0'|, |w_3'| <= 0.75 on their intervals: at most 4.5 D / 2 <= 3 D per unit: 6 U (in_h + in_w) D.
      2. t = src - floor(src) is exact given src.  Each coefficient is a cubic in Horner form; the far taps' (x = t + 1 in [1, 2]: ((a x - 5 a) x + 8 a) x - 4 a) has
         partial results of magnitude <= 4.5 and accumulates, operation by operation, 1.5 U, 4.5 U, 13.5 U, 16.5 U, 36 U, 37 U, plus 3 U for the rounding of x:
         <= 40 U absolute per evaluation (the near taps' less), 80 U for the pair; four taps per axis against values of magnitude <= A: 2 x 4 x 80 U A = 640 U A.
      3. the two four-term dot products: sum |w_k| <= 1.25 per axis, 8 roundings each on magnitudes <= 1.6 A: 2 x 2 x 8 x 1.6 U A <= 52 U A for the pair.
    Total: U (700 A + 6 (in_h + in_w) D), rounded up."""
    return U * (700.0 * A + 6.0 * (in_h + in_w) * D)


def bicubic_local(pred: torch.Tensor, H: int, W: int, ph: int, pw: int):
    """Per output pixel of the cropped bicubic resize: max |v| and max - min of ``pred`` [B, th, tw] over the 7 x 7 neighbourhood of the floor tap (a superset of the
    4 x 4 taps of either evaluation, should floor() fall on different sides)."""
    th, tw = pred.shape[-2:]

    def first(n_in, n_out, pad, n):
        src = np.float32(n_in) / np.float32(n_out) * (np.arange(pad, pad + n, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
        return torch.from_numpy(np.clip(np.floor(src).astype(np.int64), 0, n_in - 1))
    y0, x0 = first(th, H + 2 * ph, ph, H), first(tw, W + 2 * pw, pw, W)
    v = pred[:, None].double()
    mx, mn = F.max_pool2d(v, 7, 1, 3), -F.max_pool2d(-v, 7, 1, 3)
    A, D = torch.maximum(mx.abs(), mn.abs())[:, 0], (mx - mn)[:, 0]
    return A[:, y0][:, :, x0], D[:, y0][:, :, x0]


def linear_taps_numpy(n_in: int, n_out: int):
    """ATen's align_corners=True bilinear taps of one axis in float32 -> (i0, i1, l0, l1): scale = float32(in - 1) / float32(out - 1) (0 for out == 1), src = scale d,
    i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = scale * np.arange(n_out, dtype=np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i0 + (i0 < n_in - 1), (np.float32(1) - l1).astype(np.float32), l1


def bilinear_numpy(x: np.ndarray, h: int, w: int) -> np.ndarray:
    """float32 NHWC [B, hp, wp, C] -> [B, h, w, C]: l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), every operation rounded to float32 on its own."""
    y0, y1, ly0, ly1 = linear_taps_numpy(x.shape[1], h)
    x0, x1, lx0, lx1 = linear_taps_numpy(x.shape[2], w)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    top = lx0 * x[:, y0][:, :, x0] + lx1 * x[:, y0][:, :, x1]
    bot = lx0 * x[:, y1][:, :, x0] + lx1 * x[:, y1][:, :, x1]
    return (ly0[None, :, None, None] * top + ly1[None, :, None, None] * bot).astype(np.float32)


def attractor_numpy(att: np.ndarray, prev: np.ndarray, kind: str) -> np.ndarray:
    """vd3d_zoedepth_attractor_f32 stated in NumPy float32, NHWC: attractor points [B, h, w, nA], previous bins [B, hp, wp, nb] -> [B, h, w, nb]; the module's loop
    (modeling_zoedepth.py:735-743) in the module's operation order: dx dx, times 300, plus 1, the division, the accumulation from zero, / nA for "mean"."""
    att, prev = np.ascontiguousarray(att, np.float32), np.ascontiguousarray(prev, np.float32)
    c = bilinear_numpy(prev, att.shape[1], att.shape[2])
    delta = np.zeros_like(c)
    for i in range(att.shape[3]):
        dx = att[..., i:i + 1] - c
        delta = delta + dx / (np.float32(1) + np.float32(300) * (dx * dx))
    if kind == "mean":
        delta = delta / np.float32(att.shape[3])
    return (c + delta).astype(np.float32)


def planted_tail(B: int, H: int, W: int, hc: int, wc: int, nb: int, with_rel: bool, E: int = 16, Ch: int = 24, seed: int = 0,
                 min_temp: float = 0.0212, max_temp: float = 50.0):
    """Inputs and weights of the log-binomial tail planted so that every branch shows: hidden channels 0 .. 7 each read ONE feature of ``last`` (weight 1, no other
    input) and output m of the MLP is gelu(v[2 m]) - gelu(v[2 m + 1]) plus the small contribution of the random channels (no bias: nothing large cancels on the
    ordinary pixels, so the comparison measures the arithmetic and not the conditioning of the planted weights).  Both v in [0, 1.5] on most pixels (moderate p and
    temperature), and on pixel columns x % 8 == 1 .. 4: (30, 0) on the probability pair -> softplus argument 30 (> 20: the threshold) against -30, 1 - p < 1e-4;
    (0, 30) -> p < 1e-4; (30, 0) on the temperature pair -> temperature near max_temp; (0, 30) -> near min_temp.
    Returns a dict of float32 CPU tensors in the MODULE's layout (NCHW; w1 [Ch, 32 (+ 1) + E]) plus a ZoeDepthConditionalLogBinomialSoftmax carrying the weights."""
    from types import SimpleNamespace

    from transformers.models.zoedepth.modeling_zoedepth import ZoeDepthConditionalLogBinomialSoftmax
    rng = np.random.Generator(np.random.PCG64(seed))
    cl = 32 + int(with_rel)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))   # noqa: E731
    last = rng.uniform(0, 1, (B, 32, H, W))
    drive = rng.uniform(0, 1.5, (B, 8, H, W))
    col = np.arange(W) % 8
    for m0, cols in ((0, (1, 2)), (2, (3, 4))):   # m0: the first output of the pair (probability: 0, 1; temperature: 2, 3)
        for m, hi_col in ((m0, cols[0]), (m0 + 1, cols[1])):
            drive[:, 2 * m, :, col == hi_col], drive[:, 2 * m + 1, :, col == hi_col] = 30.0, 0.0
        drive[:, 2 * m0, :, col == cols[1]], drive[:, 2 * m0 + 1, :, col == cols[1]] = 0.0, 30.0
        drive[:, 2 * m0 + 2, :, col == cols[0]], drive[:, 2 * m0 + 3, :, col == cols[0]] = 0.0, 30.0
    last[:, :8] = drive
    w1 = rng.uniform(-0.2, 0.2, (Ch, cl + E))
    w1[:8] = 0.0
    w1[:, :8] = 0.0
    w1[np.arange(8), np.arange(8)] = 1.0
    b1 = rng.uniform(-0.1, 0.1, Ch)
    b1[:8] = 0.0
    w2 = rng.uniform(-0.3, 0.3, (4, Ch))
    w2[:, :8] = 0.0
    for m in range(4):
        w2[m, 2 * m], w2[m, 2 * m + 1] = 1.0, -1.0
    b2 = rng.uniform(-0.1, 0.1, 4)
    clb = ZoeDepthConditionalLogBinomialSoftmax(SimpleNamespace(min_temp=min_temp, max_temp=max_temp), cl, E, n_classes=nb, bottleneck_factor=1).eval()
    assert clb.mlp[0].weight.shape[0] == cl + E
    clb.mlp[0] = torch.nn.Conv2d(cl + E, Ch, 1)
    clb.mlp[2] = torch.nn.Conv2d(Ch, 4, 1)
    with torch.no_grad():
        clb.mlp[0].weight.copy_(f32(w1)[:, :, None, None]); clb.mlp[0].bias.copy_(f32(b1))
        clb.mlp[2].weight.copy_(f32(w2)[:, :, None, None]); clb.mlp[2].bias.copy_(f32(b2))
    bins = np.sort(rng.uniform(0.3, 9.0, (B, nb, hc, wc)), axis=1)
    return dict(last=f32(last), rel=f32(rng.uniform(0, 2, (B, H, W))) if with_rel else None, e=f32(rng.uniform(-1, 1, (B, E, hc, wc))), bins=f32(bins), clb=clb,
                cl=cl, min_temp=min_temp, max_temp=max_temp)


def tail_in_module(d: dict, dtype):
    """The stock tail in ``dtype`` on the CPU (modeling_zoedepth.py:1184-1198): cat(last [, rel]), the embedding and the bins up-sampled (align_corners=True), the
    conditional log-binomial module, the expectation -> ([B, H, W], the per-pixel magnitude scale max_k |bins|)."""
    import copy
    clb = copy.deepcopy(d["clb"]).to(dtype)
    c = lambda t: t.to(dtype)   # noqa: E731
    last = c(d["last"])
    size = last.shape[-2:]
    if d["rel"] is not None:
        last = torch.cat([last, c(d["rel"]).unsqueeze(1)], dim=1)
    up = lambda t: F.interpolate(c(t), size=tuple(size), mode="bilinear", align_corners=True)   # noqa: E731
    with torch.no_grad():
        x = clb(last, up(d["e"]))
        bins = up(d["bins"])
        return torch.sum(x * bins, dim=1), bins.abs().amax(dim=1)


def head_inputs(model, B: int, th: int, tw: int, seed: int = 0):
    """What ZoeDepthForDepthEstimation.forward hands its metric head for deterministic pixel values: (outconv_activation, bottleneck, feature_blocks, relative_depth)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, th, tw, generator=g) * 2 - 1
    with torch.no_grad():
        fm = model.backbone.forward_with_filtered_kwargs(x).feature_maps
        hs, feat = model.neck(fm, th // model.patch_size, tw // model.patch_size)
        out = [feat] + hs
        rel, features = model.relative_head(hs)
    out = [features] + out
    return out[0], out[1], out[2:], rel
