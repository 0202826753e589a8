"""Shared by the DepthPro tests: the two synthetic geometries, the image processor's two ends restated in torch, and the derived bound for comparing two float32
evaluations of ATen's bilinear interpolation.  Not a test module.

MINI (where the kernels can still go wrong): encoders of hidden 384 / 6 heads / 2 layers at 64 x 64 with 16 x 16 patches (a 4 x 4 token grid), DepthPro patch size
64 on a 256 x 256 input -- 1 / 9 / 25 patches, the padding clamp engages (min(4 // 4, 6 or 3) = 1), merged sizes 8 and 12 against outputs 8 and 16.
TRUE-GRID: the same encoders at 384 x 384 (the published 24 x 24 grid) on a 1536 x 1536 input: merges of 24 / 48 / 96, every resize the identity."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24   # unit round-off of float32


def encoder(image_size):
    return dict(model_type="dinov2", hidden_size=384, num_hidden_layers=2, num_attention_heads=6, image_size=image_size, patch_size=16, use_mask_token=False)


def mini_config(**over):
    from transformers import DepthProConfig
    kw = dict(patch_size=64, fusion_hidden_size=64, intermediate_hook_ids=[1, 0], intermediate_feature_dims=[64, 64], scaled_images_feature_dims=[128, 128, 64],
              use_fov_model=True, image_model_config=encoder(64), patch_model_config=encoder(64), fov_model_config=encoder(64))
    kw.update(over)
    return DepthProConfig(**kw)


def true_grid_config():
    from transformers import DepthProConfig
    return DepthProConfig(patch_size=384, fusion_hidden_size=64, intermediate_hook_ids=[1, 0], intermediate_feature_dims=[64, 64], scaled_images_feature_dims=[128, 128, 64],
                          use_fov_model=True, image_model_config=encoder(384), patch_model_config=encoder(384), fov_model_config=encoder(384))


def build(cfg, seed=4, fov_gain=400.0):
    from transformers import DepthProForDepthEstimation
    from visiondepth3d_amd.depth import synthetic_weights_
    m = DepthProForDepthEstimation(cfg).eval()
    synthetic_weights_(m, seed)
    # Unit-gain synthetic weights leave the depth below 0.5 and the field of view within a tenth of a degree of zero: depth * width / focal is then ~ 0, every pixel
    # clamps to 1e-4 and the plane is flat.  The two last layers are therefore scaled and offset: depths of a few units, a field of view around 55 degrees that
    # differs between frames -- the post-process then works in its ordinary range and a wrong value shows in the uint8 plane.
    with torch.no_grad():
        m.head.layers[4].weight.mul_(24.0)
        m.head.layers[4].bias.fill_(5.0)
        if m.fov_model is not None:
            last = m.fov_model.head.layers[-1]
            last.weight.mul_(fov_gain)   # (TRUE-GRID's last convolution is 6 x 6, its sum ten times MINI's: it takes a tenth of the gain)
            last.bias.fill_(55.0)
    return m


def mini_processor():
    from visiondepth3d_amd.depth import PROCESSORS
    return dict(PROCESSORS["depth_pro"], size=(256, 256))


def frames(B, H, W, seed):
    """uint8 BGR frames with structure at every scale (a gradient, a checker and noise), so that a wrong tap shows."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:H, 0:W]
    base = (y * 255 // max(H - 1, 1))[None, :, :, None] * np.array([1, 0, 1]) + (x * 255 // max(W - 1, 1))[None, :, :, None] * np.array([0, 1, 0])
    f = base // 2 + ((y // 7 + x // 5) % 2)[None, :, :, None] * 60 + rng.integers(0, 64, (B, H, W, 3))
    return torch.from_numpy(np.clip(f, 0, 255).astype(np.uint8))


def processor_in_torch(frames_bgr, size):
    """DepthProImageProcessor._preprocess (image_processing_depth_pro.py:70-80) for uint8 BGR frames, in torch because torchvision is not installed: the images
    reach it as RGB uint8 [3, H, W]; rescale_and_normalize (image_processing_backends.py:297-337) fuses the two steps into
    normalize(image.float(), mean * (1 / rescale_factor), std * (1 / rescale_factor)) = (x - 127.5) / 127.5 for mean = std = 0.5, rescale_factor = 1 / 255;
    resize (:205-257) is torchvision's F.resize(..., BILINEAR, antialias=False) of the float tensor = F.interpolate(mode="bilinear", align_corners=False)."""
    rgb = frames_bgr.flip(-1).permute(0, 3, 1, 2).to(torch.float32)
    mean = torch.tensor([0.5, 0.5, 0.5]) * (1.0 / (1 / 255))
    std = torch.tensor([0.5, 0.5, 0.5]) * (1.0 / (1 / 255))
    x = (rgb - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    return F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False, antialias=False)


def post_process_in_torch(predicted_depth, field_of_view, target_sizes):
    """DepthProImageProcessor.post_process_depth_estimation (image_processing_depth_pro.py:92-124), its loop body copied operation for operation (the class cannot
    be imported without torchvision); resample BILINEAR maps to mode "bilinear"."""
    results = []
    fov = [None] * len(predicted_depth) if field_of_view is None else field_of_view
    for depth, fov_value, target_size in zip(predicted_depth, fov, target_sizes):
        if target_size is not None:
            if fov_value is not None:
                width = target_size[1]
                focal_length = 0.5 * width / torch.tan(0.5 * torch.deg2rad(fov_value))
                depth = depth * width / focal_length
            depth = torch.nn.functional.interpolate(input=depth.unsqueeze(0).unsqueeze(1), size=target_size, mode="bilinear").squeeze()
        depth = 1.0 / torch.clamp(depth, min=1e-4, max=1e4)
        results.append(depth)
    return results


def bilinear_bound(A, D, in_h, in_w, extra_rel=0.0):
    """Bound on |a - b| for two float32 evaluations a, b of ATen's bilinear tap formula on the same data, one compiled with every operation rounded on its own
    (the kernels: -ffp-contract=off), the other possibly with multiply-adds contracted (ATen's CPU build).  A = max |value| over the taps, D = max - min over the
    taps' neighbourhood, U = 2^-24.
      1. source coordinate src = scale (d + 0.5) - 0.5: scale = fl(in / out) is the same float in both (a correctly rounded division), d + 0.5 is exact; the
         unfused form rounds the product (<= U in) and the difference (<= U in), the fused form the difference alone -- the two coordinates differ by at most
         2 U in.  The interpolant is continuous and piecewise linear in src with slope at most D per axis (also across a cell boundary, should floor() fall on
         different sides): <= 2 U (in_h + in_w) D.
      2. lambda1 = src - floor(src) is exact; lambda0 = fl(1 - lambda1) errs by <= U / 2 in each evaluation: <= U A per axis for the pair, 2 U A.
      3. the blend l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11): products and sums four deep, each rounding <= U relative on a partial result of magnitude
         <= (1 + U)^2 A; contraction only removes roundings: each evaluation is within 4 U A (1 + 3 U) of the exact blend of its weights, the pair within 9 U A.
      4. ``extra_rel``: a relative difference already present in the tap values (the field-of-view scale of the post-process) passes through with weight sum 1.
    Total: U (11 A + 2 (in_h + in_w) D) + extra_rel A.  Works on floats and tensors."""
    return U * (11.0 * A + 2.0 * (in_h + in_w) * D) + extra_rel * A
