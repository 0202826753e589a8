"""Trained-like weights for the depth networks' tests: ``outlier_weights_(model, seed)``.

``synthetic_weights_`` (visiondepth3d_amd/depth.py) gives unit-gain uniform weights and LayerScale 0.2: the largest value that ever enters a linear layer of
DA-V2-Small is about 5, every LayerNorm output has unit scale and no softmax is sharp.  Trained DINOv2 checkpoints look different, and the split kernels'
range claims (include/vd3d.h) are about exactly that difference.  This recipe starts from the synthetic weights and plants, deterministically from ``seed``:

  * LayerScale spread log-uniformly over two decades (0.02 .. 2) instead of the constant 0.2;
  * "massive activations": in one early and one middle layer, three fc2 output channels 60 times larger than the rest, so the residual stream carries a
    few channels in the hundreds and every later LayerNorm sees rows dominated by them (everything else in such a row becomes small);
  * sharper attention: the query and key projections times 3 (logits times 9);
  * a handful of LayerNorm gains far above (x 6) and far below (x 0.02) one, per LayerNorm; behind the massive layers one of the high gains sits on a
    massive channel, so the linears there see inputs near 100 among values below 1;
  * two layers whose value projection is 2^-8 of the usual size with the output projection 2^8 larger (the same function, exactly): the attention output
    -- the rows the output projection reads -- is small everywhere, 2^-12 .. 2^-6, where the second fp16 term of a split operand is subnormal;
  * a head bias that keeps the prediction off the ReLU floor (the synthetic head predicts exactly 0 on a third of the pixels, where every arithmetic agrees).

Pure NumPy / torch, no file fixtures.  tests/test_outlier_weights_host.py asserts on the CPU, against the stock float64 graph, that the recipe produces
the statistics the GPU tests rely on."""
import zlib

import numpy as np
import torch

from visiondepth3d_amd.depth import synthetic_weights_

MASSIVE_LAYERS = (2, 6)        # fc2 of these blocks grows three massive output channels
MASSIVE_GAIN = 60.0
QK_GAIN = 3.0
LN_HIGH, LN_LOW, LN_EACH = 6.0, 0.02, 4     # per LayerNorm: LN_EACH gains times LN_HIGH and LN_EACH times LN_LOW
SMALL_V_LAYERS = (3, 9)        # value projection times 2^-8, output projection times 2^8
SMALL_V = 2.0 ** -8
HEAD_BIAS = 2.5


def _rng(name, seed):
    return np.random.Generator(np.random.PCG64((zlib.crc32(("outlier:" + name).encode()) ^ (seed * 0x9E3779B1)) & 0xFFFFFFFF))


@torch.no_grad()
def outlier_weights_(model: torch.nn.Module, seed: int = 0) -> None:
    """In place, for a ``DepthAnythingForDepthEstimation`` on a DINOv2 backbone (any of its three sizes)."""
    synthetic_weights_(model, seed)
    params = dict(model.named_parameters())
    layers = list(model.backbone.encoder.layer)
    massive = None
    for li, layer in enumerate(layers):
        pre = f"backbone.encoder.layer.{li}."
        for ls in ("layer_scale1.lambda1", "layer_scale2.lambda1"):
            p = params[pre + ls]
            p.copy_(torch.from_numpy(10.0 ** _rng(pre + ls, seed).uniform(-1.7, 0.3, size=tuple(p.shape))).to(p.dtype))
        for proj in ("query", "key"):
            params[pre + f"attention.attention.{proj}.weight"].mul_(QK_GAIN)
            params[pre + f"attention.attention.{proj}.bias"].mul_(QK_GAIN)
        if li in MASSIVE_LAYERS:
            w, ls2 = params[pre + "mlp.fc2.weight"], params[pre + "layer_scale2.lambda1"]
            if massive is None:   # the same channels in both layers, as in trained checkpoints (the massive channels are a property of the stream)
                massive = torch.from_numpy(_rng("massive", seed).choice(w.shape[0], size=3, replace=False))
            w[massive] *= MASSIVE_GAIN
            ls2[massive] = 1.0    # their LayerScale does not undo them
        if li in SMALL_V_LAYERS:
            params[pre + "attention.attention.value.weight"].mul_(SMALL_V)
            params[pre + "attention.attention.value.bias"].mul_(SMALL_V)
            params[pre + "attention.output.dense.weight"].mul_(1.0 / SMALL_V)
        for ln in ("norm1", "norm2"):
            g = params[pre + ln + ".weight"]
            idx = torch.from_numpy(_rng(pre + ln, seed).choice(g.shape[0], size=2 * LN_EACH, replace=False))
            if massive is not None and li > MASSIVE_LAYERS[0]:
                idx = torch.cat([massive[:1], idx[~torch.isin(idx, massive[:1])]])[:2 * LN_EACH]
            g[idx[:LN_EACH]] *= LN_HIGH
            g[idx[LN_EACH:]] *= LN_LOW
    params["head.conv3.bias"].fill_(HEAD_BIAS)


def stock_model(seed: int, dtype=torch.float64, name: str = "depth-anything-v2-small"):
    """The stock Hugging Face module graph with the outlier weights, on the CPU in ``dtype`` (the float32 parameter values, widened exactly for float64)."""
    from transformers import DepthAnythingForDepthEstimation
    from visiondepth3d_amd.depth import build_config
    model = DepthAnythingForDepthEstimation(build_config(name)).eval()
    outlier_weights_(model, seed)
    return model.to(dtype)


def clip_frames(n: int = 2, h: int = 210, w: int = 378) -> np.ndarray:
    """uint8 BGR frames [n, h, w, 3] of the synthetic clip: 15 x 27 patches of 14 pixels + CLS = 406 tokens (two 256-query workgroups, 22 valid rows in the
    last 64-row KV tile)."""
    from visiondepth3d_amd import synth
    return np.stack([synth.synth_frame(i, h, w)[0] for i in range(n)])


def pixel_values(frames_bgr_u8: np.ndarray, dtype=torch.float64) -> torch.Tensor:
    """The image processor at the frame's own size (a bicubic resize to the same size is the identity): RGB, 1 / 255, ImageNet mean / std, in ``dtype``."""
    from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD
    x = torch.from_numpy(np.ascontiguousarray(frames_bgr_u8[..., ::-1])).permute(0, 3, 1, 2).to(dtype)
    mean = torch.tensor(IMAGENET_MEAN, dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=dtype).view(1, 3, 1, 1)
    return ((x / 255.0) - mean) / std


_REF = {}


@torch.no_grad()
def reference_predictions(seed: int, instrument=None):
    """(pred64, pred32) of the stock graph on the CPU for ``clip_frames()``: float64 behind a float64 pre-process (the reference) and float32 behind a float32
    one (the solver-independent yardstick).  Computed once per seed and process; callers must not modify the tensors.  ``instrument(model64)`` may register
    hooks on the float64 model before its forward (then the forward runs even when cached)."""
    if seed not in _REF or instrument is not None:
        frames = clip_frames()
        m64 = stock_model(seed, torch.float64)
        if instrument is not None:
            instrument(m64)
        p64 = m64(pixel_values=pixel_values(frames, torch.float64)).predicted_depth
        p32 = _REF[seed][1] if seed in _REF else stock_model(seed, torch.float32)(pixel_values=pixel_values(frames, torch.float32)).predicted_depth
        _REF[seed] = (p64, p32)
    return _REF[seed]


def errors_of_range(pred, pred64):
    """(E, RMS): max |pred - pred64| and the root mean square of pred - pred64, both over range(pred64)."""
    d = pred.detach().double().cpu() - pred64
    rng = float(pred64.max() - pred64.min())
    return float(d.abs().max()) / rng, float(d.pow(2).mean().sqrt()) / rng
