"""Pillow's 8-bit bicubic resampler (``ImagingResample``, what ``Image.resize(size, Image.BICUBIC)`` runs on an RGB image) stated in integers, and the
Hugging Face image processor's rescale + normalise as a table -- the reference's depth front end (core/render_depth.py:1113-1116 and the
DPTImageProcessor behind its pipeline), bit for bit.

``coeffs(n_in, n_out)``      the per-axis tables in numpy float64: first tap, tap count and the 22-bit fixed-point coefficients of every output index
``resize(t, w, h)``          uint8 [..., H, W, 3] torch tensor (CPU or GPU) -> uint8 [..., h, w, 3]; integer arithmetic only in the pixel path
``normalise_lut(mean, std)`` float32 [3, 256]: the processor's ``(v * rescale - mean) / std`` of every byte value, per channel

This is the CPU implementation of ``DepthPipe(front_end="pil")``, what runs on the device where a geometry exceeds the tap budget of
csrc/vd3d_pilresample.hip, and the statement the GPU tests compare the kernels with (tests/test_pil_resample_host.py holds it to Pillow itself)."""
from __future__ import annotations

import functools

import numpy as np
import torch

PRECISION_BITS = 22   # Pillow: 32 - 8 - 2


def _cubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


@functools.lru_cache(maxsize=256)
def coeffs(n_in: int, n_out: int):
    """(xmin int64 [n_out], count int64 [n_out], k int32 [n_out, ksize]) of one axis; taps past ``count`` are zero.  Every step is IEEE double in
    Pillow's order (precompute_coeffs + normalize_coeffs_8bpc): the sum runs in index order, the casts truncate."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("sizes must be positive")
    scale = np.float64(n_in) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support = 2.0 * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    count = xmax - xmin
    w = np.zeros((n_out, ksize), np.float64)
    tot = np.zeros(n_out, np.float64)
    for j in range(ksize):
        wj = np.where(j < count, _cubic((np.float64(j) + xmin - center + 0.5) * ss), 0.0)
        w[:, j] = wj
        tot = tot + wj   # a tap past the count adds +0.0: the sum of the taps in index order
    inv = np.where(tot != 0.0, 1.0 / np.where(tot != 0.0, tot, 1.0), 1.0)
    w = w * inv[:, None]
    k = np.where(w < 0, np.trunc(w * float(1 << PRECISION_BITS) - 0.5), np.trunc(w * float(1 << PRECISION_BITS) + 0.5)).astype(np.int32)
    for a in (xmin, count, k):
        a.setflags(write=False)
    return xmin, count, k


def _pass(t: torch.Tensor, axis: int, n_out: int) -> torch.Tensor:
    """One pass along ``axis`` of an integer tensor holding bytes: int32 sums from 2^21, arithmetic shift, clamp -- a uint8 image again."""
    n_in = t.shape[axis]
    xmin, count, k = coeffs(n_in, n_out)
    xm = torch.tensor(xmin, device=t.device)
    kk = torch.tensor(k, device=t.device)
    shape = [1] * t.dim()
    shape[axis] = n_out
    src = t.to(torch.int32)
    acc = None
    for j in range(int(count.max())):
        idx = (xm + j).clamp_(max=n_in - 1)   # past the count the coefficient is zero: any byte may stand there
        term = src.index_select(axis, idx) * kk[:, j].view(shape)
        acc = term + (1 << (PRECISION_BITS - 1)) if acc is None else acc + term
    return (acc >> PRECISION_BITS).clamp_(0, 255).to(torch.uint8)


def resize(t: torch.Tensor, w: int, h: int) -> torch.Tensor:
    """``Image.fromarray(t).resize((w, h), Image.BICUBIC)`` for every image of a uint8 [..., H, W, 3] tensor: the horizontal pass first and only if the
    width changes, then the vertical pass on that uint8 image and only if the height changes; equal sizes are a copy."""
    if t.dtype != torch.uint8 or t.dim() < 3:
        raise TypeError("resize takes a uint8 [..., H, W, C] tensor")
    w, h = int(w), int(h)
    H, W = t.shape[-3], t.shape[-2]
    out = t
    if w != W:
        out = _pass(out, t.dim() - 2, w)
    if h != H:
        out = _pass(out, t.dim() - 3, h)
    return out.clone() if out is t else out


def normalise_lut(mean, std, rescale: float = 1 / 255) -> torch.Tensor:
    """float32 [3, 256]: ``float32(float64(v) * rescale)``, then ``(x - float32(mean)) / float32(std)`` in float32 -- what the image processor's rescale
    and normalise make of the byte ``v`` in channel c."""
    x = (np.arange(256, dtype=np.float64) * np.float64(rescale)).astype(np.float32)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    return torch.from_numpy(((x[None, :] - m[:, None]) / s[:, None]).astype(np.float32))


def pixel_values(frames_bgr: torch.Tensor, th: int, tw: int, mean, std, dtype=torch.float32, inference_size=None) -> torch.Tensor:
    """The network input of uint8 BGR [B, H, W, 3] frames: optional pre-resize to ``inference_size`` = (W', H'), resize to (th, tw), RGB, table.
    Returns ``dtype`` NHWC [B, th, tw, 3] (the table rounded to bf16 first for a bf16 result)."""
    u8 = frames_bgr
    if inference_size is not None:
        u8 = resize(u8, int(inference_size[0]), int(inference_size[1]))
    u8 = resize(u8, tw, th)
    lut = normalise_lut(mean, std).to(u8.device).to(dtype)
    idx = u8.flip(-1).long()
    return torch.stack([lut[c][idx[..., c]] for c in range(3)], dim=-1)
