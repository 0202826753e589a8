"""Frame-interpolation network behind ``upscale.run_rife`` (core/merged_pipeline.py:33-60,204-218).

The reference feeds two BGR frames, concatenated along the channel axis and scaled to [0, 1], to an ONNX Runtime session
(``weights/RIFE_fp32.onnx``: input ``[N, 6, H, W]`` float32, output ``[N, 3, H, W]``, the frame half-way between the two) and keeps
its glue in NumPy.  The ONNX file is not part of the reference tree (``weights/WEIGHTS_README_PLACEHOLDER.md`` points to a download)
and there is no network here, so -- like the depth and up-scale networks -- the ARCHITECTURE is built from its published definition with
deterministic synthetic weights: RIFE v4 "IFNet HDv3" (hzwer/Practical-RIFE, MIT licence; restated from the paper "Real-Time
Intermediate Flow Estimation for Video Frame Interpolation", Huang et al., ECCV 2022, and the public model definition -- no code of it
is in /root/reference).  Three coarse-to-fine IFBlocks (scales 4, 2, 1; 90 channels) estimate the two intermediate flows and a fusion
mask; the frames are back-warped by ``grid_sample`` and blended.  **Parity unpinned** w.r.t. the reference's checkpoint (absent);
``tests/test_hip_upscale.py`` checks the GPU run of ``run_rife`` (HIP glue + this module on PyTorch-ROCm) against a CPU float32 run of
the same module, and ``RifeNet.load_state_dict`` accepts a Practical-RIFE ``flownet.pkl`` state dict (``block0..2`` keys) when one exists.

By default PyTorch-ROCm executes the convolutions (MIOpen); hand-written HIP is the glue on both sides (``vd3d_rife_preprocess`` /
``vd3d_rife_postprocess``), like the reference's split between its session and its NumPy lines.

``RifeSession(..., conv="bf16x3")`` (opt-in) runs the whole forward on this library's kernels instead: the 42 convolutions as 36 launches of
``vd3d_conv_ifn`` (float32-faithful three-term bf16 split on the matrix cores, bias / PReLU / residual in the epilogue; the two transposed-convolution heads
of a block merged into one 96 -> 96 and one block-diagonal 96 -> 32 launch) and the warp / resize / concatenate / blend glue as three HIP kernels.  The
rewrite of the weights (``ifnet_plan``) and the same operation list in plain torch ops (``plan_forward_reference``) are pure torch and run on the CPU.
"""
from __future__ import annotations

import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv(cin, cout, k=3, stride=1, pad=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, pad, bias=True), nn.PReLU(cout))


class IFBlock(nn.Module):
    """One refinement block: two stride-2 convolutions, four residual pairs of 3x3 convolutions, two transposed-convolution heads
    (flow: 4 channels, mask: 1 channel).  ``scale``: the block works at 1/scale of the frame size."""

    def __init__(self, in_planes: int, c: int = 90):
        super().__init__()
        self.conv0 = nn.Sequential(_conv(in_planes, c // 2, 3, 2, 1), _conv(c // 2, c, 3, 2, 1))
        self.convblock0 = nn.Sequential(_conv(c, c), _conv(c, c))
        self.convblock1 = nn.Sequential(_conv(c, c), _conv(c, c))
        self.convblock2 = nn.Sequential(_conv(c, c), _conv(c, c))
        self.convblock3 = nn.Sequential(_conv(c, c), _conv(c, c))
        self.conv1 = nn.Sequential(nn.ConvTranspose2d(c, c // 2, 4, 2, 1), nn.PReLU(c // 2), nn.ConvTranspose2d(c // 2, 4, 4, 2, 1))
        self.conv2 = nn.Sequential(nn.ConvTranspose2d(c, c // 2, 4, 2, 1), nn.PReLU(c // 2), nn.ConvTranspose2d(c // 2, 1, 4, 2, 1))

    def forward(self, x, flow, scale: float = 1.0):
        x = F.interpolate(x, scale_factor=1.0 / scale, mode="bilinear", align_corners=False, recompute_scale_factor=False)
        flow = F.interpolate(flow, scale_factor=1.0 / scale, mode="bilinear", align_corners=False, recompute_scale_factor=False) * (1.0 / scale)
        feat = self.conv0(torch.cat((x, flow), 1))
        feat = self.convblock0(feat) + feat
        feat = self.convblock1(feat) + feat
        feat = self.convblock2(feat) + feat
        feat = self.convblock3(feat) + feat
        flow = self.conv1(feat)
        mask = self.conv2(feat)
        flow = F.interpolate(flow, scale_factor=scale, mode="bilinear", align_corners=False, recompute_scale_factor=False) * scale
        mask = F.interpolate(mask, scale_factor=scale, mode="bilinear", align_corners=False, recompute_scale_factor=False)
        return flow, mask


def backwarp(img: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """Sample ``img`` at ``pixel + flow`` (bilinear, border padding, align_corners=True): the ``warp`` of the published model."""
    n, _, h, w = img.shape
    xs = torch.linspace(-1.0, 1.0, w, device=img.device, dtype=img.dtype).view(1, 1, 1, w).expand(n, -1, h, -1)
    ys = torch.linspace(-1.0, 1.0, h, device=img.device, dtype=img.dtype).view(1, 1, h, 1).expand(n, -1, -1, w)
    grid = torch.cat((xs, ys), 1)
    fl = torch.cat((flow[:, 0:1] / ((w - 1.0) / 2.0), flow[:, 1:2] / ((h - 1.0) / 2.0)), 1)
    g = (grid + fl).permute(0, 2, 3, 1)
    return F.grid_sample(img, g, mode="bilinear", padding_mode="border", align_corners=True)


class RifeNet(nn.Module):
    """IFNet (HDv3, v4.0 form: the blocks see the two warped frames, the mask and the flow; the mid-point is implicit):
    ``forward(x [N,6,H,W] in [0,1]) -> [N,3,H,W]``, the frame half-way between x[:, :3] and x[:, 3:]."""

    def __init__(self, c: int = 90, scale_list=(4.0, 2.0, 1.0)):
        super().__init__()
        self.block0 = IFBlock(7 + 4, c)
        self.block1 = IFBlock(7 + 4, c)
        self.block2 = IFBlock(7 + 4, c)
        self.scale_list = tuple(float(s) for s in scale_list)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        n, _, h, w = x.shape
        ph, pw = (-h) % 32, (-w) % 32           # the coarsest block works at 1/16 of the frame: pad like the published inference script
        if ph or pw:
            x = F.pad(x, (0, pw, 0, ph))
        img0, img1 = x[:, :3], x[:, 3:6]
        flow = torch.zeros_like(x[:, :4])
        mask = torch.zeros_like(x[:, :1])
        w0, w1 = img0, img1
        for blk, sc in zip((self.block0, self.block1, self.block2), self.scale_list):
            f, m = blk(torch.cat((w0, w1, mask), 1), flow, scale=sc)        # 3 + 3 + 1 image channels, + 4 flow channels inside the block
            flow = flow + f
            mask = mask + m
            w0 = backwarp(img0, flow[:, :2])
            w1 = backwarp(img1, flow[:, 2:4])
        mk = torch.sigmoid(mask)
        out = w0 * mk + w1 * (1.0 - mk)
        return out[:, :, :h, :w]


@torch.no_grad()
def synthetic_weights_(model: nn.Module, seed: int = 0) -> None:
    """Deterministic, platform-stable weights (PCG64 keyed by the parameter name), small enough that the estimated flow stays within
    a few pixels: an interpolation that actually moves and blends content, not an identity."""
    for name, p in model.named_parameters():
        rng = np.random.Generator(np.random.PCG64((zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0xFFFFFFFF))
        if p.ndim >= 2:
            fan_in = int(np.prod(p.shape[1:]))
            a = float(np.sqrt(3.0 / max(fan_in, 1))) * 0.7
            v = rng.uniform(-a, a, size=tuple(p.shape)).astype(np.float32)
        elif name.endswith("bias"):
            v = rng.uniform(-0.02, 0.02, size=tuple(p.shape)).astype(np.float32)
        else:                                   # PReLU slopes
            v = np.full(tuple(p.shape), 0.25, np.float32)
        p.copy_(torch.from_numpy(v).to(p.dtype))


# ---- the rewrite behind RifeSession(conv="bf16x3"): padded channel counts, merged heads, the transposed convolution as four phases (pure torch, CPU-capable)
K3S1, K3S2, T4S2 = 0, 1, 2          # _abi.IFN_*: the geometries of vd3d_conv_ifn
_KIND_NAMES = {K3S1: "k3s1", K3S2: "k3s2", T4S2: "t4s2"}


def _ceil_to(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _cout_pad(n: int) -> int:
    for c in (32, 64, 96):
        if n <= c:
            return c
    raise ValueError(f"{n} output channels: the kernels are built for at most 96")


def _zero_pad(t: torch.Tensor, shape) -> torch.Tensor:
    out = t.new_zeros(tuple(shape))
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


def pad_conv(kind: int, w: torch.Tensor, b: torch.Tensor, slope, cin_p: int, cout_p: int):
    """Zero-pad a convolution to ``cin_p`` input and ``cout_p`` output channels: weight (``[Cout,Cin,3,3]``, or ``[Cin,Cout,4,4]`` for ``T4S2``), bias and PReLU
    slopes.  A padded output channel computes 0 * x + 0 -> PReLU(0) = 0, and a padded input channel meets zero weights: the real channels do not change."""
    shape = (cin_p, cout_p) if kind == T4S2 else (cout_p, cin_p)
    return (_zero_pad(w, shape + tuple(w.shape[2:])), _zero_pad(b, (cout_p,)), None if slope is None else _zero_pad(slope, (cout_p,)))


def merge_heads(blk: IFBlock):
    """``conv1[0]`` and ``conv2[0]`` (both c -> c/2 from ``feat``) as ONE c -> 2 (c/2) transposed convolution (flow branch in channels [0, c/2), mask branch behind
    it), ``conv1[2]`` (c/2 -> 4) and ``conv2[2]`` (c/2 -> 1) as ONE block-diagonal 2 (c/2) -> 5 transposed convolution (flow 0..3, mask 4).  Returns
    ``((w1, b1, slope1), (w2, b2))`` in ConvTranspose2d's ``[Cin, Cout, 4, 4]`` layout."""
    a1, p1, o1 = blk.conv1
    a2, p2, o2 = blk.conv2
    h = a1.out_channels
    w1 = torch.cat((a1.weight, a2.weight), 1)
    b1 = torch.cat((a1.bias, a2.bias))
    s1 = torch.cat((p1.weight, p2.weight))
    w2 = w1.new_zeros((2 * h, 5, 4, 4))
    w2[:h, :4] = o1.weight
    w2[h:, 4:] = o2.weight
    b2 = torch.cat((o1.bias, o2.bias))
    return (w1, b1, s1), (w2, b2)


def conv_transpose_4phase(x: torch.Tensor, w: torch.Tensor, b) -> torch.Tensor:
    """``F.conv_transpose2d(x, w, b, stride=2, padding=1)`` for a 4 x 4 kernel as four output phases, each a 2 x 2 stride-1 convolution of the input: output
    (2q + p, .) takes k = 3 at i = q - 1 and k = 1 at i = q for p = 0, k = 2 at i = q and k = 0 at i = q + 1 for p = 1 (the same in x) -- what vd3d_conv_ifn runs."""
    n, _, h, wd = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros((n, w.shape[1], 2 * h, 2 * wd))
    for py in (0, 1):
        for px in (0, 1):
            k = w[:, :, [3 - py, 1 - py], :][:, :, :, [3 - px, 1 - px]].permute(1, 0, 2, 3)      # tap t reads row q + p + t - 1 with k = 3 - p - 2t
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + wd + 1], k, b)
    return out


@torch.no_grad()
def ifnet_plan(net: RifeNet):
    """The 12 launches per IFBlock of ``RifeSession(conv="bf16x3")``, weights padded and heads merged: a list (one per block) of lists of dicts with ``name``,
    ``kind``, ``w``, ``b``, ``slope`` (or None), ``cin`` / ``cout`` (padded), ``real`` (``(cin, cout)`` of the module) and ``residual`` (add the input of the
    previous layer behind the activation).  A 45-channel output is padded to 64 and read back as 48 input channels."""
    plans = []
    for bi, blk in enumerate((net.block0, net.block1, net.block2)):
        L = []

        def add(name, kind, w, b, slope, residual=False):
            cin, cout = (w.shape[0], w.shape[1]) if kind == T4S2 else (w.shape[1], w.shape[0])
            cin_p, cout_p = _ceil_to(cin, 16), _cout_pad(cout)
            wp, bp, sp = pad_conv(kind, w.detach(), b.detach(), None if slope is None else slope.detach(), cin_p, cout_p)
            L.append(dict(name=f"block{bi}.{name}", kind=kind, w=wp, b=bp, slope=sp, cin=cin_p, cout=cout_p, real=(cin, cout), residual=residual))
        for i, seq in enumerate(blk.conv0):
            add(f"conv0.{i}", K3S2, seq[0].weight, seq[0].bias, seq[1].weight)
        for j in range(4):
            cb = getattr(blk, f"convblock{j}")
            add(f"convblock{j}.0", K3S1, cb[0][0].weight, cb[0][0].bias, cb[0][1].weight)
            add(f"convblock{j}.1", K3S1, cb[1][0].weight, cb[1][0].bias, cb[1][1].weight, residual=True)
        (w1, b1, s1), (w2, b2) = merge_heads(blk)
        add("heads.0", T4S2, w1, b1, s1)
        add("heads.1", T4S2, w2, b2, None)
        plans.append(L)
    return plans


def warp_pixels(img: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """``backwarp`` in pixel units: a bilinear sample of ``img`` at ``pixel + flow`` with the position clamped to the image (what grid_sample's border padding with
    align_corners=True computes once its normalisation is undone)."""
    n, c, h, w = img.shape
    xs = (torch.arange(w, device=img.device, dtype=img.dtype).view(1, 1, w) + flow[:, 0]).clamp(0, w - 1)
    ys = (torch.arange(h, device=img.device, dtype=img.dtype).view(1, h, 1) + flow[:, 1]).clamp(0, h - 1)
    x0, y0 = xs.floor(), ys.floor()
    ax, ay = (xs - x0).unsqueeze(1), (ys - y0).unsqueeze(1)
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    flat = img.flatten(2)

    def at(yy, xx):
        return flat.gather(2, (yy * w + xx).view(n, 1, h * w).expand(n, c, h * w)).view(n, c, h, w)
    return at(y0, x0) * ((1 - ax) * (1 - ay)) + at(y0, x1) * (ax * (1 - ay)) + at(y1, x0) * ((1 - ax) * ay) + at(y1, x1) * (ax * ay)


def downscale_2tap(t: torch.Tensor, s: int) -> torch.Tensor:
    """``F.interpolate(t, scale_factor=1/s, bilinear, align_corners=False)`` for sizes that are multiples of s in {1, 2, 4}: the mean of the two centre pixels of
    each s-cell per axis."""
    if s == 1:
        return t
    a, b = s // 2 - 1, s // 2
    return 0.5 * (0.5 * t[:, :, a::s, a::s] + 0.5 * t[:, :, a::s, b::s]) + 0.5 * (0.5 * t[:, :, b::s, a::s] + 0.5 * t[:, :, b::s, b::s])


def run_layer_reference(layer: dict, x: torch.Tensor, residual=None) -> torch.Tensor:
    """One entry of ``ifnet_plan`` with plain torch ops on an NCHW tensor (channels [0, cin) of ``x`` are read)."""
    w, b = layer["w"].to(x.dtype), layer["b"].to(x.dtype)
    x = x[:, :layer["cin"]]
    if layer["kind"] == T4S2:
        y = conv_transpose_4phase(x, w, b)
    else:
        y = F.conv2d(x, w, b, 2 if layer["kind"] == K3S2 else 1, 1)
    if layer["slope"] is not None:
        y = torch.where(y >= 0, y, layer["slope"].to(x.dtype).view(1, -1, 1, 1) * y)
    return y if residual is None else y + residual


@torch.no_grad()
def plan_forward_reference(net: RifeNet, x: torch.Tensor, plans=None) -> torch.Tensor:
    """``RifeNet.forward`` as the operation list ``RifeSession(conv="bf16x3")`` launches, executed with plain torch ops in ``x``'s dtype (float64 on the CPU for the
    host-side proof that the rewrite is the same function): padded and merged weights, four-phase transposed convolutions, the 2-tap down-scale, the
    pixel-unit warp."""
    plans = ifnet_plan(net) if plans is None else plans
    n, _, h, w = x.shape
    ph, pw = (-h) % 32, (-w) % 32
    xp = F.pad(x, (0, pw, 0, ph))
    img0, img1 = xp[:, :3], xp[:, 3:6]
    flow, mask = torch.zeros_like(xp[:, :4]), torch.zeros_like(xp[:, :1])
    for L, sc in zip(plans, net.scale_list):
        s = int(sc)
        inp = downscale_2tap(torch.cat((warp_pixels(img0, flow[:, :2]), warp_pixels(img1, flow[:, 2:4]), mask, flow), 1), s)
        inp = torch.cat((inp[:, :7], inp[:, 7:] * (1.0 / s), torch.zeros_like(inp[:, :5])), 1)        # 16 channels: 7 image, 4 flow / s, 5 zeros
        t = run_layer_reference(L[0], inp)
        feat = run_layer_reference(L[1], t)
        for j in range(4):
            t = run_layer_reference(L[2 + 2 * j], feat)
            feat = run_layer_reference(L[3 + 2 * j], t, residual=feat)
        t = run_layer_reference(L[11], run_layer_reference(L[10], feat))
        up = t[:, :5] if s == 1 else F.interpolate(t[:, :5], scale_factor=float(s), mode="bilinear", align_corners=False, recompute_scale_factor=False)
        flow = flow + up[:, :4] * float(s)
        mask = mask + up[:, 4:5]
    mk = torch.sigmoid(mask)
    out = warp_pixels(img0, flow[:, :2]) * mk + warp_pixels(img1, flow[:, 2:4]) * (1.0 - mk)
    return out[:, :, :h, :w]


class RifeSession:
    """The callable ``upscale.run_rife`` takes as its session: ``[N,6,H,W] -> [N,3,H,W]`` on the device (float32 like ``RIFE_fp32.onnx``;
    channels_last memory for MIOpen).

    ``conv=None`` (default): the module graph on PyTorch-ROCm.  ``conv="bf16x3"``: the whole forward on this library's kernels (``vd3d_conv_ifn`` and the three
    ``vd3d_rife_*`` glue kernels, include/vd3d.h) on ``renderer``'s stream -- needs a ``renderer`` and a CUDA device, float32; anything else raises ``ValueError``
    (there is no fall-back).  ``routes`` then lists, per convolution launch, ``(layer, kernel, padded shape)`` of the last forward, ``glue_routes`` the glue launches."""

    def __init__(self, device="cuda", dtype=torch.float32, net: RifeNet | None = None, seed: int = 0, renderer=None, conv=None):
        self.device, self.dtype = torch.device(device), dtype
        if conv not in (None, "bf16x3"):
            raise ValueError(f"RifeSession: conv={conv!r} is not a mode (None | 'bf16x3')")
        if conv == "bf16x3":
            if renderer is None:
                raise ValueError("RifeSession(conv='bf16x3') needs a renderer (its context and stream run the kernels)")
            if self.device.type != "cuda":
                raise ValueError("RifeSession(conv='bf16x3') runs on the GPU only: there is no CPU path for the kernels")
            if dtype != torch.float32:
                raise ValueError("RifeSession(conv='bf16x3') is the float32 network (three-term bf16 split); dtype must be torch.float32")
        self.conv, self.renderer = conv, renderer
        self.routes, self.glue_routes = [], []
        if net is None:
            net = RifeNet()
            synthetic_weights_(net, seed)
        self.net = net.eval().to(self.device, dtype)
        if self.device.type == "cuda":
            self.net = self.net.to(memory_format=torch.channels_last)
        if conv == "bf16x3":
            if tuple(self.net.scale_list) != (4.0, 2.0, 1.0):
                raise ValueError("RifeSession(conv='bf16x3') is built for the scale list (4, 2, 1)")
            self.device = renderer.device
            self._layers = []
            for L in ifnet_plan(self.net):
                packed = []
                for ly in L:
                    img = renderer.conv_ifn_pack(ly["kind"], ly["w"])
                    if img is None:
                        raise ValueError(f"RifeSession(conv='bf16x3'): {ly['name']} {ly['real']} has no kernel")
                    packed.append(dict(ly, img=img, b=ly["b"].to(self.device, torch.float32).contiguous(),
                                       slope=None if ly["slope"] is None else ly["slope"].to(self.device, torch.float32).contiguous(), w=None))
                self._layers.append(packed)
            self._bufs = {}

    def _buffers(self, n, h, w):
        key = (n, h, w)
        if key not in self._bufs:
            self._bufs.clear()                                      # one input size at a time
            hp, wp = _ceil_to(h, 32), _ceil_to(w, 32)
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)      # noqa: E731
            nhwc = lambda c, hh, ww: z(n, hh, ww, c).permute(0, 3, 1, 2)                          # noqa: E731  a channels_last [n,c,hh,ww] view
            blocks = []
            for s in (4, 2, 1):
                hs, ws = hp // s, wp // s
                blocks.append(dict(inp=nhwc(16, hs, ws), c0=nhwc(64, hs // 2, ws // 2), f=[nhwc(96, hs // 4, ws // 4) for _ in range(3)],
                                   h1=nhwc(96, hs // 2, ws // 2), t=nhwc(32, hs, ws)))
            self._bufs[key] = dict(state=z(n, hp, wp, 8), blocks=blocks, out=z(n, 3, h, w))
        return self._bufs[key]

    def _forward_hip(self, x: torch.Tensor) -> torch.Tensor:
        R = self.renderer
        x = x.to(self.device, torch.float32).contiguous()
        n, c, h, w = x.shape
        if c != 6:
            raise ValueError("RifeSession: the input is [N,6,H,W]")
        B = self._buffers(n, h, w)
        state, routes, glue = B["state"], [], []

        def conv(ly, src, dst, residual=None):
            R.conv_ifn(ly["kind"], src, ly["cin"], ly["img"], ly["b"], ly["slope"], ly["cout"], dst, 0, residual)
            routes.append((ly["name"], "vd3d_conv_ifn/" + _KIND_NAMES[ly["kind"]], (n, int(src.shape[2]), int(src.shape[3]), ly["cin"], ly["cout"])))
        for bi, (L, s) in enumerate(zip(self._layers, (4, 2, 1))):
            bb = B["blocks"][bi]
            R.rife_warp_pack(x, None if bi == 0 else state, s, bb["inp"].permute(0, 2, 3, 1))
            glue.append((f"block{bi}.input", "vd3d_rife_warp_pack", s))
            conv(L[0], bb["inp"], bb["c0"])
            f = bb["f"]
            conv(L[1], bb["c0"], f[0])
            cur = 0
            for j in range(4):
                tmp, nxt = (cur + 1) % 3, (cur + 2) % 3
                conv(L[2 + 2 * j], f[cur], f[tmp])
                conv(L[3 + 2 * j], f[tmp], f[nxt], residual=f[cur])
                cur = nxt
            conv(L[10], f[cur], bb["h1"])
            conv(L[11], bb["h1"], bb["t"])
            R.rife_update(bb["t"].permute(0, 2, 3, 1), state, s, bi == 0, h, w)
            glue.append((f"block{bi}.update", "vd3d_rife_update", s))
        out = R.rife_blend(x, state, B["out"])
        glue.append(("blend", "vd3d_rife_blend", 1))
        R.ordered_after()
        self.routes, self.glue_routes = routes, glue
        return out.clone()

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if self.conv == "bf16x3":
            return self._forward_hip(x)
        x = x.to(self.device, self.dtype)
        if self.device.type == "cuda":
            x = x.contiguous(memory_format=torch.channels_last)
        return self.net(x)
