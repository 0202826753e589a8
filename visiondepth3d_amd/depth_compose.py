"""The depth leg's pure functions of tensors and module attributes: resize targets, the uint8 hand-off, and the weight compositions the routes of
depth_routes.py and depth_pro.py pack (transposed convolution / im2col / patch-embedding GEMM weights, the polyphase neck, the head's coarse-GEMM forms, BiT's
standardised weight).  Nothing here launches a kernel or knows a pipe or a renderer; the module imports torch only."""
import torch
import torch.nn.functional as F


def dpt_resize_target(h: int, w: int, size=518, multiple: int = 14, keep_aspect_ratio: bool = True):
    """DPTImageProcessor.get_resize_output_image_size (keep_aspect_ratio, ensure_multiple_of=14): 1080x1920 -> 518x924."""
    size_h, size_w = (size, size) if isinstance(size, int) else size
    sh, sw = size_h / h, size_w / w
    if keep_aspect_ratio:
        if abs(1 - sw) < abs(1 - sh):
            sh = sw
        else:
            sw = sh

    def snap(v):
        return max(int(round(v / multiple)) * multiple, multiple)

    return snap(sh * h), snap(sw * w)


def depth_to_u8(pred: torch.Tensor, invert: bool = False) -> torch.Tensor:
    """convert_depth_to_grayscale (core/render_depth.py:585-611) per frame, on device: min-max normalise,
    ``(norm*255).astype(uint8)`` truncation; invalid / flat frames -> zeros; optional ``255 - u8`` (:1914-1916)."""
    p = pred.float()
    flat = p.flatten(1)
    mn, mx = flat.min(dim=1).values, flat.max(dim=1).values
    bad = torch.isnan(mn) | torch.isnan(mx) | ((mx - mn) < 1e-6)
    norm = (p - mn[:, None, None]) / (mx - mn + 1e-6)[:, None, None]
    u8 = (norm * 255).clamp(0, 255).to(torch.uint8)
    u8 = torch.where(bad[:, None, None], torch.zeros_like(u8), u8)
    return 255 - u8 if invert else u8


def conv_transpose_gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d weight [C_in, C_out, s, s] (kernel == stride: non-overlapping windows) -> the GEMM weight [(i, j, c_out)][c_in] of
    Y[p][(i, j, co)] = sum_ci X[p][ci] W[ci][co][i][j]; vd3d_depth_to_space_bias_nhwc_f32 then scatters Y's rows to their s x s windows."""
    return w.detach().permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()


def _is_conv(m, k, s, p):
    """Module m convolves with a k x k kernel at stride s and padding p, dilation 1, in one group."""
    return m.kernel_size == (k, k) and m.stride == (s, s) and m.padding == (p, p) and m.dilation == (1, 1) and m.groups == 1


def neck_poly_offsets(f: int):
    """The blocks of the polyphase form of conv3x3(ConvTranspose2d(kernel = stride = f)) in the order vd3d_neck_poly_conv_f32 sums them: [(pa, pb, di, dj)], phases
    (pa, pb) row-major, inside a phase di ascending, then dj ascending.  A fine tap dy in {-1, 0, 1} of phase coordinate a lands in coarse offset (a + dy) // f:
    coordinate 0 reaches {-1, 0}, f - 1 reaches {0, 1}, any other {0}.  (f + 2)^2 blocks: 36 for f = 4 (2.25 per output pixel), 16 for f = 2 (4)."""
    if int(f) != f or f < 2:
        raise ValueError(f"neck_poly: factor {f!r}: an integer of at least 2 expected")
    reach = [sorted({(a + d) // f for d in (-1, 0, 1)}) for a in range(f)]
    return [(pa, pb, di, dj) for pa in range(f) for pb in range(f) for di in reach[pa] for dj in reach[pb]]


def neck_poly_compose(wt: torch.Tensor, bt, w3: torch.Tensor, f: int, dtype=torch.float32):
    """ConvTranspose2d(C, C, kernel_size=f, stride=f) (weight ``wt`` [C_in, C, f, f], bias ``bt`` [C] or None) followed by a bias-free 3 x 3 / padding 1 convolution
    (``w3`` [C_out, C, 3, 3]) as one linear map on the COARSE grid -> (Wc [blocks, C_out, C_in], bc [blocks, C_out]) float32 in ``neck_poly_offsets(f)``'s order:
        out[:, f i + pa, f j + pb] = sum over the blocks k of phase (pa, pb) whose coarse pixel (i + di, j + dj) lies inside the map of  Wc[k] @ x[:, i + di, j + dj] + bc[k]
    Wc[k] sums W3[dy, dx] @ Wt[(pa + dy) % f, (pb + dx) % f]^T over the fine taps (dy, dx) that land in offset (di, dj) = ((pa + dy) // f, (pb + dx) // f), bc[k] sums
    W3[dy, dx] @ bt over the same taps (a coarse pixel outside the map contributes neither: the convolution pads the fine map with zeros, not with the bias).
    Composed in float64, rounded once to ``dtype``.  C_in x blocks / f^2 multiply-adds per output pixel and channel instead of C_in + 9 C."""
    offs = neck_poly_offsets(f)
    if wt.dim() != 4 or w3.dim() != 4 or tuple(wt.shape[2:]) != (f, f) or tuple(w3.shape[2:]) != (3, 3) or w3.shape[1] != wt.shape[1]:
        raise ValueError(f"neck_poly: weights {tuple(wt.shape)} / {tuple(w3.shape)} are not [C_in, C, {f}, {f}] and [C_out, C, 3, 3]")
    if bt is not None and tuple(bt.shape) != (wt.shape[1],):
        raise ValueError(f"neck_poly: bias {tuple(bt.shape)} is not [{wt.shape[1]}]")
    wt64, w364 = wt.detach().to(torch.float64), w3.detach().to(torch.float64)
    bt64 = torch.zeros(wt.shape[1], dtype=torch.float64, device=wt.device) if bt is None else bt.detach().to(torch.float64)
    Wc = torch.zeros(len(offs), w3.shape[0], wt.shape[0], dtype=torch.float64, device=wt.device)
    bc = torch.zeros(len(offs), w3.shape[0], dtype=torch.float64, device=wt.device)
    at = {o: k for k, o in enumerate(offs)}
    for pa in range(f):
        for pb in range(f):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    k = at[pa, pb, (pa + dy) // f, (pb + dx) // f]
                    Wc[k] += w364[:, :, dy + 1, dx + 1] @ wt64[:, :, (pa + dy) % f, (pb + dx) % f].t()
                    bc[k] += w364[:, :, dy + 1, dx + 1] @ bt64
    return Wc.to(dtype).contiguous(), bc.to(dtype).contiguous()


HEAD_UPCONV_BUILT = ((128, 64), (64, 32))   # (C, C_out) of head.conv1 that vd3d_head_upconv_gather_f32 builds and the probe cleared (profiles/r26_head_upconv.md)


def head_upconv_compose(proj_w: torch.Tensor, proj_b, conv1_w: torch.Tensor, dtype=torch.float32):
    """A 1 x 1 projection (weight ``proj_w`` [C, C_in, 1, 1] or [C, C_in], bias ``proj_b`` [C] or None), a bilinear up-sampling and a bias-free 3 x 3 convolution
    (``conv1_w`` [C_out, C, 3, 3], zero padding) have nothing non-linear between them, the up-sampling U acts per channel and a tap's matrix W_t per pixel:
        conv1(U(P h + b_p)) = sum over the 9 taps t of  S_t U ( (W_t P) h + W_t b_p )           (S_t: the tap's shift on the fine grid, zero outside it)
    -> (Wc [9 * C_out, C_in], bc [9 * C_out]): tap t = 3 ky + kx, channel t * C_out + o,
        Wc[t * C_out + o, i] = sum_c conv1_w[o, c, ky, kx] proj_w[c, i],      bc[t * C_out + o] = sum_c conv1_w[o, c, ky, kx] proj_b[c]
    (folding W_t b_p into the coarse map relies on the interpolation weights summing to one).  Composed in float64, rounded once to ``dtype``.  The coarse GEMM
    Z = h Wc^T + bc has a quarter of the fine map's pixels: 9 C_in multiply-adds per coarse pixel and channel instead of C_in per coarse and 9 C per fine one."""
    if conv1_w.dim() != 4 or tuple(conv1_w.shape[2:]) != (3, 3):
        raise ValueError(f"head_upconv: convolution weight {tuple(conv1_w.shape)} is not [C_out, C, 3, 3]")
    Co, Cm = int(conv1_w.shape[0]), int(conv1_w.shape[1])
    if proj_w.dim() not in (2, 4) or proj_w.shape[0] != Cm or (proj_w.dim() == 4 and tuple(proj_w.shape[2:]) != (1, 1)):
        raise ValueError(f"head_upconv: projection weight {tuple(proj_w.shape)} is not [{Cm}, C_in, 1, 1]")
    if proj_b is not None and tuple(proj_b.shape) != (Cm,):
        raise ValueError(f"head_upconv: projection bias {tuple(proj_b.shape)} is not [{Cm}]")
    P = proj_w.detach().to(torch.float64).reshape(Cm, -1)
    W = conv1_w.detach().to(torch.float64).permute(2, 3, 0, 1).reshape(9, Co, Cm)   # [t = 3 ky + kx][o][c]
    b = torch.zeros(Cm, dtype=torch.float64, device=P.device) if proj_b is None else proj_b.detach().to(torch.float64)
    return (W @ P).reshape(9 * Co, -1).to(dtype).contiguous(), (W @ b).reshape(9 * Co).to(dtype).contiguous()


HEAD_CONV2_GATHER_BUILT = (32, 64, 128)    # C_in of head.conv2 (-> 32 channels) that vd3d_head_conv_gather_f32 builds
HEAD_CONV2_GATHER_ROUTED = (32, 64)        # ... and routes by default: those whose probe cleared its bar (profiles/r27_head_conv2_gather.md)


def head_conv2_compose(conv2_w: torch.Tensor, conv1_b: torch.Tensor, dtype=torch.float32):
    """A bias ``conv1_b`` [C], a bilinear up-sampling U and a bias-free 3 x 3 convolution (``conv2_w`` [C_out, C, 3, 3], zero padding) have nothing non-linear between
    them (``head_upconv_compose``'s identity with the identity as projection):
        conv2(U(y1 + b1)) = sum over the 9 taps t of  S_t U ( W_t y1 + W_t b1 )
    -> (Wt [9 * C_out, C], bc [9 * C_out]): tap t = 3 ky + kx, row t * C_out + o,  Wt[t * C_out + o, c] = conv2_w[o, c, ky, kx],  bc[t * C_out + o] = sum_c conv2_w[o, c, ky, kx] b1[c].
    Computed in float64, rounded once to ``dtype`` (Wt is a permutation of the weight: exact)."""
    if conv2_w.dim() != 4 or tuple(conv2_w.shape[2:]) != (3, 3):
        raise ValueError(f"head_conv2: convolution weight {tuple(conv2_w.shape)} is not [C_out, C, 3, 3]")
    Co, Cm = int(conv2_w.shape[0]), int(conv2_w.shape[1])
    if tuple(conv1_b.shape) != (Cm,):
        raise ValueError(f"head_conv2: bias {tuple(conv1_b.shape)} is not [{Cm}]")
    W = conv2_w.detach().to(torch.float64).permute(2, 3, 0, 1).reshape(9, Co, Cm)   # [t = 3 ky + kx][o][c]
    b = conv1_b.detach().to(torch.float64)
    return W.reshape(9 * Co, Cm).to(dtype).contiguous(), (W @ b).reshape(9 * Co).to(dtype).contiguous()


def patch_embedding_gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """Patch-embedding weight [C, 3, p, p] (kernel == stride: every patch is one GEMM row) -> [C, Kp]: the flattened (c, ky, kx) columns, zero-padded from 3 p^2
    to the next multiple of 16 (vd3d_gemm_x3's K unit; p = 14: 588 -> 592).  vd3d_patchify_f32 writes the matching rows, zero tail included."""
    C, k = w.shape[0], w[0].numel()
    return F.pad(w.detach().reshape(C, k), (0, (k + 15) // 16 * 16 - k)).contiguous()


def patch_embedding_conv_ok(conv) -> bool:
    """Conv2d(3, C, kernel_size=p, stride=p), p <= 64: the patch embeddings vd3d_patchify_f32 takes."""
    p = conv.kernel_size[0] if isinstance(conv, torch.nn.Conv2d) else 0
    return 0 < p <= 64 and conv.kernel_size == (p, p) and conv.stride == (p, p) and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.in_channels == 3


def im2col_gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """Convolution weight [C_out, C_in, k, k] -> the GEMM weight [C_out, Kp] whose columns are in vd3d_im2col_nhwc_f32's order, (ky, kx, c_in): a permute to
    [C_out, k, k, C_in], flattened, zero-padded from k k C_in to the next multiple of 16 (the 7 x 7 stem on 3 channels: 147 -> 160)."""
    Cout, kk = w.shape[0], w[0].numel()
    return F.pad(w.detach().permute(0, 2, 3, 1).reshape(Cout, kk), (0, (kk + 15) // 16 * 16 - kk)).contiguous()


def same_padding(size: int, k: int, stride: int):
    """TensorFlow "same" padding of one axis as transformers' DynamicPad2d computes it (dilation 1) -> (low, high): 384 / 7 / 2 -> (2, 3); 96 / 3 / 2 -> (0, 1)."""
    total = max((-(-size // stride) - 1) * stride + k - size, 0)
    return total // 2, total - total // 2


def bit_standardized_weight(m) -> torch.Tensor:
    """The weight a WeightStandardizedConv2d convolves with, by the module's own expression (it recomputes this on every forward), in float32 on the CPU --
    the values the CPU module computes, whatever device the module is on.  Folded once, before packing, by DepthPipe(self_contained=True)."""
    w = m.weight.detach().to("cpu", torch.float32)
    return F.batch_norm(w.reshape(1, m.out_channels, -1), None, None, training=True, momentum=0.0, eps=m.eps).reshape_as(w)
