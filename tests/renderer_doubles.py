"""Torch doubles of the renderer for CPU tests of the rewrites (tests/test_dpt_split_rewrite.py, tests/test_vit_blocks.py): every entry point states in float32
what the HIP kernel computes (include/vd3d.h) and counts its calls."""
import torch

F = torch.nn.functional


class SplitDouble:
    """Float32 torch statements of the renderer entry points the rewrite calls (include/vd3d.h)."""

    def __init__(self):
        self.calls = dict(linear_x3=0, attention_x3=0, attention_f32=0, add_layernorm=0, depth_to_space_bias=0, bias_act=0, upsample_bilinear_bias=0, dpt_head_tail=0)

    def gemm_x3_pack(self, w, mode="bf16x3"):
        return w.detach().float().contiguous()

    def linear_x3(self, x, img, N, bias=None, gelu=False, mode="bf16x3"):
        self.calls["linear_x3"] += 1
        assert x.is_contiguous() and img.shape == (N, x.shape[-1])
        y = F.linear(x, img, bias)
        return F.gelu(y) if gelu else y

    def attention_x3(self, qkv, n_heads, scale, mode="bf16x3"):
        self.calls["attention_x3"] += 1
        return self._attention(qkv, n_heads, scale)

    def attention_f32(self, qkv, n_heads, scale, form=0):
        self.calls["attention_f32"] += 1
        assert qkv.dtype == torch.float32 and qkv.is_contiguous() and qkv.shape[-1] == 3 * n_heads * 64
        return self._attention(qkv, n_heads, scale)

    @staticmethod
    def _attention(qkv, n_heads, scale):
        B, T, C3 = qkv.shape
        q, k, v = qkv.view(B, T, 3, n_heads, C3 // (3 * n_heads)).unbind(2)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=scale)
        return o.transpose(1, 2).reshape(B, T, C3 // 3)

    def add_layernorm(self, x, y, norm):
        self.calls["add_layernorm"] += 1
        s = x if y is None else x + y
        return s, F.layer_norm(s, norm.normalized_shape, norm.weight, norm.bias, norm.eps)

    def depth_to_space_bias(self, y, B, H, W, s, bias=None):
        self.calls["depth_to_space_bias"] += 1
        C = y.shape[1] // (s * s)
        o = y.view(B, H, W, s, s, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H * s, W * s, C)
        if bias is not None:
            o = o + bias
        return o.permute(0, 3, 1, 2)

    def conv3x3_x2_pack(self, w):
        return w.detach().float().contiguous() if w.shape[0] in (32, 64, 128) and w.shape[1] % 16 == 0 else None

    def conv3x3_x2(self, x, img, Cout):
        return F.conv2d(x, img, None, 1, 1).contiguous(memory_format=torch.channels_last)

    def upsample_bilinear(self, x, size):
        return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)

    def bias_act(self, y, bias=None, r1=None, r2=None, relu=False, want_relu_copy=False):
        self.calls["bias_act"] += 1
        v = y if bias is None else y + bias.view(1, -1, 1, 1)
        if r1 is not None:
            v = v + r1
        if r2 is not None:
            v = r2 + v
        if relu:
            v = torch.relu(v)
        y.copy_(v)
        return (y, torch.relu(y)) if want_relu_copy else y

    def upsample_bilinear_bias(self, x, size, bias):
        self.calls["upsample_bilinear_bias"] += 1
        return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True) + bias.view(1, -1, 1, 1)

    def dpt_head_tail(self, y, b2, w3, b3, scale):
        self.calls["dpt_head_tail"] += 1
        return torch.relu((torch.relu(y + b2.view(1, -1, 1, 1)) * w3.view(1, -1, 1, 1)).sum(1) + b3) * scale
