"""The pre-LayerNorm transformer block of the ViT encoders (Dinov2Layer: Depth-Anything's backbone, DepthPro's three encoders; DPTViTLayer: DPT-Large, DPT-Hybrid) as
an inference-only rewrite, stated once: same math as the stock modules, fewer launches.  ``BlockOperands`` is one layer as tensors (``dinov2_operands``,
``dpt_vit_operands``), ``_block`` the skeleton every mode shares, and a back-end says where its linears, attention and residual add + LayerNorm pairs run:
``_LibraryBackend`` (``mode="f32"``, float32 or bf16: library GEMMs, vd3d_attention_f32 or SDPA, vd3d_add_layernorm with a renderer and plain ATen operators without
one) or ``_SplitBackend`` ("bf16x3" / "fp16x2", float32 only: vd3d_gemm_x3, vd3d_attention_x3, vd3d_add_layernorm; what it is not built for is refused by name at the
call).  ``encoder_blocks`` chains the blocks of one encoder and owns the stash between them.  Nothing here knows ``DepthPipe``; ``renderer`` is anything with
``render_3d.Renderer``'s entry points of these names."""
from collections import namedtuple

import torch
import torch.nn.functional as F

HIDDEN_SIZES = (384, 768, 1024)   # what vd3d_add_layernorm and the attention kernels are built for
# one transformer layer as the operands of _block: Linear weights [out, in] and biases (bqkv may be None; w1 = fc1, w2 = fc2), the two LayerNorm modules, the activation module
BlockOperands = namedtuple("BlockOperands", "wqkv bqkv wo bo w1 b1 w2 b2 heads head_dim scaling norm1 norm2 act")


def head_geometry_ok(hidden: int, heads: int) -> bool:
    """Hidden size 384 / 768 / 1024 in 64-wide heads: every DINOv2 size, ViT-B/16 and ViT-L/16."""
    return int(hidden) in HIDDEN_SIZES and int(hidden) == 64 * int(heads)


def _qkv(att):
    """q / k / v weights and biases concatenated for ONE GEMM (N = 3 * hidden)."""
    w = torch.cat([att.query.weight, att.key.weight, att.value.weight], 0).contiguous()
    return w, None if att.query.bias is None else torch.cat([att.query.bias, att.key.bias, att.value.bias], 0).contiguous()


@torch.no_grad()
def dinov2_operands(layer) -> BlockOperands:
    """A Dinov2Layer: LayerScale folded into the output projection and fc2 (lambda * (xW^T + b) == x(lambda*W)^T + lambda*b), in float32 whatever the model's dtype."""
    def scaled(lin, lam):
        lam = lam.float()
        return (lin.weight.float() * lam[:, None]).to(lin.weight.dtype).contiguous(), (lin.bias.float() * lam).to(lin.bias.dtype).contiguous()
    att, mlp = layer.attention.attention, layer.mlp
    return BlockOperands(*_qkv(att), *scaled(layer.attention.output.dense, layer.layer_scale1.lambda1), mlp.fc1.weight, mlp.fc1.bias,
                         *scaled(mlp.fc2, layer.layer_scale2.lambda1), att.num_attention_heads, att.attention_head_size, att.scaling, layer.norm1, layer.norm2, mlp.activation)


@torch.no_grad()
def dpt_vit_operands(layer) -> BlockOperands:
    """A DPTViTLayer: layernorm_before / layernorm_after are its two LayerNorms (eps 1e-12), attention.output.dense the output projection, intermediate.dense fc1
    (hidden_act "gelu": exact), output.dense fc2 (the module adds the residual itself; here the block does).  There is no LayerScale to fold."""
    att, out, fc1, fc2 = layer.attention.attention, layer.attention.output.dense, layer.intermediate.dense, layer.output.dense
    return BlockOperands(*_qkv(att), out.weight, out.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, att.num_attention_heads, att.attention_head_size, att.scaling,
                         layer.layernorm_before, layer.layernorm_after, layer.intermediate.intermediate_act_fn)


def query_padding(embeddings, final_norm) -> dict:
    """Query-length padding for the library back-end on the GPU: AOTriton's flash kernel takes a ~1.5x slower path when the QUERY length is not a multiple of 256
    (measured on MI355X: Tq=2443 446 us, Tq=2560 302 us per layer, keys unpadded).  DINOv2 always has an odd token count (patches + CLS), so the bf16 token sequence is
    padded ONCE after ``embeddings`` with dummy tokens that are never used as keys / values (k, v are sliced to the real length) and are dropped before ``final_norm``:
    exact.  Returns ``{"T": the real token count of the forward in flight, or None}`` for ``encoder_blocks(pad_state=)``."""
    pad_state = {"T": None}

    def pad_tokens(_mod, _inp, out):
        T = out.shape[1]
        Tp = -(-T // 256) * 256
        pad_state["T"] = None
        if out.dtype == torch.bfloat16 and Tp != T and Tp <= T * 1.1:
            pad_state["T"] = T
            return F.pad(out, (0, 0, 0, Tp - T))
        return out
    embeddings.register_forward_hook(pad_tokens)
    final_ln = final_norm.forward
    final_norm.forward = lambda x: final_ln(x if pad_state["T"] is None else x[:, :pad_state["T"]])
    return pad_state


def _sdpa(qkv, B, T, d, ops, Tk):
    qkv = qkv.view(B, T, 3, ops.heads, ops.head_dim)   # real tokens only on the key / value side
    q, k, v = qkv[:, :, 0].transpose(1, 2), qkv[:, :Tk, 1].transpose(1, 2), qkv[:, :Tk, 2].transpose(1, 2)
    return F.scaled_dot_product_attention(q, k, v, scale=ops.scaling).transpose(1, 2).reshape(B, T, d)


class _LibraryBackend:
    """``mode="f32"``: library GEMMs on the folded weights.  ``begin`` decides per call whether the renderer's launches take the add + LayerNorm pairs."""
    gelu = False   # the activation runs behind fc1

    def __init__(self, renderer, ops, pad_state):
        self.R, self.ops, self.pad = renderer, ops, pad_state or {"T": None}
        self.w = dict(qkv=(ops.wqkv, ops.bqkv), wo=(ops.wo, ops.bo), fc1=(ops.w1, ops.b1), w2=(ops.w2, ops.b2))

    def begin(self, x):
        self.hip = self.R is not None and x.dtype in (torch.bfloat16, torch.float32) and x.is_contiguous() and x.shape[-1] in HIDDEN_SIZES

    def lin(self, key, t, gelu=False):
        return F.linear(t, *self.w[key])

    def attn(self, qkv, B, T, d):
        if self.R is not None and qkv.dtype == torch.float32 and self.ops.head_dim == 64 and not self.pad["T"]:   # the library's exact-float32 attention
            return self.R.attention_f32(qkv, self.ops.heads, self.ops.scaling)
        return _sdpa(qkv, B, T, d, self.ops, self.pad["T"] or T)

    def add_ln(self, x, y, norm):
        if self.hip:   # residual add + LayerNorm as a single HIP launch (vd3d_add_layernorm)
            return self.R.add_layernorm(x, y, norm)
        s = x if y is None else x + y
        return s, norm(s)


class _SplitBackend(_LibraryBackend):
    """"bf16x3" / "fp16x2": the weights are split and packed once, here; fc1 takes the exact GELU in its epilogue (any other activation runs behind it).  ``keyword``
    names the DepthPipe keyword that asked (``gemm`` / ``encoders``) in the refusal.  The modes are float32 only, so there is no query padding on this path."""
    hip = True   # past begin's check every residual add + LayerNorm is the renderer's launch

    def __init__(self, renderer, ops, mode, keyword):
        self.R, self.ops, self.mode, self.keyword = renderer, ops, mode, keyword
        self.gelu = bool(isinstance(ops.act, torch.nn.GELU) and getattr(ops.act, "approximate", "none") == "none" or type(ops.act).__name__ == "GELUActivation")
        self.w = {key: (renderer.gemm_x3_pack(w, mode), w.shape[0], b)
                  for key, w, b in (("qkv", ops.wqkv, ops.bqkv), ("wo", ops.wo, ops.bo), ("fc1", ops.w1, ops.b1), ("w2", ops.w2, ops.b2))}

    def begin(self, x):
        d = x.shape[-1]
        if not (x.dtype == torch.float32 and x.is_contiguous() and d in HIDDEN_SIZES):
            raise NotImplementedError(f"{self.keyword}={self.mode!r}: hidden size {d} / dtype {x.dtype} not built (float32, 384 / 768 / 1024) -- refusing to fall back silently")

    def lin(self, key, t, gelu=False):
        img, n, bias = self.w[key]
        return self.R.linear_x3(t if t.is_contiguous() else t.contiguous(), img, n, bias, gelu=gelu, mode=self.mode)

    def attn(self, qkv, B, T, d):
        if self.ops.head_dim == 64:   # the library's split attention (every DINOv2 size and ViT-L/16 have 64-wide heads)
            return self.R.attention_x3(qkv, self.ops.heads, self.ops.scaling, mode=self.mode)
        return _sdpa(qkv, B, T, d, self.ops, T)


def _block(be, ops, stash, nxt):
    """``x -> block(x)``, the residual stream as the stock layer returns it: LayerNorm 1 (taken from ``stash`` where the block before left it for this very tensor),
    q / k / v as one GEMM, attention, output projection, residual add + LayerNorm 2, fc1 / activation / fc2, and the second residual add -- together with the NEXT
    block's first LayerNorm ``nxt``, left in ``stash``, unless this is the encoder's last block."""
    def fwd(x):
        be.begin(x)
        B, T, d = x.shape
        h = stash["h"] if stash["x"] is x else be.add_ln(x, None, ops.norm1)[1]
        stash["x"] = stash["h"] = None
        o = be.attn(be.lin("qkv", h), B, T, d)
        x, h = be.add_ln(x, be.lin("wo", o), ops.norm2)
        m = be.lin("w2", be.lin("fc1", h, gelu=True) if be.gelu else ops.act(be.lin("fc1", h)))
        if nxt is None:
            return x + m
        x, hn = be.add_ln(x, m, nxt)
        stash["x"], stash["h"] = x, hn
        return x
    return fwd


def _split_block(renderer, ops, stash, nxt, mode, keyword="gemm"):
    """One block in the split arithmetic ``mode`` (``_SplitBackend``)."""
    return _block(_SplitBackend(renderer, ops, mode, keyword), ops, stash, nxt)


def encoder_blocks(renderer, operands_list, mode="f32", keyword="gemm", pad_state=None) -> list:
    """The layers of ONE encoder (``BlockOperands`` each, in order) as block functions ``x -> x`` in ``mode`` ("f32": the library back-end, ``renderer`` may be None;
    "bf16x3" / "fp16x2": the split back-end).  The blocks share one stash of their own; the modules the operands came from are left as they are."""
    ops = list(operands_list)
    stash = {"x": None, "h": None}   # (x, LayerNorm1(x)) computed by the PREVIOUS block's fused add + LayerNorm
    nxts = [o.norm1 for o in ops[1:]] + [None]
    if mode == "f32":
        return [_block(_LibraryBackend(renderer, o, pad_state), o, stash, nxt) for o, nxt in zip(ops, nxts)]
    return [_split_block(renderer, o, stash, nxt, mode, keyword) for o, nxt in zip(ops, nxts)]
