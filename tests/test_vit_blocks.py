"""CPU checks of visiondepth3d_amd/vit_blocks.py, the one transformer-block rewrite behind DepthPipe's DINOv2, DPT-ViT and DepthPro encoders: operand
construction, the block skeleton on both back-ends against the stock transformers layers, the stash that hands a block's first LayerNorm over from the block
before, and the split back-end's refusals.  The renderer is the torch double of tests/renderer_doubles.py, or None (the plain ATen path of a CPU pipe).

Geometry: hidden 384 in 6 heads (the smallest the kernels are built for), THREE layers -- a first, a middle and a last block: the stash starts, is handed over and
ends -- batch 2, 7 tokens (CLS + a 2 x 3 grid) and 5."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
F = torch.nn.functional

from renderer_doubles import SplitDouble   # noqa: E402
from visiondepth3d_amd import vit_blocks as vb   # noqa: E402
from visiondepth3d_amd.depth import synthetic_weights_   # noqa: E402

L, D, HEADS, B = 3, 384, 6, 2
TOKENS = (7, 5)


def _dinov2(dtype=torch.float32):
    cfg = transformers.Dinov2Config(hidden_size=D, num_hidden_layers=L, num_attention_heads=HEADS, mlp_ratio=2, image_size=28, patch_size=14)
    m = transformers.Dinov2Model(cfg).eval()
    synthetic_weights_(m, 3)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for lay in m.encoder.layer:   # LayerScale that is neither one nor uniform: a fold that misses a row, or folds the wrong lambda, shows
            lay.layer_scale1.lambda1.copy_(torch.rand(D, generator=g) * 1.5 + 0.25)
            lay.layer_scale2.lambda1.copy_(torch.rand(D, generator=g) * 1.5 + 0.25)
    return m.to(dtype)


def _dpt(**kw):
    cfg = transformers.DPTConfig(hidden_size=D, num_hidden_layers=L, num_attention_heads=HEADS, intermediate_size=768, image_size=32, patch_size=16,
                                 backbone_out_indices=[0, 1, 2], neck_hidden_sizes=[16, 32, 64], **kw)
    m = transformers.DPTModel(cfg, add_pooling_layer=False).eval()
    synthetic_weights_(m, 4)
    return m


FAMILIES = {"dinov2": (_dinov2, vb.dinov2_operands), "dpt_vit": (_dpt, vb.dpt_vit_operands)}


@pytest.fixture(scope="module")
def stock():
    """Per family: the model, its operands and, per token count, (input, the stock encoder's output) -- computed once, read by every test."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = {}
    for fam, (build, operands) in FAMILIES.items():
        m = build()
        runs = {}
        for T in TOKENS:
            x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(T))
            with torch.no_grad():
                runs[T] = (x, m.encoder(x).last_hidden_state)
        out[fam] = (m, [operands(lay) for lay in m.encoder.layer], runs)
    return out


def _run(blocks, x):
    with torch.no_grad():
        for blk in blocks:
            x = blk(x)
    return x


def _close(got, exp):
    assert got.shape == exp.shape
    return float((got - exp).abs().max() / exp.abs().max()) < 1e-5


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("mode", ["bf16x3", "fp16x2"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_split_blocks_are_the_stock_layers(stock, fam, mode, T):
    _, ops, runs = stock[fam]
    x, exp = runs[T]
    R = SplitDouble()
    assert _close(_run(vb.encoder_blocks(R, ops, mode), x.clone()), exp)
    # the first block's LayerNorm alone, two add + LayerNorm launches per block, the last block's second residual add stands alone: 1 + 2 L - 1
    assert (R.calls["linear_x3"], R.calls["attention_x3"], R.calls["add_layernorm"], R.calls["attention_f32"]) == (4 * L, L, 2 * L, 0), R.calls


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_library_blocks_with_a_renderer_are_the_stock_layers(stock, fam, T):
    _, ops, runs = stock[fam]
    x, exp = runs[T]
    R = SplitDouble()
    assert _close(_run(vb.encoder_blocks(R, ops, "f32"), x.clone()), exp)
    assert (R.calls["attention_f32"], R.calls["add_layernorm"], R.calls["linear_x3"], R.calls["attention_x3"]) == (L, 2 * L, 0, 0), R.calls


def _plain_fused_layers(model, x):
    """The fused Dinov2Layer of a pipe without a renderer, stated straight: folded weights, one QKV GEMM, SDPA, x + a, x + fc2(act(fc1(LN2(x))))."""
    for lay in model.encoder.layer:
        att, out, mlp = lay.attention.attention, lay.attention.output.dense, lay.mlp
        wqkv = torch.cat([att.query.weight, att.key.weight, att.value.weight], 0)
        bqkv = torch.cat([att.query.bias, att.key.bias, att.value.bias], 0)
        l1, l2 = lay.layer_scale1.lambda1.float(), lay.layer_scale2.lambda1.float()
        wo, bo = (out.weight.float() * l1[:, None]).to(out.weight.dtype), (out.bias.float() * l1).to(out.bias.dtype)
        w2, b2 = (mlp.fc2.weight.float() * l2[:, None]).to(mlp.fc2.weight.dtype), (mlp.fc2.bias.float() * l2).to(mlp.fc2.bias.dtype)
        Bn, T, d = x.shape
        qkv = F.linear(lay.norm1(x), wqkv, bqkv).view(Bn, T, 3, HEADS, d // HEADS)
        q, k, v = qkv[:, :, 0].transpose(1, 2), qkv[:, :, 1].transpose(1, 2), qkv[:, :, 2].transpose(1, 2)
        o = F.scaled_dot_product_attention(q, k, v, scale=att.scaling).transpose(1, 2).reshape(Bn, T, d)
        x = x + F.linear(o, wo, bo)
        x = x + F.linear(mlp.activation(F.linear(lay.norm2(x), mlp.fc1.weight, mlp.fc1.bias)), w2, b2)
    return x


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_library_blocks_without_a_renderer_are_the_plain_aten_operators(dtype, T):
    """No renderer: the same ATen calls on the same values as the straight statement, so the same bits -- in float32 and in bf16."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m = _dinov2(dtype)
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(T)).to(dtype)
    got = _run(vb.encoder_blocks(None, [vb.dinov2_operands(lay) for lay in m.encoder.layer], "f32"), x.clone())
    with torch.no_grad():
        exp = _plain_fused_layers(m, x)
    assert got.dtype == dtype and torch.equal(got, exp)


def test_operands(stock):
    m, ops, _ = stock["dinov2"]
    for lay, o in zip(m.encoder.layer, ops):
        att = lay.attention.attention
        assert torch.equal(o.wqkv, torch.cat([att.query.weight, att.key.weight, att.value.weight])) and o.wqkv.shape == (3 * D, D)
        assert torch.equal(o.bqkv, torch.cat([att.query.bias, att.key.bias, att.value.bias]))
        for (w, b), lin, lam in (((o.wo, o.bo), lay.attention.output.dense, lay.layer_scale1.lambda1), ((o.w2, o.b2), lay.mlp.fc2, lay.layer_scale2.lambda1)):
            assert torch.equal(w, (lin.weight.double() * lam.double()[:, None]).float()) and torch.equal(b, (lin.bias.double() * lam.double()).float())
            assert w.is_contiguous() and not w.requires_grad
        assert o.w1 is lay.mlp.fc1.weight and o.b1 is lay.mlp.fc1.bias and o.norm1 is lay.norm1 and o.norm2 is lay.norm2 and o.act is lay.mlp.activation
        assert (o.heads, o.head_dim, o.scaling) == (HEADS, 64, 64 ** -0.5)
    lay = _dpt(qkv_bias=False).encoder.layer[0]
    o = vb.dpt_vit_operands(lay)
    assert o.bqkv is None and o.wqkv.shape == (3 * D, D)
    assert o.wo is lay.attention.output.dense.weight and o.w2 is lay.output.dense.weight and o.norm1 is lay.layernorm_before and o.norm2 is lay.layernorm_after
    assert stock["dpt_vit"][1][0].bqkv.shape == (3 * D,)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_a_stash_is_taken_only_by_the_tensor_it_was_left_for(stock, mode):
    _, ops, runs = stock["dinov2"]
    x, _ = runs[7]
    R = SplitDouble()
    blocks = vb.encoder_blocks(R, ops, mode)
    _run(blocks, x.clone())
    assert R.calls["add_layernorm"] == 2 * L
    with torch.no_grad():
        x1 = blocks[0](x.clone())                 # a fresh tensor after a whole forward: LayerNorm 1 computed, then the two add + LayerNorm launches
        assert R.calls["add_layernorm"] == 2 * L + 3
        taken = blocks[1](x1)                     # the tensor the stash was left for: taken
        assert R.calls["add_layernorm"] == 2 * L + 3 + 2
        blocks[0](x.clone())                      # leaves a stash for ITS output ...
        n = R.calls["add_layernorm"]
        computed = blocks[1](x1.clone())          # ... which an equal tensor that is not that output must not take
        assert R.calls["add_layernorm"] == n + 3
        assert torch.equal(computed, taken)
        n = R.calls["add_layernorm"]
        blocks[2](taken.clone())                  # and the mismatch cleared it: nothing stale is left for a later call
        assert R.calls["add_layernorm"] == n + 2  # (the last block: LayerNorm 1, add + LayerNorm 2, a plain add)


def test_split_refusals_keep_their_text(stock):
    _, ops, _ = stock["dinov2"]
    gemm = vb.encoder_blocks(SplitDouble(), ops, "bf16x3")[0]
    enc = vb.encoder_blocks(SplitDouble(), ops, "fp16x2", keyword="encoders")[0]
    with pytest.raises(NotImplementedError) as e:
        gemm(torch.zeros(B, 5, D, dtype=torch.bfloat16))
    assert str(e.value) == "gemm='bf16x3': hidden size 384 / dtype torch.bfloat16 not built (float32, 384 / 768 / 1024) -- refusing to fall back silently"
    with pytest.raises(NotImplementedError) as e:
        gemm(torch.zeros(B, 5, 320))
    assert str(e.value) == "gemm='bf16x3': hidden size 320 / dtype torch.float32 not built (float32, 384 / 768 / 1024) -- refusing to fall back silently"
    with pytest.raises(NotImplementedError) as e:
        enc(torch.zeros(B, 5, 320))
    assert str(e.value) == "encoders='fp16x2': hidden size 320 / dtype torch.float32 not built (float32, 384 / 768 / 1024) -- refusing to fall back silently"
    with pytest.raises(NotImplementedError, match="hidden size 384 / dtype torch.float32 not built"):
        gemm(torch.zeros(B, D, 5).transpose(1, 2))   # not contiguous
