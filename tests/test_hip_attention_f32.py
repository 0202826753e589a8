"""GPU tests (-m gpu) of the exact-float32 attention (vd3d_attention_f32, csrc/vd3d_attn.hip k_attn_f32): the default depth leg's attention.

A floating-point kernel in the arithmetic class of PyTorch's float32 scaled_dot_product_attention (AOTriton): float32 operands on the float32-input matrix
cores, float32 online softmax.  The bar is stated against FLOAT64, beside AOTriton's float32 kernel on the same operands; then known answers, determinism
under load, and that the float32 DINOv2 pipe routes through it (and nothing else does)."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("B,T,H", [(2, 31, 3), (1, 64, 2), (2, 77, 4), (1, 257, 6), (3, 300, 2), (2, 1370, 6), (1, 2443, 12)])
def test_attention_f32_is_float32_faithful(R, B, T, H):
    """vd3d_attention_f32 against float64 softmax attention, beside AOTriton's float32 kernel on the same operands: RMS error <= 1.25 x AOTriton's, the maximum
    over all elements <= 2 x AOTriton's.  Token counts that are not multiples of the 64-row KV tile / 32-query wave / 256-query workgroup (the last KV tile is
    masked, its DMA rows clamped to T - 1), DINOv2's 1370 (1080p) and 2443 (4K) among them; per-query temperatures (nearly one-hot softmax for some queries,
    flat for others) and scaled values."""
    D = 64
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + T)
    qkv = torch.randn(B, T, 3, H, D, device="cuda", generator=g)
    qkv[:, :, 0] *= torch.exp(torch.randn(B, T, H, 1, device="cuda", generator=g))        # per-query temperature
    qkv[:, :, 2] *= 3.0
    scale = D ** -0.5
    out = R.attention_f32(qkv.view(B, T, 3 * H * D), H, scale)
    assert out.shape == (B, T, H * D) and bool(torch.isfinite(out).all())
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    ref = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale, dim=-1) @ v.double()
    ref = ref.transpose(1, 2).reshape(B, T, H * D)
    o32 = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(B, T, H * D)
    e, e32 = float((out.double() - ref).abs().max()), float((o32.double() - ref).abs().max())
    r = float((out.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    r32 = float((o32.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"B {B} T {T} H {H}: max {e:.3g} vs {e32:.3g} ({e / e32:.2f}x), rms {r:.3g} vs {r32:.3g} ({r / r32:.2f}x)")
    assert e <= max(2.0 * e32, 1e-6 * float(ref.abs().max())), (e, e32)
    assert r <= 1.25 * r32 + 1e-8, (r, r32)
    assert torch.equal(R.attention_f32(qkv.view(B, T, 3 * H * D), H, scale), out)   # no state between calls


def test_attention_f32_full_batch_is_deterministic_under_load(R):
    """A batch that fills the chip several times over (16 frames x 12 heads x 1370 tokens), five times in a row: identical bits every time, and frame 0 equal
    to the same frame computed alone (an LDS ring race shows as a difference here, under load, and nowhere in the small cases)."""
    B, T, H, D = 16, 1370, 12, 64
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.randn(B, T, 3 * H * D, device="cuda", generator=g)
    out = R.attention_f32(qkv, H, 0.125)
    for _ in range(5):
        assert torch.equal(R.attention_f32(qkv, H, 0.125), out)
    assert torch.equal(R.attention_f32(qkv[:1].contiguous(), H, 0.125), out[:1])


def test_attention_f32_known_answers(R):
    """(i) one key: softmax is 1, the output is v itself -- bit for bit.  (ii) identical keys, integer values: the output is the exact mean over 128 tokens
    (every probability exp2(0) = 1, a sum of integers, one division by 128).  (iii) a query that matches one key by a wide margin copies that key's value."""
    D, H = 64, 2
    g = torch.Generator(device="cuda").manual_seed(3)
    qkv = torch.randn(2, 1, 3, H, D, device="cuda", generator=g)
    out = R.attention_f32(qkv.view(2, 1, -1), H, 0.125)
    assert torch.equal(out.view(2, 1, H, D), qkv[:, :, 2])
    T = 128
    qkv = torch.randn(1, T, 3, H, D, device="cuda", generator=g)
    qkv[:, :, 1] = qkv[:, :1, 1]                                   # every key the same -> uniform softmax
    vi = torch.randint(-8, 9, (1, T, H, D), device="cuda", generator=g).float()
    qkv[:, :, 2] = vi
    out = R.attention_f32(qkv.view(1, T, -1), H, 0.125).view(1, T, H, D)
    assert torch.equal(out, vi.mean(dim=1, keepdim=True).expand(1, T, H, D))
    T = 200
    qkv = torch.randn(1, T, 3, H, D, device="cuda", generator=g) * 0.01
    e = torch.zeros(D, device="cuda"); e[5] = 1.0
    qkv[0, :, 0] = e * 64.0                                        # every query points at key 17 with logit 64 * 64 * 0.125 = 512 above the rest
    qkv[0, 17, 1] = e * 64.0
    out = R.attention_f32(qkv.view(1, T, -1), H, 0.125).view(1, T, H, D)
    assert torch.allclose(out, qkv[:, 17:18, 2].expand(1, T, H, D), rtol=0, atol=1e-30)


def test_attention_f32_refuses_what_it_does_not_build(R):
    """D != 64, an empty shape, B * H > 65 535 and misaligned pointers are VD3D_E_UNSUPPORTED from the C entry point (no silent fallback)."""
    L = R._L
    q = torch.zeros(2, 8, 3 * 2 * 64, device="cuda")
    o = torch.empty(2, 8, 2 * 64, device="cuda")
    unsupported = -4   # VD3D_E_UNSUPPORTED
    assert L.vd3d_attention_f32(R._ctx, q.data_ptr(), 2, 8, 2, 64, 0.125, o.data_ptr()) == 0
    torch.cuda.synchronize()
    assert L.vd3d_attention_f32(R._ctx, q.data_ptr(), 2, 8, 4, 32, 0.125, o.data_ptr()) == unsupported
    assert L.vd3d_attention_f32(R._ctx, q.data_ptr(), 0, 8, 2, 64, 0.125, o.data_ptr()) == unsupported
    assert L.vd3d_attention_f32(R._ctx, q.data_ptr(), 2, 0, 2, 64, 0.125, o.data_ptr()) == unsupported
    assert L.vd3d_attention_f32(R._ctx, q.data_ptr(), 65536, 8, 1, 64, 0.125, o.data_ptr()) == unsupported
    assert L.vd3d_attention_f32(R._ctx, q.data_ptr() + 4, 1, 8, 2, 64, 0.125, o.data_ptr()) == unsupported
    assert L.vd3d_attention_f32(R._ctx, q.data_ptr(), 1, 8, 2, 64, 0.125, o.data_ptr() + 4) == unsupported
    with pytest.raises(NotImplementedError):
        R.attention_f32(torch.zeros(1, 8, 3 * 4 * 32, device="cuda"), 4, 0.125)


def _count(monkeypatch, R):
    calls = dict(attention_f32=0, sdpa=0)
    orig_a, orig_s = R.attention_f32, F.scaled_dot_product_attention

    def a(*args, **kw):
        calls["attention_f32"] += 1
        return orig_a(*args, **kw)

    def s(*args, **kw):
        calls["sdpa"] += 1
        return orig_s(*args, **kw)

    monkeypatch.setattr(R, "attention_f32", a)
    monkeypatch.setattr(F, "scaled_dot_product_attention", s)
    return calls


def test_float32_pipe_runs_the_library_attention_and_bf16_keeps_sdpa(R, monkeypatch):
    """DA-V2-Small in float32 with a renderer: attention_f32 once per layer (12), SDPA never.  The bfloat16 pipe still runs SDPA (with token padding), and
    attention_f32 never."""
    import numpy as np

    from visiondepth3d_amd.depth import DepthPipe
    frames = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (2, 140, 252, 3), dtype=np.uint8)).cuda()
    calls = _count(monkeypatch, R)
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.float32, renderer=R)
    pipe.infer_bgr_u8(frames, raw=True)
    torch.cuda.synchronize()
    assert calls == dict(attention_f32=12, sdpa=0), calls
    calls.update(attention_f32=0, sdpa=0)
    pipe = DepthPipe("depth-anything-v2-small", device="cuda", dtype=torch.bfloat16, renderer=R)
    pipe.infer_bgr_u8(frames, raw=True)
    torch.cuda.synchronize()
    assert calls["attention_f32"] == 0 and calls["sdpa"] == 12, calls
