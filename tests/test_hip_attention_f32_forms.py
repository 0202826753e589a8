"""GPU tests (-m gpu) of the two forms of the exact-float32 attention kernel (csrc/vd3d_attn.hip k_attn_f32<NW, NS>, vd3d_attention_f32_form): 8 waves / 256
queries per workgroup with a ring of three stages, and 4 waves / 128 queries with a ring of two, two workgroups per CU, padding waves that skip their matrix work.

Per query both forms run the same operations in the same order, so the main test is BIT IDENTITY of form 4 against form 8 at every size where the 4-wave
form takes another path (a padding wave in a live workgroup, the workgroup edge, the ring wrapping, the XCD grouping with empty slots).  Then form 4 on its own:
float32 faithfulness against float64 beside AOTriton (the bars of test_hip_attention_f32.py), the known answers, determinism under load, the refusals."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

D = 64
INVALID, UNSUPPORTED = -1, -4   # VD3D_E_INVALID, VD3D_E_UNSUPPORTED


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _operands(B, T, H):
    """The operand recipe of test_hip_attention_f32.py: per-query temperatures (nearly one-hot softmax for some queries, flat for others), v x 3, seeded by shape."""
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + T)
    qkv = torch.randn(B, T, 3, H, D, device="cuda", generator=g)
    qkv[:, :, 0] *= torch.exp(torch.randn(B, T, H, 1, device="cuda", generator=g))
    qkv[:, :, 2] *= 3.0
    return qkv


# T: 1 = one row, every DMA row clamped, one KV tile; 31 / 32 / 33 = below, at and past one wave's 32 queries (a padding wave inside a live workgroup);
# 64 / 65 = the KV tile edge (one tile -> two, the masked last tile); 127 / 128 / 129 = the 4-wave workgroup's edge (129: a second workgroup with one real row
# and three padding waves, three KV tiles: the two-stage ring wraps); 257 / 300 = the 8-wave edge, several workgroups per (b, h).
# (B, H): (1, 1) a single (b, h); (1, 3) fewer (b, h) than XCD slots; (3, 3) nine: a second XCD group with seven empty slots (the bh >= B * H return);
# (2, 8) two full XCD groups.
@pytest.mark.parametrize("B,H", [(1, 1), (1, 3), (3, 3), (2, 8)])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 65, 127, 128, 129, 257, 300])
def test_form_4_has_the_bits_of_form_8(R, T, B, H):
    qkv = _operands(B, T, H).view(B, T, 3 * H * D)
    s = D ** -0.5
    o8 = R.attention_f32(qkv, H, s, form=8)
    o4 = R.attention_f32(qkv, H, s, form=4)
    assert o4.shape == (B, T, H * D) and bool(torch.isfinite(o4).all())
    assert torch.equal(o4, o8)
    assert torch.equal(R.attention_f32(qkv, H, s), o8)   # form 0: one of the two


@pytest.mark.parametrize("B,T,H", [(2, 31, 3), (2, 77, 4), (1, 257, 6), (3, 300, 2)])
def test_form_4_is_float32_faithful(R, B, T, H):
    """Form 4 against float64 softmax attention beside AOTriton's float32 kernel on the same operands, with the bars and the formula of
    test_hip_attention_f32.py unchanged: max <= max(2 x AOTriton's, 1e-6 max|ref|), RMS <= 1.25 x AOTriton's + 1e-8."""
    qkv = _operands(B, T, H)
    scale = D ** -0.5
    out = R.attention_f32(qkv.view(B, T, 3 * H * D), H, scale, form=4)
    assert out.shape == (B, T, H * D) and bool(torch.isfinite(out).all())
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    ref = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * scale, dim=-1) @ v.double()
    ref = ref.transpose(1, 2).reshape(B, T, H * D)
    o32 = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(B, T, H * D)
    e, e32 = float((out.double() - ref).abs().max()), float((o32.double() - ref).abs().max())
    r = float((out.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    r32 = float((o32.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"form 4, B {B} T {T} H {H}: max {e:.3g} vs {e32:.3g} ({e / e32:.2f}x), rms {r:.3g} vs {r32:.3g} ({r / r32:.2f}x)")
    assert e <= max(2.0 * e32, 1e-6 * float(ref.abs().max())), (e, e32)
    assert r <= 1.25 * r32 + 1e-8, (r, r32)


def test_form_4_known_answers(R):
    """The three known answers of test_hip_attention_f32.py through form 4: (i) one key: the output is v itself, bit for bit; (ii) identical keys, integer
    values: the exact mean over 128 tokens; (iii) a query that matches one key by a wide margin copies that key's value."""
    H = 2
    g = torch.Generator(device="cuda").manual_seed(3)
    qkv = torch.randn(2, 1, 3, H, D, device="cuda", generator=g)
    out = R.attention_f32(qkv.view(2, 1, -1), H, 0.125, form=4)
    assert torch.equal(out.view(2, 1, H, D), qkv[:, :, 2])
    T = 128
    qkv = torch.randn(1, T, 3, H, D, device="cuda", generator=g)
    qkv[:, :, 1] = qkv[:, :1, 1]
    vi = torch.randint(-8, 9, (1, T, H, D), device="cuda", generator=g).float()
    qkv[:, :, 2] = vi
    out = R.attention_f32(qkv.view(1, T, -1), H, 0.125, form=4).view(1, T, H, D)
    assert torch.equal(out, vi.mean(dim=1, keepdim=True).expand(1, T, H, D))
    T = 200
    qkv = torch.randn(1, T, 3, H, D, device="cuda", generator=g) * 0.01
    e = torch.zeros(D, device="cuda"); e[5] = 1.0
    qkv[0, :, 0] = e * 64.0
    qkv[0, 17, 1] = e * 64.0
    out = R.attention_f32(qkv.view(1, T, -1), H, 0.125, form=4).view(1, T, H, D)
    assert torch.allclose(out, qkv[:, 17:18, 2].expand(1, T, H, D), rtol=0, atol=1e-30)


def test_form_4_full_batch_is_deterministic_under_load(R):
    """A batch that fills the chip several times over (16 frames x 12 heads x 1370 tokens, two workgroups per CU), three times: identical bits, frame 0 equal
    to the same frame computed alone, and everything equal to form 8 (a race in the two-stage ring shows here, under load, and nowhere in the small cases)."""
    B, T, H = 16, 1370, 12
    g = torch.Generator(device="cuda").manual_seed(11)
    qkv = torch.randn(B, T, 3 * H * D, device="cuda", generator=g)
    out = R.attention_f32(qkv, H, 0.125, form=4)
    for _ in range(2):
        assert torch.equal(R.attention_f32(qkv, H, 0.125, form=4), out)
    assert torch.equal(R.attention_f32(qkv[:1].contiguous(), H, 0.125, form=4), out[:1])
    assert torch.equal(R.attention_f32(qkv, H, 0.125, form=8), out)


def test_form_refusals(R):
    """A form outside {0, 4, 8} is VD3D_E_INVALID; D != 64, an empty shape, B * H > 65 535 and misaligned pointers stay VD3D_E_UNSUPPORTED through
    vd3d_attention_f32_form, whatever the form."""
    L = R._L
    q = torch.zeros(2, 8, 3 * 2 * 64, device="cuda")
    o = torch.empty(2, 8, 2 * 64, device="cuda")
    for form in (0, 4, 8):
        assert L.vd3d_attention_f32_form(R._ctx, q.data_ptr(), 2, 8, 2, 64, 0.125, o.data_ptr(), form) == 0
    torch.cuda.synchronize()
    for form in (-1, 1, 2, 3, 5, 16, 256):
        assert L.vd3d_attention_f32_form(R._ctx, q.data_ptr(), 2, 8, 2, 64, 0.125, o.data_ptr(), form) == INVALID, form
    from visiondepth3d_amd._lib import Vd3dError
    with pytest.raises(Vd3dError):
        R.attention_f32(q, 2, 0.125, form=2)
    for form in (0, 4, 8):
        assert L.vd3d_attention_f32_form(R._ctx, q.data_ptr(), 2, 8, 4, 32, 0.125, o.data_ptr(), form) == UNSUPPORTED
        assert L.vd3d_attention_f32_form(R._ctx, q.data_ptr(), 0, 8, 2, 64, 0.125, o.data_ptr(), form) == UNSUPPORTED
        assert L.vd3d_attention_f32_form(R._ctx, q.data_ptr(), 2, 0, 2, 64, 0.125, o.data_ptr(), form) == UNSUPPORTED
        assert L.vd3d_attention_f32_form(R._ctx, q.data_ptr(), 65536, 8, 1, 64, 0.125, o.data_ptr(), form) == UNSUPPORTED
        assert L.vd3d_attention_f32_form(R._ctx, q.data_ptr() + 4, 1, 8, 2, 64, 0.125, o.data_ptr(), form) == UNSUPPORTED
        assert L.vd3d_attention_f32_form(R._ctx, q.data_ptr(), 1, 8, 2, 64, 0.125, o.data_ptr() + 4, form) == UNSUPPORTED
