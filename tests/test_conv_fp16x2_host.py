"""Host-side tests (no GPU) of the fp16x2 tile convolutions vd3d_conv3x3_s1_x2 / vd3d_conv3x3_s2_x2 (csrc/vd3d_conv_x2t.hip) and of the keywords that route
them, DepthPipe(gemm="fp16x2", conv="fp16x2"[, self_contained=True]): the byte rule of the weight images and the shapes that are refused, the export list, a
numpy statement of both weight images (per-channel power-of-two exponent, round-to-nearest two-term split, K-step order, channel scales, zero page), and the
keyword refusals with their wording.

``x2_image_reference`` is what tests/test_hip_conv_fp16x2.py holds the device packers to, every byte."""
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_self_contained_host import s2_schedule   # noqa: E402  (the stride-2 step order is the bf16x3 kernel's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vd3d_conv3x3_s1_x2_weight_bytes", "vd3d_conv3x3_s1_x2_pack_weights", "vd3d_conv3x3_s1_x2",
       "vd3d_conv3x3_s2_x2_weight_bytes", "vd3d_conv3x3_s2_x2_pack_weights", "vd3d_conv3x3_s2_x2")
S1_TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]          # stride 1: the taps of a chunk row-major
S2_TAPS = [(ky, kx) for *_, ky, kx in s2_schedule()]                # stride 2: sub-pixel order, no tap on a zero weight


def x2_exponent(W: np.ndarray) -> np.ndarray:
    """include/vd3d.h: e(oc) = 13 - floor(log2 max |W[oc]|), read from the float32 exponent field (a subnormal maximum counts as 2^-127), clamped to
    [-100, 100]; 0 for an all-zero or non-finite channel."""
    mx = np.abs(np.ascontiguousarray(W, np.float32)).reshape(W.shape[0], -1).max(axis=1)
    ef = ((mx.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    return np.where((mx > 0) & (ef != 255), np.clip(140 - ef, -100, 100), 0)


def fp16x2_terms(v: np.ndarray):
    """The round-to-nearest two-term split (vd3d_x3.h): h1 = fp16(v), h2 = fp16(v - h1); numpy's float32 -> float16 conversion rounds to nearest even."""
    v = np.ascontiguousarray(v, np.float32)
    h1 = v.astype(np.float16)
    h2 = (v - h1.astype(np.float32)).astype(np.float16)
    return h1, h2


def x2_image_reference(W: np.ndarray, stride: int) -> np.ndarray:
    """The weight image of vd3d_conv3x3_s{stride}_x2 for W[Cout][Cin][3][3], as bytes: [slice Cout / CK][step 9 Cin / 16][term 2][k-half 2][oc CK][8 fp16] with
    CK = min(Cout, 128) and the terms those of 2^e(oc) W, then colscale[Cout] = 2^-e as float32, then the 64-byte zero page."""
    Cout, Cin = W.shape[:2]
    CK = min(Cout, 128)
    e = x2_exponent(W)
    Ws = (W.astype(np.float32) * np.ldexp(np.float32(1), e).astype(np.float32)[:, None, None, None]).astype(np.float32)   # a power of two: exact
    taps = S1_TAPS if stride == 1 else S2_TAPS
    img = np.zeros((Cout // CK, (Cin // 16) * 9, 2, 2, CK, 8), np.float16)
    for c16 in range(Cin // 16):
        for j, (ky, kx) in enumerate(taps):
            for t, term in enumerate(fp16x2_terms(Ws[:, c16 * 16:(c16 + 1) * 16, ky, kx])):          # [Cout][16]
                img[:, c16 * 9 + j, t] = term.reshape(Cout // CK, CK, 2, 8).transpose(0, 2, 1, 3)
    cs = np.ldexp(np.float32(1), -e).astype(np.float32)
    return np.concatenate([img.reshape(-1).view(np.uint8), cs.view(np.uint8), np.zeros(64, np.uint8)])


def test_weight_bytes_rule_and_refused_shapes():
    from visiondepth3d_amd import _lib
    L = _lib.lib()
    rule = lambda cin, cout: cin // 16 * 9 * cout * 64 + 4 * cout + 64   # noqa: E731  (include/vd3d.h)
    for cin in (16, 48, 256, 1024):
        for cout in (32, 64, 128, 256):
            assert L.vd3d_conv3x3_s1_x2_weight_bytes(cin, cout) == rule(cin, cout), (cin, cout)
        for cout in (128, 256, 384, 768, 1024):
            assert L.vd3d_conv3x3_s2_x2_weight_bytes(cin, cout) == rule(cin, cout), (cin, cout)
    for cin in (24, 0, -16):
        assert L.vd3d_conv3x3_s1_x2_weight_bytes(cin, 64) < 0 and L.vd3d_conv3x3_s2_x2_weight_bytes(cin, 128) < 0, cin
    for cout in (16, 96, 512):
        assert L.vd3d_conv3x3_s1_x2_weight_bytes(64, cout) < 0, cout
    for cout in (64, 192, 1152):
        assert L.vd3d_conv3x3_s2_x2_weight_bytes(64, cout) < 0, cout


def test_exports():
    from visiondepth3d_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    for name in NEW:
        assert re.search(r"\bint(64_t)? " + name + r"\(", hdr) and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.vd3d_abi_version() == 6
    assert "vd3d_conv_x2t.hip" in open(os.path.join(ROOT, "visiondepth3d_amd", "csrc", "Makefile")).read()


def test_exponent_rule_puts_the_largest_weight_in_the_top_binade():
    W = np.zeros((8, 16, 3, 3), np.float32)
    W[0, 3, 1, 1] = 1.0            # 2^0 -> e 13
    W[1, 0, 0, 0] = -0.7           # floor(log2) = -1 -> e 14
    W[2, 5, 2, 2] = 2.0 ** 14      # e -1
    W[3, 1, 0, 1] = 2.0 ** -126    # e clamps to 100
    W[4, 1, 0, 1] = 1e-41          # subnormal: clamped too
    W[5, 0, 0, 0] = np.float32(2.0) - np.float32(2.0 ** -23)   # just below 2: floor(log2) = 0, where a rounded log2f would say 1
    W[6, 0, 0, 0] = np.inf         # non-finite: e 0
    assert x2_exponent(W).tolist() == [13, 14, -1, 100, 100, 13, 0, 0]
    for oc in (0, 1, 2, 5):
        m = float(np.abs(W[oc]).max()) * 2.0 ** int(x2_exponent(W)[oc])
        assert 2.0 ** 13 <= m < 2.0 ** 14


def test_split_rounds_to_nearest_and_keeps_22_bits():
    v = np.array([4097.0, 4099.0, 1.0 + 2.0 ** -11 + 2.0 ** -12, 0.3, -1234.567], np.float32)
    h1, h2 = fp16x2_terms(v)
    assert float(h1[0]) == 4096.0 and float(h2[0]) == 1.0 and float(h1[1]) == 4100.0 and float(h2[1]) == -1.0
    assert float(h1[2]) == 1.0 + 2.0 ** -10 and float(h2[2]) < 0     # rounded UP to the next fp16, a negative second term: truncation would give 1.0 and +
    back = h1.astype(np.float64) + h2.astype(np.float64)
    assert np.all(np.abs(back - v.astype(np.float64)) <= 2.0 ** -22 * np.abs(v))


@pytest.mark.parametrize("stride,Cout", [(1, 32), (1, 64), (1, 256), (2, 128), (2, 384)])
def test_image_reference_decodes_to_the_weights_in_step_order(stride, Cout):
    """The image's two terms times colscale give W back to 22 bits at the position the kernel reads: slice oc // CK, step 9 c16 + j, k-half (ci % 16) // 8,
    row oc % CK; the byte count is the header's; the zero page is zero."""
    from visiondepth3d_amd import _lib
    rng = np.random.default_rng(7 + Cout)
    Cin = 48
    W = (rng.standard_normal((Cout, Cin, 3, 3)) * 0.05 * np.exp(rng.standard_normal((Cout, 1, 1, 1)) * 3)).astype(np.float32)
    raw = x2_image_reference(W, stride)
    fn = _lib.lib().vd3d_conv3x3_s1_x2_weight_bytes if stride == 1 else _lib.lib().vd3d_conv3x3_s2_x2_weight_bytes
    assert raw.size == fn(Cin, Cout) and not raw[-64:].any()
    CK = min(Cout, 128)
    nstep = Cin // 16 * 9 * Cout * 64
    img = raw[:nstep].view(np.float16).reshape(Cout // CK, Cin // 16 * 9, 2, 2, CK, 8).astype(np.float64)
    cs = raw[nstep:nstep + 4 * Cout].view(np.float32).astype(np.float64)
    assert np.array_equal(cs, 2.0 ** -x2_exponent(W).astype(np.float64))
    assert np.isfinite(img).all() and np.abs(img[:, :, 0]).max() <= 2.0 ** 14   # (a weight just below 2^14 rounds up to it)
    tot = img[:, :, 0] + img[:, :, 1]
    for c16 in range(Cin // 16):
        for j, (ky, kx) in enumerate(S1_TAPS if stride == 1 else S2_TAPS):
            got = tot[:, c16 * 9 + j].transpose(0, 2, 1, 3).reshape(Cout, 16) * cs[:, None]
            want = W[:, c16 * 16:(c16 + 1) * 16, ky, kx].astype(np.float64)
            # 22 bits of each weight, or the last place of a subnormal second term (2^-24 in the scaled domain) for the small ones
            tol = np.maximum(2.0 ** -22 * np.abs(want), 2.0 ** -24 * cs[:, None])
            assert np.all(np.abs(got - want) <= tol), (c16, j)


def test_keyword_refusals_and_defaults():
    from visiondepth3d_amd.depth import CONV_X2_MIN_TILES, DepthPipe
    name = "depth-anything-v2-small"
    cpu = dict(device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="conv"):                                          # the convolution half needs its own gemm mode
        DepthPipe(name, gemm="f32", conv="fp16x2", **cpu)
    with pytest.raises(ValueError, match="conv"):
        DepthPipe(name, gemm="bf16x3", conv="fp16x2", **cpu)
    with pytest.raises(ValueError, match="conv"):
        DepthPipe(name, gemm="fp16x2", conv="bf16x3", **cpu)
    with pytest.raises(ValueError, match="gemm"):                                          # an unknown gemm is still named first
        DepthPipe(name, gemm="nonsense", conv="fp16x2", **cpu)
    with pytest.raises(ValueError, match="renderer"):                                      # a valid pair still needs the GPU and a renderer
        DepthPipe(name, gemm="fp16x2", conv="fp16x2", **cpu)
    ok = dict(device="cuda", dtype=torch.float32, gemm="fp16x2", conv="fp16x2", renderer=object(), self_contained=True)
    with pytest.raises(ValueError, match="renderer"):
        DepthPipe(name, **dict(ok, renderer=None))
    with pytest.raises(ValueError, match="float32"):
        DepthPipe(name, **dict(ok, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="fuse_backbone=True"):
        DepthPipe(name, **dict(ok, fuse_backbone=False))
    # the wording tests/test_self_contained_host.py pins: the bf16x3 pair leads, the second pair is named behind it
    with pytest.raises(ValueError, match=r"self_contained=True needs gemm='bf16x3', conv='bf16x3' \(or gemm='fp16x2', conv='fp16x2'\)$"):
        DepthPipe(name, **dict(ok, conv=None))
    with pytest.raises(ValueError, match=r"self_contained=True needs gemm='bf16x3', conv='bf16x3' \(or gemm='fp16x2', conv='fp16x2'\), fuse_backbone=True"):
        DepthPipe(name, **dict(ok, gemm="f32", conv=None, fuse_backbone=False))
    with pytest.raises(ValueError, match=r"self_contained=True needs conv='bf16x3'$"):
        DepthPipe(name, **dict(ok, gemm="bf16x3", conv=None))
    with pytest.raises(ValueError, match=r"or gemm='fp16x2', conv='fp16x2'"):            # a mixed pair is no pair
        DepthPipe(name, **dict(ok, conv="bf16x3"))
    p = inspect.signature(DepthPipe.__init__).parameters
    assert p["gemm"].default == "f32" and p["conv"].default is None and p["self_contained"].default is False
    assert isinstance(CONV_X2_MIN_TILES, int) and CONV_X2_MIN_TILES > 0


def test_dpt_large_stays_refused_by_name_under_the_fp16x2_pair():
    transformers = pytest.importorskip("transformers")
    from visiondepth3d_amd.depth import DepthPipe
    cfg = transformers.DPTConfig(hidden_size=64, num_hidden_layers=4, num_attention_heads=1, intermediate_size=128, image_size=32, patch_size=16,
                                 backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[16, 16, 16, 16], fusion_hidden_size=16, readout_type="project")
    dpt = transformers.DPTForDepthEstimation(cfg).eval()
    with pytest.raises(NotImplementedError, match=r"self_contained=True: 'dpt-large' \(DPTForDepthEstimation"):
        DepthPipe("dpt-large", model=dpt, device="cuda", dtype=torch.float32, gemm="fp16x2", conv="fp16x2", renderer=object(), self_contained=True)
