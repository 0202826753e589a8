"""Host-side tests (no GPU) of DepthPipe(self_contained=True) and the two kernels it adds: the keyword's refusals, the stride-2 weight image against a numpy
statement of the kernel's K-step schedule, the patch embedding and the transposed convolutions restated as GEMMs (numpy gather / scatter against F.unfold and
F.conv_transpose2d), the export list, and the register / LDS budget of the new instantiation from hipcc's own metadata.

The numpy statements here (``s2_schedule``, ``s2_image_reference``, ``patchify_reference``) are what tests/test_hip_self_contained.py holds the device kernels to,
bit for bit."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visiondepth3d_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ("vd3d_conv3x3_s2_x3_weight_bytes", "vd3d_conv3x3_s2_x3_pack_weights", "vd3d_conv3x3_s2_x3", "vd3d_patchify_f32")


# ---- the kernel's schedule, from k_conv_x3<K3S2>'s loop: per 16 input channels the four sub-pixels (sy, sx) of the space-to-depth view are staged in the order
# (0,0), (0,1), (1,0), (1,1); a staged sub-pixel holds input pixel (2 ty + sy, 2 tx + sx) at tile position (ty, tx).  A step reads the tile shifted by (dy, dx);
# output (q, r) reads input row 2 q - 1 + ky, and the shifted sub-row is 2 (q + dy) + sy, so ky = 2 dy + sy + 1 (the same in x).  Sub-row 0 can only serve
# dy = 0 (ky = 1); sub-row 1 serves dy = -1 (ky = 0) and dy = 0 (ky = 2): 1 + 2 + 2 + 4 = 9 steps, each tap once, none on a zero weight.
def s2_schedule():
    """[(sy, sx, dy, dx, ky, kx)] in step order for one 16-channel chunk."""
    steps = []
    for sy in (0, 1):
        for sx in (0, 1):
            for dy in ((0,) if sy == 0 else (-1, 0)):
                for dx in ((0,) if sx == 0 else (-1, 0)):
                    steps.append((sy, sx, dy, dx, 2 * dy + sy + 1, 2 * dx + sx + 1))
    return steps


def bf16x3_terms(w: np.ndarray):
    """The exact three-term truncation split of float32 values (vd3d_x3.h x3_split): uint16 bf16 bit patterns t1, t2, t3 with t1 + t2 + t3 == w."""
    w = np.ascontiguousarray(w, np.float32)
    t1 = w.view(np.uint32) & np.uint32(0xFFFF0000)
    r1 = w - t1.view(np.float32)
    t2 = r1.view(np.uint32) & np.uint32(0xFFFF0000)
    r2 = r1 - t2.view(np.float32)
    t3 = r2.view(np.uint32)
    assert not (t3 & np.uint32(0xFFFF)).any()   # at most 8 significant bits are left
    return [(t >> np.uint32(16)).astype(np.uint16) for t in (t1, t2, t3)]


def s2_image_reference(W: np.ndarray) -> np.ndarray:
    """The weight image of vd3d_conv3x3_s2_x3 for W[Cout][Cin][3][3], as bytes: [slice Cout / 128][step 9 Cin / 16][term 3][k-half 2][oc 128][8 bf16], the steps
    of a slice in the order ``s2_schedule`` runs them chunk after chunk, then the 64-byte zero page."""
    Cout, Cin = W.shape[:2]
    sched = s2_schedule()
    img = np.zeros((Cout // 128, (Cin // 16) * 9, 3, 2, 128, 8), np.uint16)
    for c16 in range(Cin // 16):
        for j, (_, _, _, _, ky, kx) in enumerate(sched):
            blk = W[:, c16 * 16:(c16 + 1) * 16, ky, kx]                        # [Cout][16]
            for t, term in enumerate(bf16x3_terms(blk)):
                img[:, c16 * 9 + j, t] = term.reshape(Cout // 128, 128, 2, 8).transpose(0, 2, 1, 3)
    return np.concatenate([img.reshape(-1).view(np.uint8), np.zeros(64, np.uint8)])


def patchify_reference(x_nhwc: np.ndarray, p: int) -> np.ndarray:
    """vd3d_patchify_f32's statement: x [B][th][tw][3] -> rows [B][gh * gw][Kp], column (c p + ky) p + kx, zero tail."""
    B, th, tw, _ = x_nhwc.shape
    gh, gw, K = th // p, tw // p, 3 * p * p
    rows = np.zeros((B, gh * gw, (K + 15) // 16 * 16), np.float32)
    v = x_nhwc[:, :gh * p, :gw * p].reshape(B, gh, p, gw, p, 3)               # [b][gy][ky][gx][kx][c]
    rows[:, :, :K] = v.transpose(0, 1, 3, 5, 2, 4).reshape(B, gh * gw, K)
    return rows


def unfold_rows(x_nchw: torch.Tensor, p: int) -> torch.Tensor:
    return F.unfold(x_nchw, kernel_size=p, stride=p).transpose(1, 2)          # [B][L][3 p p]


def test_schedule_runs_every_tap_once_and_none_on_a_zero_weight():
    s = s2_schedule()
    assert [sum(1 for e in s if e[:2] == sub) for sub in ((0, 0), (0, 1), (1, 0), (1, 1))] == [1, 2, 2, 4]
    assert sorted((ky, kx) for *_, ky, kx in s) == [(a, b) for a in range(3) for b in range(3)]
    assert [(ky, kx) for *_, ky, kx in s] == [(1, 1), (1, 0), (1, 2), (0, 1), (2, 1), (0, 0), (0, 2), (2, 0), (2, 2)]   # the order include/vd3d.h states
    for sy, sx, dy, dx, ky, kx in s:   # the shifted sub-pixel IS the tap's input pixel: 2 (q + dy) + sy == 2 q - 1 + ky
        assert 2 * dy + sy == ky - 1 and 2 * dx + sx == kx - 1


def test_s2_image_reference_decodes_to_the_weights_in_schedule_order():
    """The image's three terms sum back to W exactly, at the position the kernel reads: slice oc // 128, step 9 c16 + j, k-half (ci % 16) // 8, row oc % 128."""
    rng = np.random.default_rng(5)
    Cout, Cin = 256, 48
    W = (rng.standard_normal((Cout, Cin, 3, 3)) * 0.05).astype(np.float32)
    raw = s2_image_reference(W)
    from visiondepth3d_amd import _lib
    assert raw.size == _lib.lib().vd3d_conv3x3_s2_x3_weight_bytes(Cin, Cout) and not raw[-64:].any()
    img = raw[:-64].view(np.uint16).reshape(Cout // 128, Cin // 16 * 9, 3, 2, 128, 8)
    val = (img.astype(np.uint32) << 16).view(np.float32)
    tot = (val[:, :, 0] + val[:, :, 1]) + val[:, :, 2]                       # exact: the terms do not overlap
    for c16 in range(Cin // 16):
        for j, (*_, ky, kx) in enumerate(s2_schedule()):
            got = tot[:, c16 * 9 + j].transpose(0, 2, 1, 3).reshape(Cout, 16)
            assert np.array_equal(got, W[:, c16 * 16:(c16 + 1) * 16, ky, kx]), (c16, j)


def test_weight_bytes_rule_and_exports():
    from visiondepth3d_amd import _lib
    L = _lib.lib()
    for cin in (16, 48, 384, 1024):
        for cout in (128, 256, 384, 768, 1024):
            assert L.vd3d_conv3x3_s2_x3_weight_bytes(cin, cout) == cin // 16 * 9 * cout * 96 + 64
    for cin, cout in ((24, 128), (0, 128), (-16, 128), (16, 96), (16, 64), (16, 0), (16, 1152), (16, 192)):
        assert L.vd3d_conv3x3_s2_x3_weight_bytes(cin, cout) < 0, (cin, cout)
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    for name in NEW:
        assert re.search(r"\bint(64_t)? " + name + r"\(", hdr) and name in _lib.EXPORTS and hasattr(L, name), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "vd3d_conv_s2.hip" in mk and "vd3d_conv_x3.h" in mk


def test_keyword_refusals_name_the_missing_condition():
    from visiondepth3d_amd.depth import DepthPipe
    ok = dict(device="cuda", dtype=torch.float32, gemm="bf16x3", conv="bf16x3", renderer=object(), self_contained=True)
    name = "depth-anything-v2-small"
    with pytest.raises(ValueError, match="renderer"):                                        # the CPU: no renderer on a GPU
        DepthPipe(name, device="cpu", dtype=torch.float32, gemm="bf16x3", conv="bf16x3", self_contained=True)
    with pytest.raises(ValueError, match="renderer"):
        DepthPipe(name, **dict(ok, device="cpu"))                                            # a renderer does not make the CPU a GPU
    with pytest.raises(ValueError, match="renderer"):
        DepthPipe(name, **dict(ok, renderer=None))
    with pytest.raises(ValueError, match=r"self_contained=True needs gemm='bf16x3'"):
        DepthPipe(name, **dict(ok, gemm="f32", conv=None))
    with pytest.raises(ValueError, match=r"self_contained=True needs gemm='bf16x3'"):
        DepthPipe(name, **dict(ok, gemm="fp16x2", conv=None))
    with pytest.raises(ValueError, match=r"self_contained=True needs conv='bf16x3'"):
        DepthPipe(name, **dict(ok, conv=None))
    with pytest.raises(ValueError, match="float32"):
        DepthPipe(name, **dict(ok, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="fuse_backbone=True"):
        DepthPipe(name, **dict(ok, fuse_backbone=False))
    with pytest.raises(ValueError, match=r"gemm='bf16x3', conv='bf16x3'.*fuse_backbone=True"):   # every missing condition is named
        DepthPipe(name, **dict(ok, gemm="f32", conv=None, fuse_backbone=False))


def test_other_models_are_refused_by_name_before_a_device_is_touched():
    """DPT-Large's class (a small configuration of it: the refusal reads the model's type, not its size) and a DepthAnything model on another backbone."""
    transformers = pytest.importorskip("transformers")
    from visiondepth3d_amd.depth import DepthPipe
    ok = dict(device="cuda", dtype=torch.float32, gemm="bf16x3", conv="bf16x3", renderer=object(), self_contained=True)
    cfg = transformers.DPTConfig(hidden_size=64, num_hidden_layers=4, num_attention_heads=1, intermediate_size=128, image_size=32, patch_size=16,
                                 backbone_out_indices=[0, 1, 2, 3], neck_hidden_sizes=[16, 16, 16, 16], fusion_hidden_size=16, readout_type="project")
    dpt = transformers.DPTForDepthEstimation(cfg).eval()
    with pytest.raises(NotImplementedError, match=r"self_contained=True: 'dpt-large' \(DPTForDepthEstimation"):
        DepthPipe("dpt-large", model=dpt, **ok)
    # the defaults of the keyword leave DepthPipe's signature as it was: the mode is off unless asked for
    import inspect
    assert inspect.signature(DepthPipe.__init__).parameters["self_contained"].default is False


def test_patch_embedding_weight_and_patchify_match_unfold_bit_for_bit():
    from visiondepth3d_amd.depth import patch_embedding_gemm_weight
    g = torch.Generator().manual_seed(3)
    w = torch.randn(24, 3, 14, 14, generator=g)
    wg = patch_embedding_gemm_weight(w)
    assert tuple(wg.shape) == (24, 592) and wg.is_contiguous() and torch.equal(wg[:, :588], w.reshape(24, 588)) and not bool(wg[:, 588:].any())
    for B, th, tw in ((1, 28, 42), (2, 126, 238), (1, 30, 45)):                               # the last: a remainder the convolution drops
        x = torch.randn(B, 3, th, tw, generator=g)
        rows = patchify_reference(x.permute(0, 2, 3, 1).contiguous().numpy(), 14)
        want = unfold_rows(x[:, :, :th // 14 * 14, :tw // 14 * 14], 14)
        assert rows.shape == (B, (th // 14) * (tw // 14), 592)
        assert np.array_equal(rows[:, :, :588], want.numpy()) and not rows[:, :, 588:].any()
        # and the GEMM on those rows is the convolution (float64: the two differ by re-association only)
        y = torch.from_numpy(rows).double() @ wg.double().t()
        ref = F.conv2d(x.double(), w.double(), None, stride=14).flatten(2).transpose(1, 2)
        assert float((y - ref).abs().max()) <= 1e-11 * float(ref.abs().max() + 1)
    assert tuple(patch_embedding_gemm_weight(torch.zeros(8, 3, 16, 16)).shape) == (8, 768)   # 3 x 16 x 16 is a multiple of 16 already: no tail


@pytest.mark.parametrize("s,C,gh,gw", [(4, 48, 9, 17), (2, 96, 5, 3)])
def test_conv_transpose_as_gemm_and_depth_to_space_matches_conv_transpose2d(s, C, gh, gw):
    """conv_transpose_gemm_weight + the scatter of vd3d_depth_to_space_bias_nhwc_f32 (numpy) against F.conv_transpose2d in float64: kernel == stride 4 and 2."""
    from visiondepth3d_amd.depth import conv_transpose_gemm_weight
    g = torch.Generator().manual_seed(s)
    B = 2
    w = torch.randn(C, C, s, s, generator=g, dtype=torch.float64)
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    x = torch.randn(B, C, gh, gw, generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x, w, bias, stride=s)
    rows = x.permute(0, 2, 3, 1).reshape(B * gh * gw, C)
    y = (rows @ conv_transpose_gemm_weight(w).t()).numpy().reshape(B, gh, gw, s, s, C)      # [b][y][x][i][j][c]
    out = y.transpose(0, 1, 3, 2, 4, 5).reshape(B, gh * s, gw * s, C) + bias.numpy()            # out[b][y s + i][x s + j][c]
    got = torch.from_numpy(out).permute(0, 3, 1, 2)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_conv3x3_s2_x3_census():
    """k_conv_x3<K3S2, 4, 2, false> (vd3d_conv_s2.hip): a 512-thread workgroup, two waves per SIMD -- at most 256 registers, nothing spilled, no scratch; no static
    LDS in front of the dynamic array; the launcher's dynamic LDS request is the 128-channel plan, within CX_LDS_MAX."""
    from test_conv_x3_host import _census
    k, asm = _census("vd3d_conv_s2.hip")
    convs = {n: v for n, v in k.items() if n.startswith("_Z9k_conv_x3ILi")}
    assert list(convs) == [n for n in convs if n.startswith("_Z9k_conv_x3ILi1ELi4ELi2ELb0E")] and len(convs) == 1, sorted(k)
    c = next(iter(convs.values()))
    assert c["spill"] == 0 and c["sgpr_spill"] == 0 and c["vgpr"] <= 256 and c["lds"] % 16 == 0 and c["lds"] == 0, c
    assert "scratch_" not in asm and re.search(r"\.private_segment_fixed_size:\s+0\b", asm) and not re.search(r"\.private_segment_fixed_size:\s+[1-9]", asm)
    assert "v_mfma_f32_32x32x16_bf16" in asm and "v_mfma_f32_32x32x2_f32" not in asm
    src = open(os.path.join(CSRC, "vd3d_conv_s2.hip")).read()
    assert set(re.findall(r"cx_lds\((\d+)\), s, a\)", src)) == {"128"}
    lds_max = int(re.search(r"#define CX_LDS_MAX (\d+)", open(os.path.join(CSRC, "vd3d_conv_x3.hip")).read()).group(1))
    assert 2 * (3 * 2 * 340 * 16) + 3 * 512 * 16 + 4 * 16384 <= lds_max <= 163840          # cx_lds(128): two chunk images, staging, four 16 KB ring stages
