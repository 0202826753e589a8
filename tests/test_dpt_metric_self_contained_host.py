"""Host-side tests (no GPU) of DepthPipe(self_contained=True) for DPT-Large and the metric Depth-Anything heads, and of the sigmoid head tail
(vd3d_dpt_head_tail_act_f32): a numpy statement of the tail kernel in the kernel's own order, the two new zoo names, the constructor's refusals, the export and
the instantiations hipcc builds.

``head_tail_v`` / ``head_tail_reference`` are what tests/test_hip_head_tail_act.py holds the device kernel to, bit for bit."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
f32, f64 = np.float32, np.float64


def fma32(a, b, c):
    """The float32 fused multiply-add round(a * b + c), one rounding, on float32 arrays.  The product of two float32 values is exact in float64; the float64 sum is
    rounded to odd with the exact residual of TwoSum (Boldo & Melquiond: 53 >= 24 + 2 bits make the final rounding to float32 the correctly rounded one), so no
    double rounding can move a tie."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
        c = np.broadcast_to(np.asarray(c, f32).astype(f64), p.shape)
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)                                    # exact: s + err == p + c
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def head_tail_v(y, b2, w3, b3, act="relu"):
    """v[p] = b3 + sum_c w3[c] * max(y[p][c] + b2[c], 0) as k_head_tail forms it: lane l of the C / 4 lanes of a pixel holds channels 4 l .. 4 l + 3 and computes
    max(y.x + b.x, 0) * w.x, then three FMAs (y, z, w); the lanes meet in the xor butterfly (offsets C / 8, ..., 1; every lane adds its partner's value, lane 0
    holds the pixel's); then + b3.  Every operation is one float32 rounding.  y [n_pix][C] -> float32 [n_pix].  ``act`` decides one thing only, what the inner
    max makes of a NaN: the ReLU tail's fmaxf(NaN, 0) is 0, the sigmoid tail keeps the NaN."""
    y, b2, w3 = np.asarray(y, f32), np.asarray(b2, f32), np.asarray(w3, f32)
    n, C = y.shape
    lanes = C // 4
    with np.errstate(all="ignore"):
        r = np.maximum(y + b2[None, :], f32(0))                          # numpy's maximum keeps a NaN
        if act == "relu":
            r = np.where(np.isnan(r), f32(0), r)
        r = r.reshape(n, lanes, 4)
        w = w3.reshape(lanes, 4)
        acc = r[:, :, 0] * w[None, :, 0]
        for k in (1, 2, 3):
            acc = fma32(r[:, :, k], np.broadcast_to(w[None, :, k], acc.shape), acc)
        idx = np.arange(lanes)
        off = lanes // 2
        while off > 0:
            acc = acc + acc[:, idx ^ off]
            off //= 2
        return (acc[:, 0] + f32(b3)).astype(f32)


def head_tail_reference(y, b2, w3, b3, scale, act="relu", sigmoid=None):
    """The whole tail: act(v) * scale, two float32 roundings.  ``act="sigmoid"`` takes the sigmoid as a callable float32 array -> float32 array (the GPU test hands in
    Renderer.torch_math: torch.sigmoid's CPU values)."""
    v = head_tail_v(y, b2, w3, b3, act)
    with np.errstate(all="ignore"):
        a = np.where(np.isnan(v), f32(0), np.maximum(v, f32(0))) if act == "relu" else np.asarray(sigmoid(v), f32)
        return (a * f32(scale)).astype(f32)


def test_fma32_is_one_rounding():
    one = f32(1) + f32(2.0 ** -12)
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: a float32 tie.  An addend of +-2^-60 decides it; a float64 sum would lose the addend and break the tie to even.
    assert fma32([one], [one], [f32(2.0 ** -60)])[0] == f32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert fma32([one], [one], [f32(-2.0 ** -60)])[0] == f32(1 + 2.0 ** -11)
    assert fma32([one], [one], [f32(0)])[0] == f32(1 + 2.0 ** -11)            # the tie itself: to even
    rng = np.random.default_rng(0)
    a, b, c = (rng.integers(-50, 50, 1000).astype(f32) for _ in range(3))
    assert np.array_equal(fma32(a, b, c), a * b + c)                             # exact operands: the plain expression
    assert np.isnan(fma32([f32("nan")], [one], [one])[0])


@pytest.mark.parametrize("C", [16, 32, 64])
def test_relu_statement_equals_the_torch_expression_on_small_integers(C):
    """Small integers: every product and every partial sum is an exact float32 integer, so the kernel's order and torch's give the same bits."""
    rng = np.random.default_rng(C)
    for n in (1, 15, 17, 65):
        y = rng.integers(-6, 7, (n, C)).astype(f32)
        b2 = rng.integers(-3, 4, C).astype(f32)
        w3 = rng.integers(-4, 5, C).astype(f32)
        b3, scale = -7.0, 3.0
        want = torch.relu((torch.relu(torch.from_numpy(y) + torch.from_numpy(b2)) * torch.from_numpy(w3)).sum(1) + b3) * scale
        got = head_tail_reference(y, b2, w3, b3, scale)
        assert got.dtype == f32 and np.array_equal(got, want.numpy())
        assert n < 15 or ((got > 0).any() and (got == 0).any())                  # both sides of the last ReLU are exercised
        # and the sigmoid branch is sigmoid(v) * scale on the same v
        v = head_tail_v(y, b2, w3, b3)
        sg = head_tail_reference(y, b2, w3, b3, scale, act="sigmoid", sigmoid=lambda t: torch.sigmoid(torch.from_numpy(t)).numpy())
        assert np.array_equal(sg, (torch.sigmoid(torch.from_numpy(v)) * scale).numpy())


def test_statement_is_close_to_float64_on_random_operands():
    rng = np.random.default_rng(3)
    y, b2, w3 = rng.standard_normal((257, 32)).astype(f32), rng.standard_normal(32).astype(f32), rng.standard_normal(32).astype(f32)
    ref = (np.maximum(y.astype(f64) + b2, 0) * w3).sum(1) + 0.25
    mag = (np.maximum(y.astype(f64) + b2, 0) * np.abs(w3)).sum(1) + 0.25
    assert float((np.abs(head_tail_v(y, b2, w3, 0.25) - ref) / mag).max()) < 8 * 2.0 ** -24   # 3 FMAs + 3 butterfly adds + the bias


@pytest.mark.parametrize("name,max_depth", [("depth-anything-v2-metric-indoor-large", 20), ("depth-anything-v2-metric-outdoor-large", 80)])
def test_metric_zoo_names_build_the_dinov2_large_network_with_a_sigmoid_head(name, max_depth):
    transformers = pytest.importorskip("transformers")
    from visiondepth3d_amd.depth import MODEL_ZOO, build_config
    z = MODEL_ZOO[name]
    assert {k: z[k] for k in MODEL_ZOO["depth-anything-v2-large"]} == MODEL_ZOO["depth-anything-v2-large"] and z["metric"] is True
    cfg = build_config(name)
    assert cfg.depth_estimation_type == "metric" and cfg.max_depth == max_depth and isinstance(cfg.max_depth, int)
    with torch.device("meta"):   # no 335 M-parameter allocation
        m = transformers.DepthAnythingForDepthEstimation(cfg)
    assert isinstance(m.head.activation2, torch.nn.Sigmoid) and m.head.max_depth == max_depth and m.head.conv2.out_channels == 32
    bc = m.config.backbone_config
    assert (bc.hidden_size, bc.num_hidden_layers, bc.num_attention_heads, bc.patch_size) == (1024, 24, 16, 14)
    assert type(m.backbone).__name__ == "Dinov2Backbone" and next(m.parameters()).device.type == "meta"
    # the relative names are what they were
    assert build_config("depth-anything-v2-large").depth_estimation_type == "relative"


OK = dict(device="cuda", dtype=torch.float32, gemm="bf16x3", conv="bf16x3", renderer=object(), self_contained=True)


def _dpt_cfg(**kw):
    import transformers
    base = dict(hidden_size=384, num_hidden_layers=2, num_attention_heads=6, intermediate_size=768, image_size=64, patch_size=16, backbone_out_indices=[0, 1, 1, 1],
                neck_hidden_sizes=[16, 32, 128, 128], fusion_hidden_size=32, readout_type="project")
    base.update(kw)
    return transformers.DPTConfig(**base)


@pytest.mark.parametrize("kw,why", [(dict(readout_type="ignore"), "readout_type='ignore'"), (dict(use_batch_norm_in_fusion_residual=True), "batch norm"),
                                    (dict(hidden_size=64, num_attention_heads=1, intermediate_size=128), "hidden size 64")])
@pytest.mark.parametrize("pair", ["bf16x3", "fp16x2"])
def test_dpt_models_outside_the_split_scope_are_refused_by_name_before_the_renderer_is_touched(kw, why, pair):
    """renderer=object(): any use of the renderer, and any move to the (absent) GPU, would raise something else than the refusal."""
    transformers = pytest.importorskip("transformers")
    from visiondepth3d_amd.depth import DepthPipe
    dpt = transformers.DPTForDepthEstimation(_dpt_cfg(**kw)).eval()
    with pytest.raises(NotImplementedError, match=r"^self_contained=True: 'my-dpt' \(DPTForDepthEstimation\): .*" + re.escape(why)):
        DepthPipe("my-dpt", model=dpt, **dict(OK, gemm=pair, conv=pair))
    assert all("forward" not in m.__dict__ for m in dpt.modules())       # nothing was rewritten
    assert next(dpt.parameters()).device.type == "cpu"


def test_dpt_large_scope_is_accepted_under_the_keyword():
    """A plain-ViT DPT with 64-wide heads and readout_type="project" passes the keyword's scope check (the construction itself needs the GPU)."""
    transformers = pytest.importorskip("transformers")
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    pipe = DepthPipe("my-dpt", device="cpu", model=transformers.DPTForDepthEstimation(_dpt_cfg()).eval(), processor=dict(PROCESSORS["dpt"], size=(64, 64)))
    pipe.gemm, pipe.conv, pipe.self_contained = "bf16x3", "bf16x3", True
    assert pipe._split_scope() == "dpt-vit"


def test_depth_anything_head_with_another_activation_is_refused_by_name():
    transformers = pytest.importorskip("transformers")
    from visiondepth3d_amd.depth import DepthPipe
    bc = transformers.Dinov2Config(hidden_size=384, num_hidden_layers=4, num_attention_heads=6, patch_size=14, image_size=28, out_indices=[1, 2, 3, 4],
                                   reshape_hidden_states=False, apply_layernorm=True)
    cfg = transformers.DepthAnythingConfig(backbone_config=bc, reassemble_hidden_size=384, neck_hidden_sizes=[16, 32, 64, 128], fusion_hidden_size=32,
                                           head_hidden_size=32, reassemble_factors=[4, 2, 1, 0.5], patch_size=14)
    m = transformers.DepthAnythingForDepthEstimation(cfg).eval()
    m.head.activation2 = torch.nn.Tanh()
    with pytest.raises(NotImplementedError, match=r"^self_contained=True: 'my-da' \(DepthAnythingForDepthEstimation\): the depth head ends in Tanh.*ReLU.*Sigmoid"):
        DepthPipe("my-da", model=m, **OK)
    with pytest.raises(ValueError, match="act must be 'relu' or 'sigmoid'"):   # the renderer's keyword, checked before anything else is touched
        from visiondepth3d_amd.render_3d import Renderer
        Renderer.dpt_head_tail(None, None, None, None, 0.0, 1.0, act="tanh")


def test_entry_point_is_declared_exported_and_bound():
    from visiondepth3d_amd import _abi, _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "vd3d.h")).read()
    name = "vd3d_dpt_head_tail_act_f32"
    assert re.search(r"\bint " + name + r"\(vd3d_ctx\* ctx, const float\* y, const float\* b2, const float\* w3, float b3, float scale, int64_t n_pix, int C, int act, "
                     r"float\* out\);", hdr)
    assert name in _lib.EXPORTS and hasattr(L, name) and len(L.vd3d_dpt_head_tail_act_f32.argtypes) == len(L.vd3d_dpt_head_tail_f32.argtypes) + 1
    assert re.search(r"enum \{ VD3D_HEAD_ACT_RELU = 0, VD3D_HEAD_ACT_SIGMOID = 1 \};", hdr) and (_abi.HEAD_ACT_RELU, _abi.HEAD_ACT_SIGMOID) == (0, 1)
    assert re.search(r"Additions since 6 that leave the version as it is.*?" + name + r".*?\*/\s*#define VD3D_ABI_VERSION 6", hdr, re.S) and _abi.ABI_VERSION == 6
    # no context: both entry points refuse alike, before anything else
    import ctypes
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.vd3d_dpt_head_tail_act_f32(None, p, p, p, 0.0, 1.0, 1, 16, 1, p) == _abi.E_INVALID
    assert L.vd3d_dpt_head_tail_f32(None, p, p, p, 0.0, 1.0, 1, 16, p) == _abi.E_INVALID


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_head_tail_census_relu_instantiations_carry_no_sigmoid():
    """k_head_tail<LPP, ACT>: six instantiations (C / 4 = 4, 8, 16 lanes per pixel; ReLU and sigmoid), no spill, no LDS, no scratch; the exponential, the
    reciprocal and the division fix-up of vd_sigmoid_torch appear in the sigmoid instantiations only."""
    from test_conv_x3_host import _census
    k, asm = _census("vd3d_netops.hip")
    tails = {n: v for n, v in k.items() if n.startswith("_Z11k_head_tailILi")}
    assert sorted(re.match(r"_Z11k_head_tailILi(\d+)ELi(\d)E", n).groups() for n in tails) == sorted((str(l), str(a)) for l in (4, 8, 16) for a in (0, 1)), sorted(tails)
    for n, c in tails.items():
        assert c["spill"] == 0 and c["sgpr_spill"] == 0 and c["lds"] == 0 and c["vgpr"] <= 64, (n, c)
        body = asm[asm.index("\n" + n + ":"):]
        body = body[:body.index("s_endpgm")]
        sig = bool(re.search(r"v_(rcp|ldexp|div_fixup|div_fmas)_f32", body))
        assert sig == n.startswith(re.match(r"_Z11k_head_tailILi\d+E", n).group(0) + "Li1E"), n
        assert "scratch_" not in body
