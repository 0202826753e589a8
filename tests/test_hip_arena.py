"""GPU tests (-m gpu): the network kernels held to their own buffers (tests/arena.py states the harness, its three fills and what it cannot see: a read outside a
buffer whose value is discarded, and an access more than 1 MiB from the payload).  One table row per entry point and shape: operands seeded on the CPU, the buffers
with their roles and the alignment include/vd3d.h demands (16 unless the header says 4-byte), and the raw C call through ``R._L`` -- the pack first, then the kernel.
Weight images are ``whole`` scratch (every byte of ``*_weight_bytes`` is the packer's), workspaces plain scratch of exactly ``*_workspace_bytes``.  Where the
operation allows it the operands are small integers (x = idx % 13 - 6, w = 7 idx % 11 - 5, bias = arange), every product and partial sum an exact float32 integer,
and the output must EQUAL the float64 CPU result.  Shapes: the smallest that cross each tile boundary of the kernel (GEMM tile 256 x 256, K step 16, ring of four;
attention 32-query block / 64-row KV tile / 256-query workgroup; convolutions the sizes tests/golden/x3_bits.json records), the smallest ragged shape of each
op's own test for the heads and the glue.

Glue rows left out -- none for state kept in the context.  ``vd3d_resize_pil_bicubic_u8`` and ``vd3d_depth_preprocess_pil`` build their coefficient tables at a
geometry's first use and keep them: a later run reads the same tables, so the three-fold run repeats and the rows stay in.

Two tests at the wrapper level: ``Renderer.attention_x3``'s cached workspace overwritten with 0xFF between a large and a small call, and every ``*_pack`` wrapper
packing into an image pre-filled with 0xFF and with 0x47 (``torch.empty`` of the wrapper's module answers with filled memory): the images are equal byte for byte."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arena   # noqa: E402
from arena import Buf, Case   # noqa: E402

MODES = {"bf16x3": 0, "fp16x2": 1}


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


# ---------------------------------------------------------------------------------------------------------------- operands and buffers
def ints(shape, mul=1, mod=13, sub=6):
    idx = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    return ((idx * mul) % mod - sub).astype(np.float32)


def wints(shape):
    return ints(shape, 7, 11, 5)


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def bf16_bits(a):
    """float32 -> bf16 (round to nearest even) as int16 bits."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16).view(np.int16)


def inp(name, data, align=16):
    return Buf(name, "input", align, data=np.ascontiguousarray(data))


def out(name, shape, align=16, dtype="float32"):
    item = 2 if dtype == "bfloat16" else np.dtype(dtype).itemsize
    return Buf(name, "output", align, nbytes=int(np.prod(shape)) * item, dtype=dtype)


def image(name, nbytes):
    assert nbytes > 0, (name, nbytes)
    return Buf(name, "scratch", 16, nbytes=int(nbytes), whole=True)


def work(name, nbytes):
    assert nbytes > 0, (name, nbytes)
    return Buf(name, "scratch", 16, nbytes=int(nbytes))


def nchw(t):
    """NHWC storage -> the channels_last [B, C, H, W] view the wrappers take."""
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def f64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def conv64(x_nhwc, w, stride=1):
    return F.conv2d(f64(x_nhwc).permute(0, 3, 1, 2), f64(w), None, stride, 1).permute(0, 2, 3, 1).numpy()


ROWS = []   # (id, builder(L) -> Case)


def row(rid):
    def deco(fn):
        ROWS.append((rid, fn))
        return fn
    return deco


# ---------------------------------------------------------------------------------------------------------------- vd3d_gemm_x3
def gemm_row(mode, M, K, N, bias, gelu):
    def build(L):
        m = MODES[mode]
        X, W = ints((M, K)), wints((N, K))
        b = np.arange(N, dtype=np.float32) if bias else None
        bufs = [inp("X", X), inp("W", W), image("img", L.vd3d_gemm_x3_weight_bytes(N, K, m)), out("Y", (M, N))] + ([inp("bias", b)] if bias else [])

        def call(e):
            return (L.vd3d_gemm_x3_pack_weights(e.ctx, e.p["W"], N, K, m, e.p["img"])
                    or L.vd3d_gemm_x3(e.ctx, e.p["X"], M, K, e.p["img"], N, m, e.p["bias"] if bias else None, int(gelu), e.p["Y"]))

        def wrap(R, t):
            return {"Y": R.linear_x3(t["X"], R.gemm_x3_pack(t["W"], mode), N, t.get("bias"), gelu, mode)}
        exact = {} if gelu else {"Y": X.astype(np.float64) @ W.astype(np.float64).T + (b.astype(np.float64) if bias else 0.0)}
        return Case("vd3d_gemm_x3_pack_weights+vd3d_gemm_x3", f"{mode} M{M} K{K} N{N} bias{int(bias)} gelu{int(gelu)}", bufs, call, wrap, exact)
    return build


for _mode in MODES:
    for _M, _K, _N in ((1, 16, 1), (257, 48, 255), (255, 80, 257)):
        for _b in (False, True):
            ROWS.append((f"gemm-{_mode}-{_M}x{_K}x{_N}-b{int(_b)}", gemm_row(_mode, _M, _K, _N, _b, False)))
    ROWS.append((f"gemm-{_mode}-257x48x255-gelu", gemm_row(_mode, 257, 48, 255, True, True)))


# ---------------------------------------------------------------------------------------------------------------- attention
def attn_row(kind, T):
    """kind: "bf16x3" | "fp16x2" (vd3d_attention_x3, workspace poisoned) or 4 | 8 (vd3d_attention_f32_form)."""
    B, H, D = 2, 2, 64

    def build(L):
        qkv = rnd((B, T, 3, H, D), 100 + T)
        scale = D ** -0.5
        bufs = [inp("qkv", qkv), out("out", (B, T, H, D))]
        if kind in MODES:
            m = MODES[kind]
            nb = L.vd3d_attention_x3_workspace_bytes(B, T, H, D, m)
            bufs.append(work("workspace", nb))
            call = lambda e: L.vd3d_attention_x3(e.ctx, e.p["qkv"], B, T, H, D, scale, m, e.p["workspace"], nb, e.p["out"])   # noqa: E731
            wrap = lambda R, t: {"out": R.attention_x3(t["qkv"].view(B, T, 3 * H * D), H, scale, kind)}   # noqa: E731
            return Case("vd3d_attention_x3", f"{kind} B{B} T{T} H{H} D{D}", bufs, call, wrap)
        call = lambda e: L.vd3d_attention_f32_form(e.ctx, e.p["qkv"], B, T, H, D, scale, e.p["out"], kind)   # noqa: E731
        wrap = lambda R, t: {"out": R.attention_f32(t["qkv"].view(B, T, 3 * H * D), H, scale, kind)}   # noqa: E731
        return Case("vd3d_attention_f32_form", f"form{kind} B{B} T{T} H{H} D{D}", bufs, call, wrap)
    return build


for _kind in ("bf16x3", "fp16x2", 4, 8):
    for _T in (1, 33, 65, 257):
        ROWS.append((f"attn-{_kind}-T{_T}", attn_row(_kind, _T)))


# ---------------------------------------------------------------------------------------------------------------- the tile convolutions
def conv_row(fam, Cin, Cout, B, H, W):
    stride = 2 if fam.startswith("s2_") else 1
    y_align = 16 if fam in ("x3", "x2") else 4   # include/vd3d.h: "(Y 4-byte)" for s2_x3, s1_x2 and s2_x2

    def build(L):
        X, Wt = ints((B, H, W, Cin)), wints((Cout, Cin, 3, 3))
        Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
        nb = getattr(L, f"vd3d_conv3x3_{fam}_weight_bytes")(Cin, Cout)
        bufs = [inp("X", X), inp("W", Wt), image("img", nb), out("Y", (B, Ho, Wo, Cout), y_align)]

        def call(e):
            return (getattr(L, f"vd3d_conv3x3_{fam}_pack_weights")(e.ctx, e.p["W"], Cin, Cout, e.p["img"])
                    or getattr(L, f"vd3d_conv3x3_{fam}")(e.ctx, e.p["X"], B, H, W, Cin, e.p["img"], Cout, e.p["Y"]))

        def wrap(R, t):
            return {"Y": nhwc(R._conv3x3(fam, nchw(t["X"]), R._conv3x3_pack(fam, t["W"]), Cout))}
        return Case(f"vd3d_conv3x3_{fam}_pack_weights+vd3d_conv3x3_{fam}", f"B{B} {H}x{W} Cin{Cin} Cout{Cout}", bufs, call, wrap, {"Y": conv64(X, Wt, stride)})
    return build


for _fam, _couts, _shapes in (("x3", (32, 64, 128, 256), ((1, 1, 1), (2, 13, 47))), ("s1_x2", (32, 64, 128, 256), ((1, 1, 1), (2, 13, 47))),
                              ("x2", (32, 64, 128), ((1, 1, 1), (2, 13, 47))),
                              ("s2_x3", (128, 256), ((1, 2, 2), (2, 25, 93))), ("s2_x2", (128, 256), ((1, 2, 2), (2, 25, 93)))):
    for _co in _couts:
        for _ci in (16, 48):
            for _s in _shapes:
                ROWS.append((f"conv-{_fam}-c{_ci}-{_co}-{_s[0]}x{_s[1]}x{_s[2]}", conv_row(_fam, _ci, _co, *_s)))


def epi_row(mode):
    B, H, W, Cin, Cout = 2, 9, 33, 32, 64   # tests/test_hip_conv_epi_bits.py: one row and one column past a tile
    fam = {"bf16x3": "x3", "fp16x2": "s1_x2"}[mode]

    def build(L):
        X, Wt, b = ints((B, H, W, Cin)), wints((Cout, Cin, 3, 3)), np.arange(Cout, dtype=np.float32)
        r1, r2 = ints((B, H, W, Cout), 3, 17, 8), ints((B, H, W, Cout), 5, 19, 9)
        bufs = [inp("X", X), inp("W", Wt), image("img", getattr(L, f"vd3d_conv3x3_{fam}_weight_bytes")(Cin, Cout)), inp("bias", b, 4), inp("r1", r1, 4), inp("r2", r2, 4),
                out("Y", (B, H, W, Cout), 4), out("Yrelu", (B, H, W, Cout), 4)]

        def call(e):
            return (getattr(L, f"vd3d_conv3x3_{fam}_pack_weights")(e.ctx, e.p["W"], Cin, Cout, e.p["img"])
                    or L.vd3d_conv3x3_epi(e.ctx, MODES[mode], e.p["X"], B, H, W, Cin, e.p["img"], Cout, 0, e.p["bias"], e.p["r1"], e.p["r2"], e.p["Y"], e.p["Yrelu"]))

        def wrap(R, t):
            y, yr = R.conv3x3_epi(nchw(t["X"]), R.conv3x3_tile_pack(t["W"], mode), Cout, mode, t["bias"], nchw(t["r1"]), nchw(t["r2"]), want_relu_copy=True)
            return {"Y": nhwc(y), "Yrelu": nhwc(yr)}
        v = r2.astype(np.float64) + (conv64(X, Wt) + b.astype(np.float64) + r1.astype(np.float64))
        return Case(f"vd3d_conv3x3_{fam}_pack_weights+vd3d_conv3x3_epi", f"{mode} B{B} {H}x{W} Cin{Cin} Cout{Cout} bias r1 r2 Yrelu", bufs, call, wrap,
                    {"Y": v, "Yrelu": np.maximum(v, 0.0)})
    return build


for _mode in MODES:
    ROWS.append((f"conv-epi-{_mode}", epi_row(_mode)))


def ifn_row(kind, B, H, W, Cin, Cout):
    """Dense pitches, per-channel slopes that are powers of two (exact products), a residual."""
    name = ("K3S1", "K3S2", "T4S2")[kind]

    def build(L):
        X = ints((B, H, W, Cin))
        Wt = wints((Cin, Cout, 4, 4) if kind == 2 else (Cout, Cin, 3, 3))
        b = np.arange(Cout, dtype=np.float32)
        slope = np.array([1.0, 0.25, -0.5, 0.0], np.float32)[np.arange(Cout) % 4]
        Ho, Wo = ((H, W), ((H + 1) // 2, (W + 1) // 2), (2 * H, 2 * W))[kind]
        r = ints((B, Ho, Wo, Cout), 3, 17, 8)
        bufs = [inp("X", X), inp("W", Wt), image("img", L.vd3d_conv_ifn_weight_bytes(kind, Cin, Cout)), inp("bias", b, 4), inp("slope", slope, 4), inp("r", r, 4),
                out("Y", (B, Ho, Wo, Cout), 4)]

        def call(e):
            return (L.vd3d_conv_ifn_pack_weights(e.ctx, kind, e.p["W"], Cin, Cout, e.p["img"])
                    or L.vd3d_conv_ifn(e.ctx, kind, e.p["X"], B, H, W, Cin, Cin, e.p["img"], e.p["bias"], e.p["slope"], Cout, e.p["r"], Cout, e.p["Y"], Cout, 0))

        def wrap(R, t):
            y = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device="cuda", memory_format=torch.channels_last)
            return {"Y": nhwc(R.conv_ifn(kind, nchw(t["X"]), Cin, R.conv_ifn_pack(kind, t["W"]), t["bias"], t["slope"], Cout, y, 0, nchw(t["r"])))}
        x64 = f64(X).permute(0, 3, 1, 2)
        v = (F.conv_transpose2d(x64, f64(Wt), None, 2, 1) if kind == 2 else F.conv2d(x64, f64(Wt), None, kind + 1, 1)).permute(0, 2, 3, 1).numpy() + b.astype(np.float64)
        v = np.where(v >= 0, v, v * slope.astype(np.float64)) + r
        return Case("vd3d_conv_ifn_pack_weights+vd3d_conv_ifn", f"{name} B{B} {H}x{W} Cin{Cin} Cout{Cout} slope r", bufs, call, wrap, {"Y": v})
    return build


for _k, _s in ((0, (1, 17, 31, 48, 64)), (1, (1, 7, 65, 16, 64)), (2, (1, 9, 33, 48, 32))):   # shapes of tests/test_hip_rife_x3.py FAITHFUL
    ROWS.append((f"conv-ifn-{('k3s1', 'k3s2', 't4s2')[_k]}", ifn_row(_k, *_s)))


# ---------------------------------------------------------------------------------------------------------------- the float32 neck / head kernels
@row("dpt-head-conv-f32")
def _dpt_head_conv(L):
    B, (ih, iw), (oh, ow), Cin, Cout = 2, (5, 7), (9, 13), 64, 32   # tests/test_hip_dpt_head_f32.py CASES[0]
    x, b_in, Wt = ints((B, ih, iw, Cin)), ints((Cin,), 3, 7, 3), wints((Cout, Cin, 3, 3))
    b2, w3 = ints((Cout,), 5, 9, 4), ints((Cout,), 3, 5, 2)
    bufs = [inp("x", x), inp("b_in", b_in), inp("W", Wt), image("img", L.vd3d_dpt_head_conv_weight_bytes(Cin, Cout)), inp("b2", b2), inp("w3", w3), out("out", (B, oh, ow))]

    def call(e):
        return (L.vd3d_dpt_head_conv_pack_weights(e.ctx, e.p["W"], Cin, Cout, e.p["img"])
                or L.vd3d_dpt_head_conv_f32(e.ctx, e.p["x"], e.p["b_in"], B, ih, iw, oh, ow, Cin, e.p["img"], Cout, e.p["b2"], e.p["w3"], 0.5, 0.25, e.p["out"]))

    def wrap(R, t):
        return {"out": R.dpt_head_conv(nchw(t["x"]), t["b_in"], (oh, ow), R.dpt_head_conv_pack(t["W"]), t["b2"], t["w3"], 0.5, 0.25)}
    return Case("vd3d_dpt_head_conv_pack_weights+vd3d_dpt_head_conv_f32", f"B{B} {ih}x{iw}->{oh}x{ow} Cin{Cin} Cout{Cout} tail", bufs, call, wrap)


@row("neck-poly")
def _neck_poly(L):
    B, h, w, Cin, Cout, f = 2, 5, 7, 48, 64, 4   # tests/test_hip_neck_poly.py SMALL[0] at MAPS' 5 x 7
    nblk = (f + 2) ** 2
    x, Wc, bc = ints((B, h, w, Cin)), wints((nblk, Cout, Cin)), ints((nblk, Cout), 3, 7, 3)
    bufs = [inp("x", x), inp("Wc", Wc), image("img", L.vd3d_neck_poly_weight_bytes(Cin, Cout, f)), inp("bc", bc), out("out", (B, f * h, f * w, Cout))]

    def call(e):
        return (L.vd3d_neck_poly_pack_f32(e.ctx, e.p["Wc"], Cin, Cout, f, e.p["img"])
                or L.vd3d_neck_poly_conv_f32(e.ctx, e.p["x"], B, h, w, Cin, e.p["img"], e.p["bc"], Cout, f, e.p["out"]))

    def wrap(R, t):
        return {"out": nhwc(R.neck_poly_conv(nchw(t["x"]), R.neck_poly_pack(t["Wc"], t["bc"], f)))}
    return Case("vd3d_neck_poly_pack_f32+vd3d_neck_poly_conv_f32", f"B{B} {h}x{w} Cin{Cin} Cout{Cout} f{f}", bufs, call, wrap)


@row("head-upconv-gather")
def _head_upconv(L):
    B, (h, w), (H, W), Co = 2, (5, 7), (9, 13), 32   # tests/test_head_upconv_host.py MAPS: the non-integer factor
    z = ints((B, h, w, 9, Co))
    bufs = [inp("z", z), out("out", (B, H, W, Co))]
    call = lambda e: L.vd3d_head_upconv_gather_f32(e.ctx, e.p["z"], B, h, w, H, W, Co, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": nhwc(R.head_upconv_gather(t["z"], (H, W), Co))}   # noqa: E731
    return Case("vd3d_head_upconv_gather_f32", f"B{B} {h}x{w}->{H}x{W} Cout{Co}", bufs, call, wrap)


@row("head-conv-gather")
def _head_conv_gather(L):
    B, (ih, iw), (oh, ow), Cin = 2, (5, 7), (9, 13), 32   # tests/test_head_gather_host.py MAPS[0]
    y1, Wt, bc = ints((B, ih, iw, Cin)), wints((288, Cin)), ints((288,), 3, 7, 3)
    b2, w3 = ints((32,), 5, 9, 4), ints((32,), 3, 5, 2)
    bufs = [inp("y1", y1), inp("Wt", Wt), image("img", L.vd3d_head_conv_gather_weight_bytes(Cin)), inp("bc", bc), inp("b2", b2), inp("w3", w3), out("out", (B, oh, ow))]

    def call(e):
        return (L.vd3d_head_conv_gather_pack_weights(e.ctx, e.p["Wt"], Cin, e.p["img"])
                or L.vd3d_head_conv_gather_f32(e.ctx, e.p["y1"], B, ih, iw, oh, ow, Cin, e.p["img"], e.p["bc"], e.p["b2"], e.p["w3"], 0.5, 0.25, e.p["out"]))

    def wrap(R, t):
        return {"out": R.dpt_head_conv(nchw(t["y1"]), None, (oh, ow), R.head_conv_gather_pack(t["Wt"], t["bc"]), t["b2"], t["w3"], 0.5, 0.25, form="gather")}
    return Case("vd3d_head_conv_gather_pack_weights+vd3d_head_conv_gather_f32", f"B{B} {ih}x{iw}->{oh}x{ow} Cin{Cin}", bufs, call, wrap)


def depthpro_head_row(mode):
    B, h, w, Cin = 2, 9, 33, 32   # tests/test_hip_depth_pro_head_poly.py: the ragged map, the small channel count

    def build(L):
        m = MODES[mode]
        x, Wc, T, w3 = ints((B, h, w, Cin)), wints((16, 32, Cin)), ints((3, 3, 32), 3, 7, 3), ints((32,), 3, 5, 2)
        bufs = [inp("x", x), inp("Wc", Wc, 4), image("img", L.vd3d_depthpro_head_weight_bytes(m, Cin)), inp("T", T, 4), inp("w3", w3, 4), out("out", (B, 2 * h, 2 * w), 4)]

        def call(e):
            return (L.vd3d_depthpro_head_pack_weights(e.ctx, m, e.p["Wc"], Cin, e.p["img"])
                    or L.vd3d_depthpro_head(e.ctx, m, e.p["x"], B, h, w, Cin, e.p["img"], e.p["T"], e.p["w3"], 0.5, e.p["out"]))

        def wrap(R, t):
            return {"out": R.depthpro_head(nchw(t["x"]), R.depthpro_head_pack(t["Wc"], mode), t["T"], t["w3"], 0.5, mode)}
        return Case("vd3d_depthpro_head_pack_weights+vd3d_depthpro_head", f"{mode} B{B} {h}x{w} Cin{Cin}", bufs, call, wrap)
    return build


for _mode in MODES:
    ROWS.append((f"depthpro-head-{_mode}", depthpro_head_row(_mode)))


# ---------------------------------------------------------------------------------------------------------------- group norm, layer norm
def gn_row(C, P):
    B, G, eps = 2, 32, 1e-5

    def build(L):
        x, gamma, beta = rnd((B, P, C), C + P), rnd((C,), 1) + 1.0, rnd((C,), 2)
        nb = L.vd3d_groupnorm_nhwc_f32_workspace_bytes(B, P, C, G)
        bufs = [inp("x", x), inp("gamma", gamma), inp("beta", beta), work("workspace", nb), out("out", (B, P, C))]
        call = lambda e: L.vd3d_groupnorm_nhwc_f32(e.ctx, e.p["x"], None, e.p["gamma"], e.p["beta"], eps, 0, B, P, C, G, e.p["workspace"], nb, e.p["out"])   # noqa: E731
        wrap = lambda R, t: {"out": R.groupnorm(t["x"].view(B, P, 1, C), G, t["gamma"], t["beta"], eps)}   # noqa: E731
        return Case("vd3d_groupnorm_nhwc_f32", f"B{B} P{P} C{C} G{G}", bufs, call, wrap)
    return build


for _C in (64, 1024):
    for _P in (1, 7, 577):
        ROWS.append((f"groupnorm-c{_C}-p{_P}", gn_row(_C, _P)))


def ln_row(dtype, cols, rows):
    code = {"bf16": 0, "f32": 1}[dtype]
    name = {"bf16": "bfloat16", "f32": "float32"}[dtype]
    eps = 1e-6

    def build(L):
        conv = (lambda a: a) if dtype == "f32" else bf16_bits
        x, y, g, b = conv(rnd((rows, cols), cols + rows)), conv(rnd((rows, cols), 7)), conv(rnd((cols,), 1) + 1.0), conv(rnd((cols,), 2))
        bufs = [inp("x", x), inp("y", y), inp("gamma", g), inp("beta", b), out("out_sum", (rows, cols), 16, name), out("out_norm", (rows, cols), 16, name)]
        call = lambda e: L.vd3d_add_layernorm(e.ctx, code, e.p["x"], e.p["y"], e.p["gamma"], e.p["beta"], eps, rows, cols, e.p["out_sum"], e.p["out_norm"])   # noqa: E731

        def wrap(R, t):
            v = (lambda a: a) if dtype == "f32" else (lambda a: a.view(torch.bfloat16))
            s, n = R.add_layernorm(v(t["x"]), v(t["y"]), types.SimpleNamespace(weight=v(t["gamma"]), bias=v(t["beta"]), eps=eps))
            return {"out_sum": s, "out_norm": n}
        return Case("vd3d_add_layernorm", f"{dtype} rows{rows} cols{cols}", bufs, call, wrap)
    return build


import test_layernorm_host as _H   # noqa: E402
LN_COLS = (min(_H.COLS), max(_H.COLS))
for _dt in ("f32", "bf16"):
    for _cols in LN_COLS:
        for _rows in (1, 5):
            ROWS.append((f"layernorm-{_dt}-{_cols}-r{_rows}", ln_row(_dt, _cols, _rows)))


# ---------------------------------------------------------------------------------------------------------------- glue rows
HALF = (0.5, 0.5, 0.5)


def c3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def frames_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def upsample_row(dtype, B, Cc, ih, iw, oh, ow):
    code, name = {"bf16": (0, "bfloat16"), "f32": (1, "float32")}[dtype]

    def build(L):
        x = rnd((B, ih, iw, Cc), ih * iw)
        x = x if dtype == "f32" else bf16_bits(x)
        bufs = [inp("in", x), out("out", (B, oh, ow, Cc), 16, name)]
        call = lambda e: L.vd3d_upsample_bilinear_nhwc(e.ctx, code, e.p["in"], e.p["out"], B, ih, iw, oh, ow, Cc)   # noqa: E731

        def wrap(R, t):
            v = t["in"] if dtype == "f32" else t["in"].view(torch.bfloat16)
            return {"out": nhwc(R.upsample_bilinear(nchw(v), (oh, ow)))}
        return Case("vd3d_upsample_bilinear_nhwc", f"{dtype} B{B} C{Cc} {ih}x{iw}->{oh}x{ow}", bufs, call, wrap)
    return build


ROWS.append(("upsample-f32", upsample_row("f32", 1, 8, 1, 5, 4, 9)))      # tests/test_hip_resamplers.py UPSAMPLE_SHAPES: ih = 1
ROWS.append(("upsample-bf16", upsample_row("bf16", 1, 8, 3, 3, 2, 2)))   # tests/test_hip_depthprep.py: the down-sampling one


@row("bias-act")
def _bias_act(L):
    B, Cc, h, w = 3, 4, 5, 7   # tests/test_hip_depthprep.py test_dpt_neck_head_glue_kernels_match_torch
    y, b, r1, r2 = ints((B, h, w, Cc)), np.arange(Cc, dtype=np.float32), ints((B, h, w, Cc), 3, 17, 8), ints((B, h, w, Cc), 5, 19, 9)
    bufs = [inp("y", y), inp("bias", b), inp("r1", r1), inp("r2", r2), out("out", y.shape), out("relu_out", y.shape)]
    call = lambda e: L.vd3d_nhwc_bias_act_f32(e.ctx, e.p["y"], e.p["bias"], e.p["r1"], e.p["r2"], 0, B * h * w, Cc, e.p["out"], e.p["relu_out"])   # noqa: E731

    def wrap(R, t):
        o, ro = R.bias_act(nchw(t["y"].clone()), t["bias"], nchw(t["r1"]), nchw(t["r2"]), False, True)
        return {"out": nhwc(o), "relu_out": nhwc(ro)}
    v = r2.astype(np.float64) + ((y.astype(np.float64) + b) + r1)
    return Case("vd3d_nhwc_bias_act_f32", f"B{B} {h}x{w} C{Cc} bias r1 r2 relu_out", bufs, call, wrap, {"out": v, "relu_out": np.maximum(v, 0)})


@row("upsample-bias")
def _upsample_bias(L):
    B, Cc, ih, iw, oh, ow = 3, 4, 5, 7, 11, 14   # the same test: (2 h + 1, 2 w)
    x, b = rnd((B, ih, iw, Cc), 3), rnd((Cc,), 4)
    bufs = [inp("in", x), inp("bias", b), out("out", (B, oh, ow, Cc))]
    call = lambda e: L.vd3d_upsample_bilinear_bias_nhwc_f32(e.ctx, e.p["in"], e.p["bias"], e.p["out"], B, ih, iw, oh, ow, Cc)   # noqa: E731
    wrap = lambda R, t: {"out": nhwc(R.upsample_bilinear_bias(nchw(t["in"]), (oh, ow), t["bias"]))}   # noqa: E731
    return Case("vd3d_upsample_bilinear_bias_nhwc_f32", f"B{B} C{Cc} {ih}x{iw}->{oh}x{ow}", bufs, call, wrap)


def tail_row(act, n, Cc):
    def build(L):
        y, b2, w3 = rnd((1, 1, n, Cc), n + Cc), rnd((Cc,), 5), rnd((Cc,), 6)
        bufs = [inp("y", y), inp("b2", b2), inp("w3", w3), out("out", (n,))]
        if act is None:
            call = lambda e: L.vd3d_dpt_head_tail_f32(e.ctx, e.p["y"], e.p["b2"], e.p["w3"], 0.25, 1.5, n, Cc, e.p["out"])   # noqa: E731
        else:
            call = lambda e: L.vd3d_dpt_head_tail_act_f32(e.ctx, e.p["y"], e.p["b2"], e.p["w3"], 0.25, 1.5, n, Cc, act, e.p["out"])   # noqa: E731
        wrap = lambda R, t: {"out": R.dpt_head_tail(nchw(t["y"]), t["b2"], t["w3"], 0.25, 1.5, "sigmoid" if act == 1 else "relu")}   # noqa: E731
        return Case("vd3d_dpt_head_tail_f32" if act is None else "vd3d_dpt_head_tail_act_f32", f"n{n} C{Cc}" + ("" if act is None else f" act{act}"), bufs, call, wrap)
    return build


ROWS.append(("head-tail", tail_row(None, 9, 16)))        # tests/test_hip_depthprep.py: (1, 16, 3, 3)
ROWS.append(("head-tail-act", tail_row(1, 17, 16)))      # tests/test_hip_head_tail_act.py: NS' 17, CS' 16


@row("depth-to-space")
def _depth_to_space(L):
    B, H, W, s, Cc = 3, 7, 5, 2, 256   # tests/test_hip_dpt.py
    y, b = ints((B * H * W, s * s * Cc)), np.arange(Cc, dtype=np.float32)
    bufs = [inp("y", y), inp("bias", b), out("out", (B, H * s, W * s, Cc))]
    call = lambda e: L.vd3d_depth_to_space_bias_nhwc_f32(e.ctx, e.p["y"], e.p["bias"], B, H, W, s, Cc, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": nhwc(R.depth_to_space_bias(t["y"], B, H, W, s, t["bias"]))}   # noqa: E731
    v = y.astype(np.float64).reshape(B, H, W, s, s, Cc).transpose(0, 1, 3, 2, 4, 5).reshape(B, H * s, W * s, Cc) + b
    return Case("vd3d_depth_to_space_bias_nhwc_f32", f"B{B} {H}x{W} s{s} C{Cc}", bufs, call, wrap, {"out": v})


@row("patchify")
def _patchify(L):
    B, th, tw, p = 1, 28, 42, 14   # tests/test_hip_self_contained.py
    gh, gw, kp = th // p, tw // p, (3 * p * p + 15) // 16 * 16
    x = ints((B, th, tw, 3))
    bufs = [inp("x", x, 4), out("rows", (B * gh * gw, kp))]
    call = lambda e: L.vd3d_patchify_f32(e.ctx, e.p["x"], B, th, tw, p, e.p["rows"])   # noqa: E731
    wrap = lambda R, t: {"rows": R.patchify(nchw(t["x"]), p)}   # noqa: E731
    v = np.zeros((B * gh * gw, kp))
    v[:, :3 * p * p] = x.reshape(B, gh, p, gw, p, 3).transpose(0, 1, 3, 5, 2, 4).reshape(B * gh * gw, 3 * p * p)
    return Case("vd3d_patchify_f32", f"B{B} {th}x{tw} p{p}", bufs, call, wrap, {"rows": v})


def im2col_row(Cc):
    B, H, W, k, s, pad = 3, 9, 11, 3, 2, (0, 1, 0, 1)   # tests/test_hip_bit_stem.py: (3, 2, 0, 1) on MAPS' 9 x 11

    def build(L):
        x = ints((B, H, W, Cc))
        Ho, Wo, kp = (H + 1 - k) // s + 1, (W + 1 - k) // s + 1, (k * k * Cc + 15) // 16 * 16
        bufs = [inp("x", x, 16 if Cc % 4 == 0 else 4), out("rows", (B, Ho, Wo, kp))]
        call = lambda e: L.vd3d_im2col_nhwc_f32(e.ctx, e.p["x"], B, H, W, Cc, k, s, *pad, e.p["rows"])   # noqa: E731
        wrap = lambda R, t: {"rows": R.im2col(t["x"], k, s, pad)}   # noqa: E731
        xp = F.pad(f64(x).permute(0, 3, 1, 2), (pad[2], pad[3], pad[0], pad[1]))
        cols = F.unfold(xp, k, stride=s).view(B, Cc, k, k, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(B, Ho, Wo, k * k * Cc)
        return Case("vd3d_im2col_nhwc_f32", f"B{B} {H}x{W} C{Cc} k{k} s{s} pad{pad}", bufs, call, wrap, {"rows": F.pad(cols, (0, kp - k * k * Cc)).numpy()})
    return build


ROWS.append(("im2col-c3", im2col_row(3)))
ROWS.append(("im2col-c16", im2col_row(16)))


@row("maxpool")
def _maxpool(L):
    B, H, W, Cc, pad = 3, 9, 11, 4, (0, 1, 0, 1)   # tests/test_hip_bit_stem.py
    x = rnd((B, H, W, Cc), 10 * H + Cc + B) - 1.0
    Ho, Wo = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
    bufs = [inp("x", x), out("out", (B, Ho, Wo, Cc))]
    call = lambda e: L.vd3d_maxpool3x3_s2_nhwc_f32(e.ctx, e.p["x"], B, H, W, Cc, *pad, 0.0, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": R.maxpool3x3_s2(t["x"], pad, 0.0)}   # noqa: E731
    v = F.max_pool2d(F.pad(f64(x).permute(0, 3, 1, 2), (0, 1, 0, 1), value=0.0), 3, 2).permute(0, 2, 3, 1).numpy()
    return Case("vd3d_maxpool3x3_s2_nhwc_f32", f"B{B} {H}x{W} C{Cc} pad{pad}", bufs, call, wrap, {"out": v})


@row("depthpro-preprocess")
def _dp_pre(L):
    B, H, W, S = 2, 270, 481, 256   # tests/test_hip_depth_pro_kernels.py
    fr = frames_u8((B, H, W, 3), 100 + H + W)
    bufs = [inp("frames", fr), out("out", (B, 3, S, S))]
    call = lambda e: L.vd3d_depthpro_preprocess_u8(e.ctx, e.p["frames"], B, H, W, S, c3(HALF), c3(HALF), e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": R.depthpro_preprocess(t["frames"], S, HALF, HALF)}   # noqa: E731
    return Case("vd3d_depthpro_preprocess_u8", f"B{B} {H}x{W}->{S}", bufs, call, wrap)


@row("depthpro-post")
def _dp_post(L):
    B, S, oH, oW = 2, 24, 31, 45   # tests/test_hip_depth_pro_kernels.py, with the field of view
    pred = (np.abs(rnd((B, S, S), 7)) * 10 + 0.05).astype(np.float32)
    fov = np.array([27.5, 91.0], np.float32)
    bufs = [inp("pred", pred), inp("fov", fov), out("out", (B, oH, oW))]
    call = lambda e: L.vd3d_depthpro_post_f32(e.ctx, e.p["pred"], e.p["fov"], B, S, oH, oW, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": R.depthpro_post(t["pred"], t["fov"], oH, oW)}   # noqa: E731
    return Case("vd3d_depthpro_post_f32", f"B{B} S{S}->{oH}x{oW} fov", bufs, call, wrap)


@row("depthpro-patches")
def _dp_patches(L):
    from visiondepth3d_amd import depth_pro
    B, S, p = 2, 80, 20   # tests/test_hip_depth_pro_pyramid.py: strides 15 / 10, the 4-byte form
    lv = depth_pro.pyramid_levels(S, p)
    st = [lv[2][2], lv[1][2], lv[0][2]]
    n = int(L.vd3d_depthpro_patches_count(S, p, *st))
    assert n == lv[0][3] ** 2 + lv[1][3] ** 2 + lv[2][3] ** 2
    x = ints((B, 3, S, S), 1, 251, 125)
    bufs = [inp("pixel_values", x, 4), out("patches", (n * B, p, p, 3), 4)]
    call = lambda e: L.vd3d_depthpro_patches_f32(e.ctx, e.p["pixel_values"], B, S, p, *st, e.p["patches"])   # noqa: E731
    wrap = lambda R, t: {"patches": nhwc(R.depthpro_patches(t["pixel_values"], p, st))}   # noqa: E731
    return Case("vd3d_depthpro_patches_f32", f"B{B} S{S} p{p} strides{tuple(st)}", bufs, call, wrap)


@row("depthpro-merge")
def _dp_merge(L):
    n, B, g, padding, Cc, o = 9, 3, 4, 6, 8, 10   # tests/test_hip_depth_pro_pyramid.py: (9, 6, 4), C 8, the class token, out = M + M // 3
    T = g * g + 1
    rows = rnd((n * B, T, Cc), 11)
    bufs = [inp("rows", rows, 4), out("out", (B, o, o, Cc), 4)]
    call = lambda e: L.vd3d_depthpro_merge_f32(e.ctx, e.p["rows"], n, B, T, Cc, g, padding, o, o, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": R.depthpro_merge(t["rows"], B, g, padding, o, o)}   # noqa: E731
    return Case("vd3d_depthpro_merge_f32", f"n{n} B{B} T{T} C{Cc} g{g} pad{padding}->{o}x{o}", bufs, call, wrap)


def zoe_pre_row(H, W, target):
    def build(L):
        from visiondepth3d_amd import zoedepth
        B, (th, tw) = 2, target
        ph, pw = zoedepth.pad_amounts(H, W)
        fr, table = frames_u8((B, H, W, 3), 100 + H + W), zoedepth.rescale_table().numpy()
        bufs = [inp("frames", fr, 4), inp("table", table, 4), out("out", (B, th, tw, 3), 4)]
        call = lambda e: L.vd3d_zoedepth_preprocess_u8(e.ctx, e.p["frames"], e.p["table"], B, H, W, ph, pw, th, tw, c3(HALF), c3(HALF), e.p["out"])   # noqa: E731
        wrap = lambda R, t: {"out": nhwc(R.zoedepth_preprocess(t["frames"], (ph, pw), target, HALF, HALF, t["table"]))}   # noqa: E731
        return Case("vd3d_zoedepth_preprocess_u8", f"B{B} {H}x{W} pad{(ph, pw)}->{th}x{tw}", bufs, call, wrap)
    return build


ROWS.append(("zoedepth-preprocess-5x5", zoe_pre_row(5, 5, (32, 32))))        # tests/test_hip_zoedepth_kernels.py
ROWS.append(("zoedepth-preprocess-37x53", zoe_pre_row(37, 53, (64, 96))))


@row("zoedepth-post")
def _zoe_post(L):
    from visiondepth3d_amd import zoedepth
    B, th, tw, H, W = 2, 24, 32, 17, 23   # tests/test_hip_zoedepth_kernels.py: the output smaller than the prediction
    ph, pw = zoedepth.pad_amounts(H, W)
    pred = (np.abs(rnd((B, th, tw), 5)) * 3 + 0.5).astype(np.float32)
    bufs = [inp("pred", pred), out("out", (B, H, W))]
    call = lambda e: L.vd3d_zoedepth_post_f32(e.ctx, e.p["pred"], B, th, tw, H, W, ph, pw, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": R.zoedepth_post(t["pred"], H, W, (ph, pw))}   # noqa: E731
    return Case("vd3d_zoedepth_post_f32", f"B{B} {th}x{tw}->{H}x{W} pad{(ph, pw)}", bufs, call, wrap)


@row("zoedepth-attractor")
def _zoe_attractor(L):
    B, h, w, hp, wp, nA, nb = 2, 7, 11, 4, 6, 4, 20   # tests/test_hip_zoedepth_kernels.py GEOMETRIES[0]
    rng = np.random.default_rng(nA * 100 + nb)
    att, prev = rng.uniform(0, 3, (B, h, w, nA)).astype(np.float32), rng.uniform(0, 3, (B, hp, wp, nb)).astype(np.float32)
    bufs = [inp("attractors", att), inp("prev_bins", prev), out("out", (B, h, w, nb))]
    call = lambda e: L.vd3d_zoedepth_attractor_f32(e.ctx, e.p["attractors"], e.p["prev_bins"], B, h, w, hp, wp, nA, nb, 1, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": R.zoedepth_attractor(t["attractors"], t["prev_bins"], "mean")}   # noqa: E731
    return Case("vd3d_zoedepth_attractor_f32", f"B{B} {h}x{w} prev{hp}x{wp} nA{nA} nb{nb} mean", bufs, call, wrap)


@row("zoedepth-bins")
def _zoe_bins(L):
    B, H, W, hc, wc, Ch, nb = 2, 9, 13, 5, 7, 32, 20   # tests/test_hip_zoedepth_kernels.py: the odd map, with the relative-depth plane
    rng = np.random.default_rng(9)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)   # noqa: E731
    ops = dict(last=u(-1, 1, B, H, W, 32), rel=u(0, 1, B, H, W), wrel=u(-1, 1, Ch), P=u(-1, 1, B, hc, wc, Ch), bins=u(0.5, 10, B, hc, wc, nb), w1_last=u(-.3, .3, Ch, 32),
               b1=u(-1, 1, Ch), w2=u(-1, 1, 4, Ch), b2=u(-1, 1, 4),
               table=np.array([math.lgamma(nb) - math.lgamma(k + 1) - math.lgamma(nb - k) for k in range(nb)], np.float32))
    order = ("last", "rel", "wrel", "P", "bins", "w1_last", "b1", "w2", "b2", "table")
    bufs = [inp(k, ops[k]) for k in order] + [out("out", (B, H, W))]
    call = lambda e: L.vd3d_zoedepth_bins_f32(e.ctx, *[e.p[k] for k in order], 5.0, 50.0, B, H, W, hc, wc, Ch, nb, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": R.zoedepth_bins(*[t[k] for k in order], 5.0, 50.0)}   # noqa: E731
    return Case("vd3d_zoedepth_bins_f32", f"B{B} {H}x{W} coarse{hc}x{wc} Ch{Ch} nb{nb} rel", bufs, call, wrap)


def prep_row(dtype):
    code, name, tdt = {"bf16": (0, "bfloat16", torch.bfloat16), "f32": (1, "float32", torch.float32)}[dtype]
    B, H, W, th, tw = 1, 33, 65, 8, 16   # tests/test_hip_resamplers.py PREP_SHAPES: narrower than a strip

    def build(L):
        from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD
        fr = frames_u8((B, H, W, 3), H + W)
        bufs = [inp("frames", fr), out("out", (B, th, tw, 3), 16, name)]
        call = lambda e: L.vd3d_depth_preprocess(e.ctx, e.p["frames"], B, H, W, th, tw, c3(IMAGENET_MEAN), c3(IMAGENET_STD), code, e.p["out"])   # noqa: E731
        wrap = lambda R, t: {"out": nhwc(R.depth_preprocess(t["frames"], th, tw, IMAGENET_MEAN, IMAGENET_STD, tdt))}   # noqa: E731
        return Case("vd3d_depth_preprocess", f"{dtype} B{B} {H}x{W}->{th}x{tw}", bufs, call, wrap)
    return build


ROWS.append(("depth-preprocess-f32", prep_row("f32")))
ROWS.append(("depth-preprocess-bf16", prep_row("bf16")))


@row("depth-preprocess-pil")
def _prep_pil(L):
    from visiondepth3d_amd.depth import IMAGENET_MEAN, IMAGENET_STD
    B, H, W, th, tw = 3, 54, 96, 26, 47   # tests/test_hip_pil_front_end.py GEOMETRIES[0]
    fr = frames_u8((B, H, W, 3), H * 1000 + tw)
    bufs = [inp("frames", fr), out("out", (B, th, tw, 3))]
    call = lambda e: L.vd3d_depth_preprocess_pil(e.ctx, e.p["frames"], B, H, W, 0, 0, th, tw, c3(IMAGENET_MEAN), c3(IMAGENET_STD), 1, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": nhwc(R.depth_preprocess_pil(t["frames"], th, tw, IMAGENET_MEAN, IMAGENET_STD))}   # noqa: E731
    return Case("vd3d_depth_preprocess_pil", f"f32 B{B} {H}x{W}->{th}x{tw}", bufs, call, wrap)


@row("resize-pil-bicubic")
def _resize_pil(L):
    B, H, W, h, w = 3, 54, 96, 26, 47   # tests/test_hip_pil_front_end.py GEOMETRIES[0]
    fr = frames_u8((B, H, W, 3), H * 1000 + w)
    bufs = [inp("src", fr), out("dst", (B, h, w, 3), 16, "uint8")]
    call = lambda e: L.vd3d_resize_pil_bicubic_u8(e.ctx, e.p["src"], B, H, W, e.p["dst"], h, w)   # noqa: E731
    wrap = lambda R, t: {"dst": R.resize_pil_bicubic_u8(t["src"], h, w)}   # noqa: E731
    return Case("vd3d_resize_pil_bicubic_u8", f"B{B} {H}x{W}->{h}x{w}", bufs, call, wrap)


@row("depth-handoff")
def _handoff(L):
    B, ph, pw, H, W = 2, 2, 2, 7, 5   # tests/test_hip_resamplers.py HANDOFF_SHAPES
    pred = rnd((B, ph, pw), 13, 3.0) + 5
    bufs = [inp("pred", pred), out("out_gray", (B, H, W), 16, "uint8")]
    call = lambda e: L.vd3d_depth_handoff(e.ctx, e.p["pred"], B, ph, pw, H, W, 0, e.p["out_gray"])   # noqa: E731
    wrap = lambda R, t: {"out_gray": R.depth_handoff(t["pred"], H, W)}   # noqa: E731
    return Case("vd3d_depth_handoff", f"B{B} {ph}x{pw}->{H}x{W}", bufs, call, wrap)


TILE_GEOM = (40, 50, 64, 8)   # tests/test_hip_depth_tiles.py SMALL_GEOMETRIES: the smallest


@row("tile-gather")
def _tile_gather(L):
    from visiondepth3d_amd import depth_tiles as DT
    H, W, tile, pad = TILE_GEOM
    B = 2
    plan = DT.tile_plan(H, W, tile, pad)
    g = plan.groups[0]
    org = plan.gather_origins(g, B)
    n = org.shape[0]
    fr = frames_u8((B, H, W, 3), 11)
    bufs = [inp("frames", fr), inp("origins", org), out("out_tiles", (n, g.chs, g.cws, 3), 16, "uint8")]
    call = lambda e: L.vd3d_tile_gather_cubic_u8(e.ctx, e.p["frames"], W * 3, H * W * 3, B, H, W, e.p["origins"], n, g.ch, g.cw, g.chs, g.cws, e.p["out_tiles"])   # noqa: E731
    wrap = lambda R, t: {"out_tiles": R.tile_gather_cubic_u8(t["frames"], t["origins"], g.ch, g.cw, g.chs, g.cws)}   # noqa: E731
    return Case("vd3d_tile_gather_cubic_u8", f"B{B} {H}x{W} tile{tile} pad{pad} crop{g.ch}x{g.cw}->{g.chs}x{g.cws} n{n}", bufs, call, wrap)


@row("tile-blend")
def _tile_blend(L):
    from visiondepth3d_amd import depth_tiles as DT
    H, W, tile, pad = TILE_GEOM
    B = 2
    plan = DT.tile_plan(H, W, tile, pad)
    tab, off, total = plan.blend_tables(B, [(g.chs, g.cws) for g in plan.groups])
    pool, wp = rnd((total,), H * 7 + W, 3.0), plan.weight_pool().astype(np.float32)
    bufs = [inp("pred_pool", pool), inp("pred_off", off.reshape(-1)), inp("tile_tab", tab), inp("w_pool", wp), out("out", (B, H, W))]
    call = lambda e: L.vd3d_tile_blend_f32(e.ctx, e.p["pred_pool"], e.p["pred_off"], e.p["tile_tab"], e.p["w_pool"], B, H, W, tile, pad, e.p["out"])   # noqa: E731
    wrap = lambda R, t: {"out": R.tile_blend(t["pred_pool"], t["pred_off"], t["tile_tab"], t["w_pool"], B, H, W, tile, pad)}   # noqa: E731
    return Case("vd3d_tile_blend_f32", f"B{B} {H}x{W} tile{tile} pad{pad} tiles{plan.n_tiles}", bufs, call, wrap)


@row("depth-normalize-pclip")
def _normalize(L):
    B, H, W = 3, 50, 37   # tests/test_hip_depth_tiles.py
    planes = rnd((B, H, W), H + W)
    planes[1].reshape(-1)[::50] = 1e5   # 2 % outliers: the percentiles are not the extremes
    bufs = [inp("planes", planes), out("out_gray", (B, H, W), 16, "uint8"), out("lo_hi", (B, 2))]
    call = lambda e: L.vd3d_depth_normalize_pclip_u8(e.ctx, e.p["planes"], B, H, W, 1.0, 99.0, 0, e.p["out_gray"], e.p["lo_hi"])   # noqa: E731

    def wrap(R, t):
        lohi = torch.zeros((B, 2), dtype=torch.float32, device="cuda")
        return {"out_gray": R.depth_normalize_pclip(t["planes"], lo_hi=lohi), "lo_hi": lohi}
    return Case("vd3d_depth_normalize_pclip_u8", f"B{B} {H}x{W} p1-99 lo_hi", bufs, call, wrap)


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_required_rows_are_present():
    ids = [r for r, _ in ROWS]
    assert len(ids) == len(set(ids))
    for must in ("gemm-bf16x3-1x16x1-b0", "gemm-fp16x2-255x80x257-b1", "gemm-bf16x3-257x48x255-gelu", "attn-bf16x3-T257", "attn-fp16x2-T1", "attn-4-T65", "attn-8-T33",
                 "conv-x3-c48-256-2x13x47", "conv-s1_x2-c16-32-1x1x1", "conv-x2-c48-128-2x13x47", "conv-s2_x3-c16-128-1x2x2", "conv-s2_x2-c48-256-2x25x93",
                 "conv-epi-bf16x3", "conv-epi-fp16x2", "conv-ifn-k3s1", "conv-ifn-k3s2", "conv-ifn-t4s2", "dpt-head-conv-f32", "neck-poly", "head-upconv-gather",
                 "head-conv-gather", "depthpro-head-bf16x3", "depthpro-head-fp16x2", "groupnorm-c64-p1", "groupnorm-c1024-p577", "layernorm-f32-384-r1",
                 "layernorm-bf16-1024-r5",
                 # the glue rows: every one the issue lists
                 "upsample-f32", "upsample-bf16", "bias-act", "upsample-bias", "head-tail", "head-tail-act", "depth-to-space", "patchify", "im2col-c3", "im2col-c16",
                 "maxpool", "depthpro-preprocess", "depthpro-post", "depthpro-patches", "depthpro-merge", "zoedepth-preprocess-5x5", "zoedepth-preprocess-37x53",
                 "zoedepth-post", "zoedepth-attractor", "zoedepth-bins", "depth-preprocess-f32", "depth-preprocess-bf16", "depth-preprocess-pil",
                 "resize-pil-bicubic", "depth-handoff", "tile-gather", "tile-blend", "depth-normalize-pclip"):
        assert must in ids, must


@pytest.mark.parametrize("rid,build", ROWS, ids=[r for r, _ in ROWS])
def test_arena(R, rid, build):
    arena.check_case(build(R._L), "cuda", R)


# ---------------------------------------------------------------------------------------------------------------- the wrapper level
@pytest.mark.parametrize("mode", list(MODES))
def test_attention_x3_cached_workspace_is_rebuilt_by_every_call(R, mode):
    """``Renderer.attention_x3`` keeps one workspace and grows it on demand: after a call at T = 257 the workspace is overwritten with 0xFF, and a call at T = 33
    still has the bits of a fresh renderer's -- no row of the larger image, and no byte the smaller call's prep does not rewrite, reaches the result."""
    from visiondepth3d_amd.render_3d import Renderer
    B, H, D = 2, 2, 64
    scale = D ** -0.5
    big, small = torch.from_numpy(rnd((B, 257, 3 * H * D), 1)).cuda(), torch.from_numpy(rnd((B, 33, 3 * H * D), 2)).cuda()
    R.attention_x3(big, H, scale, mode)
    torch.cuda.synchronize()
    assert R._attn_ws.numel() >= R._L.vd3d_attention_x3_workspace_bytes(B, 257, H, D, MODES[mode])
    R._attn_ws.fill_(0xFF)
    got = R.attention_x3(small, H, scale, mode)
    fresh = Renderer(0)
    try:
        want = fresh.attention_x3(small, H, scale, mode)
        torch.cuda.synchronize()
    finally:
        fresh.close()
    assert bool(torch.isfinite(got).all()) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    print(f"ARENA Renderer.attention_x3 {mode} T257->0xFF->T33 fills=1 guards=n/a bits=same exact=n/a")


PACKS = [("gemm_x3_pack-bf16x3", lambda R: R.gemm_x3_pack(torch.from_numpy(wints((255, 48))), "bf16x3")),
         ("gemm_x3_pack-fp16x2", lambda R: R.gemm_x3_pack(torch.from_numpy(wints((255, 48))), "fp16x2")),
         ("conv3x3_x2_pack", lambda R: R.conv3x3_x2_pack(torch.from_numpy(wints((64, 48, 3, 3))))),
         ("conv3x3_x3_pack", lambda R: R.conv3x3_x3_pack(torch.from_numpy(wints((256, 48, 3, 3))))),
         ("conv3x3_s2_x3_pack", lambda R: R.conv3x3_s2_x3_pack(torch.from_numpy(wints((256, 48, 3, 3))))),
         ("conv3x3_s1_x2_pack", lambda R: R.conv3x3_s1_x2_pack(torch.from_numpy(wints((256, 48, 3, 3))))),
         ("conv3x3_s2_x2_pack", lambda R: R.conv3x3_s2_x2_pack(torch.from_numpy(wints((256, 48, 3, 3))))),
         ("conv_ifn_pack-k3s1", lambda R: R.conv_ifn_pack(0, torch.from_numpy(wints((96, 48, 3, 3))))),
         ("conv_ifn_pack-k3s2", lambda R: R.conv_ifn_pack(1, torch.from_numpy(wints((64, 16, 3, 3))))),
         ("conv_ifn_pack-t4s2", lambda R: R.conv_ifn_pack(2, torch.from_numpy(wints((48, 32, 4, 4))))),
         ("depthpro_head_pack-bf16x3", lambda R: R.depthpro_head_pack(torch.from_numpy(wints((16, 32, 48))), "bf16x3")),
         ("depthpro_head_pack-fp16x2", lambda R: R.depthpro_head_pack(torch.from_numpy(wints((16, 32, 48))), "fp16x2")),
         ("dpt_head_conv_pack", lambda R: R.dpt_head_conv_pack(torch.from_numpy(wints((32, 64, 3, 3))))),
         ("head_conv_gather_pack", lambda R: R.head_conv_gather_pack(torch.from_numpy(wints((288, 32))), torch.from_numpy(ints((288,))))),
         ("neck_poly_pack", lambda R: R.neck_poly_pack(torch.from_numpy(wints((36, 64, 48))), torch.from_numpy(ints((36, 64))), 4))]


@pytest.mark.parametrize("name,pack", PACKS, ids=[n for n, _ in PACKS])
def test_pack_wrapper_leaves_no_byte_of_its_image_to_the_allocator(R, monkeypatch, name, pack):
    """Every ``*_pack`` wrapper allocates its image with ``torch.empty``.  Here that allocation comes back filled with 0xFF, then with 0x47: the two images are
    equal over all of ``*_weight_bytes``, so the packer wrote every byte (zero pages, column scales and padding included)."""
    real = torch.empty
    images = []
    for fill in (0xFF, 0x47):
        def empty(*a, _fill=fill, **k):
            t = real(*a, **k)
            return t.fill_(_fill) if t.dtype == torch.uint8 else t
        monkeypatch.setattr(torch, "empty", empty)
        got = pack(R)
        monkeypatch.setattr(torch, "empty", real)
        img = got[0] if isinstance(got, tuple) else got
        assert img is not None and img.dtype == torch.uint8
        torch.cuda.synchronize()
        images.append(img.cpu().numpy())
    d = np.flatnonzero(images[0] != images[1])
    assert d.size == 0, f"{name}: {d.size} of {images[0].size} image bytes are the allocator's, first at byte offset {int(d[0])}"
    print(f"ARENA Renderer.{name} image{images[0].size} fills=2 guards=n/a bits=same exact=n/a")
