"""GPU tests (-m gpu) of vd3d_conv3x3_epi (csrc/vd3d_conv_epi.hip: the stride-1 tile convolution of vd3d_conv_x3.h with vd3d_nhwc_bias_act_f32's chain in its
epilogue, EPI 2), both arithmetics.  The contract is equality of BITS with the launches it replaces,
    [torch.relu ->] Renderer.conv3x3_tile (bias-free) -> Renderer.bias_act,
on random normal data with negatives, for every argument set DepthPipe(decoder=...) uses and the one with the ReLU'd copy; plus containment (a NaN frame behind
the batch, sentinel frames behind the outputs, a NaN pixel that must reach exactly its 3 x 3 windows) and the refusals, which must write nothing."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
CL = torch.channels_last
MODES = ["bf16x3", "fp16x2"]

SHAPES = [(1, 1, 1, 16, 32),       # one pixel
          (2, 9, 33, 32, 64),      # one row and one column past a tile
          (1, 8, 32, 16, 256),     # two channel slices
          (3, 17, 40, 48, 128)]    # three chunks, three frames, 3 x 2 tiles
# name -> (relu_in, bias, r1, r2, relu, relu copy): the four sets of the issue (the decoder's three residual-unit forms and head.layers.0) and the decoder's
# second convolution of residual_layer1 as it routes it, without the copy
SETS = {"relu_in+bias+relu": (True, True, False, False, True, False),
        "bias+r1": (False, True, True, False, False, False),
        "bias+r1+r2+yrelu": (False, True, True, True, False, True),
        "bias+r1+r2": (False, True, True, True, False, False),
        "bias": (False, True, False, False, False, False)}


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _operands(B, H, W, Cin, Cout, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, Cin, H, W, device="cuda", generator=g).contiguous(memory_format=CL)
    w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) * 0.05
    bias = torch.randn(Cout, device="cuda", generator=g)
    r1 = torch.randn(B, Cout, H, W, device="cuda", generator=g).contiguous(memory_format=CL)
    r2 = torch.randn(B, Cout, H, W, device="cuda", generator=g).contiguous(memory_format=CL)
    return x, w, bias, r1, r2


def _pair(R, mode, x, img, Cout, s, bias, r1, r2):
    """The launches the kernel replaces."""
    relu_in, ub, u1, u2, relu, copy = SETS[s]
    y = R.conv3x3_tile(torch.relu(x) if relu_in else x, img, Cout, mode, 1)
    out = R.bias_act(y, bias if ub else None, r1=r1 if u1 else None, r2=r2 if u2 else None, relu=relu, want_relu_copy=copy)
    return out if copy else (out, None)


def _fused(R, mode, x, img, Cout, s, bias, r1, r2):
    relu_in, ub, u1, u2, relu, copy = SETS[s]
    out = R.conv3x3_epi(x, img, Cout, mode, bias=bias if ub else None, r1=r1 if u1 else None, r2=r2 if u2 else None, relu_in=relu_in, relu=relu, want_relu_copy=copy)
    return out if copy else (out, None)


@pytest.mark.parametrize("s", list(SETS))
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_epi_equals_the_pair_it_replaces_on_bits(R, mode, B, H, W, Cin, Cout, s):
    x, w, bias, r1, r2 = _operands(B, H, W, Cin, Cout, 7 * H + Cout)
    assert float(x.min()) < 0 or x.numel() < 64
    img = R.conv3x3_tile_pack(w, mode, 1)
    (y, yr), (ey, eyr) = _fused(R, mode, x, img, Cout, s, bias, r1, r2), _pair(R, mode, x, img, Cout, s, bias, r1, r2)
    assert y.shape == (B, Cout, H, W) and y.is_contiguous(memory_format=CL) and bool(torch.isfinite(y).all())
    assert torch.equal(y, ey) and torch.equal(_bits(y), _bits(ey))
    assert (yr is None) == (eyr is None)
    if yr is not None:
        assert torch.equal(_bits(yr), _bits(eyr)) and float(yr.min()) == 0.0 and float(y.min()) < 0
    if SETS[s][4]:
        assert float(y.min()) >= 0.0 and float((y == 0).float().mean()) > 0.1    # the ReLU engaged
    again = _fused(R, mode, x, img, Cout, s, bias, r1, r2)[0]
    assert torch.equal(_bits(again), _bits(y))


@pytest.mark.parametrize("mode", MODES)
def test_epi_reads_and_writes_nothing_past_its_frames(R, mode):
    """One buffer per operand with a frame more than the call is told about: NaN behind X, r1 and r2 (a read past the batch poisons the output), a sentinel
    behind Y and Yrelu (a write past the batch destroys it).  Frame B - 1 must equal the same frame computed alone."""
    B, H, W, Cin, Cout = 2, 9, 33, 32, 64
    x, w, bias, r1, r2 = _operands(B + 1, H, W, Cin, Cout, 3)
    img = R.conv3x3_tile_pack(w, mode, 1)
    for t in (x, r1, r2):
        t[B:] = float("nan")
    ybuf = torch.full((B + 1, Cout, H, W), -7.25, device="cuda").contiguous(memory_format=CL)
    rbuf = torch.full((B + 1, Cout, H, W), -9.5, device="cuda").contiguous(memory_format=CL)
    L, vp = R._L, ctypes.c_void_p
    R._enter(x, img, ybuf, rbuf)
    rc = L.vd3d_conv3x3_epi(R._ctx, R.X3_MODES[mode], vp(x.data_ptr()), B, H, W, Cin, vp(img.data_ptr()), Cout, 0, vp(bias.data_ptr()), vp(r1.data_ptr()),
                            vp(r2.data_ptr()), vp(ybuf.data_ptr()), vp(rbuf.data_ptr()))
    assert rc == 0, L.vd3d_last_error()
    assert bool(torch.isfinite(ybuf).all()) and bool((ybuf[B:] == -7.25).all()) and bool((rbuf[B:] == -9.5).all())
    ey, eyr = _pair(R, mode, x[:B], img, Cout, "bias+r1+r2+yrelu", bias, r1[:B], r2[:B])
    assert torch.equal(_bits(ybuf[:B]), _bits(ey)) and torch.equal(_bits(rbuf[:B]), _bits(eyr))
    one = R.conv3x3_epi(x[B - 1:B], img, Cout, mode, bias=bias, r1=r1[B - 1:B], r2=r2[B - 1:B])
    assert torch.equal(_bits(one), _bits(ybuf[B - 1:B]))


@pytest.mark.parametrize("relu_in", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_a_nan_pixel_reaches_exactly_its_windows(R, mode, relu_in):
    """A NaN input pixel makes the outputs whose 3 x 3 window holds it NaN over all channels (also under RELU_IN: the ReLU in front of the split keeps it) and
    leaves every other output's bits as they are without it.  Positions on a tile seam and in a corner, in the second frame of two."""
    B, H, W, Cin, Cout = 2, 17, 40, 32, 64
    x, w, bias, r1, _ = _operands(B, H, W, Cin, Cout, 5)
    img = R.conv3x3_tile_pack(w, mode, 1)
    clean = R.conv3x3_epi(x, img, Cout, mode, bias=bias, r1=r1, relu_in=relu_in)
    for (py, px) in ((8, 32), (0, 0), (16, 39)):
        xn = x.clone()
        xn[1, 5, py, px] = float("nan")
        y = R.conv3x3_epi(xn, img, Cout, mode, bias=bias, r1=r1, relu_in=relu_in)
        hit = torch.zeros(B, 1, H, W, dtype=torch.bool, device="cuda")
        hit[1, 0, max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
        assert bool(torch.isnan(y)[hit.expand_as(y)].all()), (py, px)
        assert torch.equal(_bits(y)[~hit.expand_as(y)], _bits(clean)[~hit.expand_as(y)]), (py, px)


@pytest.mark.parametrize("mode", MODES)
def test_refusals_write_nothing(R, mode):
    B, H, W, Cin, Cout = 1, 8, 32, 32, 32
    x, w, bias, r1, r2 = _operands(B, H, W, Cin, Cout, 9)     # Cin == Cout: every map has the output's size, so any of them can be offered as the output
    img = R.conv3x3_tile_pack(w, mode, 1)
    L, vp, m = R._L, ctypes.c_void_p, R.X3_MODES[mode]
    y = torch.full_like(r1, 3.5)
    R._enter(x, img, y)

    def call(X=x, Y=y, Yr=None, a=r1, b=r2, cin=Cin, cout=Cout, flags=0, mode_=m, batch=B, h=H):
        return L.vd3d_conv3x3_epi(R._ctx, mode_, vp(X.data_ptr()) if torch.is_tensor(X) else vp(X), batch, h, W, cin, vp(img.data_ptr()), cout, flags,
                                  vp(bias.data_ptr()), vp(a.data_ptr()), vp(b.data_ptr()), vp(Y.data_ptr()), vp(Yr.data_ptr()) if Yr is not None else None)
    before = [t.clone() for t in (x, r1, r2)]
    for kw, word in ((dict(Y=x), b"overlaps"), (dict(Y=r1), b"overlaps"), (dict(Y=r2), b"overlaps"), (dict(Yr=x), b"overlaps"), (dict(Yr=r2), b"overlaps"),
                     (dict(Yr=y), b"overlaps")):
        assert call(**kw) == -4 and word in L.vd3d_last_error(), kw
    assert call(cin=24) == -4 and b"C_in 24" in L.vd3d_last_error()
    assert call(cout=96) == -4 and b"C_out 96" in L.vd3d_last_error()
    assert call(batch=0) == -4 and b"batch" in L.vd3d_last_error()
    assert call(h=0) == -4 and b"map" in L.vd3d_last_error()
    assert call(X=x.data_ptr() + 4) == -4 and b"aligned" in L.vd3d_last_error()
    assert call(flags=4) != 0 and b"flags" in L.vd3d_last_error()
    assert call(mode_=2) != 0 and b"mode" in L.vd3d_last_error()
    torch.cuda.synchronize()
    assert bool((y == 3.5).all()) and all(torch.equal(_bits(t), _bits(b4)) for t, b4 in zip((x, r1, r2), before))
    assert call() == 0
    assert torch.equal(_bits(y), _bits(R.conv3x3_epi(x, img, Cout, mode, bias=bias, r1=r1, r2=r2)))
