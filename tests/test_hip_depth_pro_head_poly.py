"""GPU tests (-m gpu) of vd3d_depthpro_head (csrc/vd3d_depthpro_head.hip: the tile convolution's T4S2 geometry with 32 output channels and the head's tail in
its epilogue, EPI 3), both arithmetics: everything behind head.layers.0 of DepthProDepthEstimationHead,
    ConvTranspose2d(C, C, 2, 2) + bt -> Conv2d(C, 32, 3, padding 1) + b2 -> ReLU -> Conv2d(32, 1, 1) + b3 -> ReLU,
as one launch on the coarse map.  The reference is the MODULE chain in float64 on the CPU.
  * Integer operands (ternary weights of density 0.25, inputs in [-2, 2]): every sum is exact in any order, so the kernel must EQUAL the float64 chain -- that pins
    the phase, the tap, the border class of the bias table, the frame seam and the weight image.
  * Random operands: the float32 torch chain on the CPU is the yardstick, the bars are the tile convolution's own (tests/test_hip_conv_x3.py,
    test_hip_conv_fp16x2.py): maximum error <= max(2.5 x the yardstick's, 2^-21), RMS <= 1.5 x the yardstick's.  The ratios are printed (DEPTHPRO_HEAD_ERR)."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
CL = torch.channels_last
MODES = ["bf16x3", "fp16x2"]


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def chain(x, wt, bt, w3, b2, w1, b3, mag=False):
    """The module chain in x's dtype; ``mag``: on magnitudes and without the ReLUs -- the sum of the absolute values of every term, the scale of the errors."""
    if mag:
        x, wt, bt, w3, b2, w1, b3 = (t.abs() for t in (x, wt, bt, w3, b2, w1, b3))
    y = F.conv2d(F.conv_transpose2d(x, wt, bt, stride=2), w3, b2, padding=1)
    return F.conv2d(y if mag else torch.relu(y), w1, b3)[:, 0] if mag else torch.relu(F.conv2d(torch.relu(y), w1, b3))[:, 0]


def ternary(shape, g, density=0.25):
    r = torch.rand(shape, generator=g)
    return (r < density / 2).float() - (r > 1 - density / 2).float()


def integer_case(C, B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    ops = dict(wt=ternary((C, C, 2, 2), g), bt=ternary((C,), g), w3=ternary((32, C, 3, 3), g), b2=ternary((32,), g), w1=ternary((1, 32, 1, 1), g), b3=torch.ones(1))
    return torch.randint(-2, 3, (B, C, h, w), generator=g).float(), ops


def run(R, mode, x, ops):
    from visiondepth3d_amd import depth_pro
    from visiondepth3d_amd.depth import neck_poly_compose
    img = R.depthpro_head_pack(neck_poly_compose(ops["wt"], None, ops["w3"], 2)[0], mode)
    assert img is not None
    T = depth_pro.head_poly_table(ops["bt"], ops["w3"], ops["b2"]).cuda()
    return R.depthpro_head(x.cuda().contiguous(memory_format=CL), img, T, ops["w1"].reshape(-1).cuda().contiguous(), float(ops["b3"]), mode)


@pytest.mark.parametrize("h,w", [(9, 33), (1, 1)])
@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("mode", MODES)
def test_integer_operands_equal_the_float64_chain(R, mode, C, h, w):
    x, ops = integer_case(C, 3, h, w, 100 + C + h)
    d = {k: v.double() for k, v in ops.items()}
    assert float(chain(x.double(), mag=True, **d).max()) < 2 ** 24          # every partial sum is an integer float32 holds: exact in any order
    ref = chain(x.double(), **d)
    mid = F.conv2d(F.conv_transpose2d(x.double(), d["wt"], d["bt"], stride=2), d["w3"], d["b2"], padding=1)
    if h > 1:
        assert 0.2 < float((mid < 0).double().mean()) < 0.8 and float((ref == 0).double().mean()) > 0.01 and float(ref.max()) > 8   # both ReLUs engage
    y = run(R, mode, x, ops)
    assert tuple(y.shape) == (3, 2 * h, 2 * w) and y.dtype == torch.float32
    assert torch.equal(y.cpu().double(), ref)


def random_case(C, B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    ops = dict(wt=torch.randn(C, C, 2, 2, generator=g) / C ** 0.5, bt=torch.randn(C, generator=g), w3=torch.randn(32, C, 3, 3, generator=g) / (3.0 * C ** 0.5),
               b2=torch.randn(32, generator=g), w1=torch.randn(1, 32, 1, 1, generator=g) / 32 ** 0.5)
    x = torch.randn(B, C, h, w, generator=g)
    # the last bias centres the 1 x 1 convolution's output, so that the final ReLU cuts about half of the pixels whatever sign the drawn weights sum to
    d = F.conv2d(torch.relu(F.conv2d(F.conv_transpose2d(x, ops["wt"], ops["bt"], stride=2), ops["w3"], ops["b2"], padding=1)), ops["w1"])
    ops["b3"] = -d.median().reshape(1)
    return x, ops


@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("mode", MODES)
def test_random_operands_against_the_float64_chain(R, mode, C):
    B, h, w = 3, 9, 33
    x, ops = random_case(C, B, h, w, 7 + C)
    d = {k: v.double() for k, v in ops.items()}
    ref, scale = chain(x.double(), **d), chain(x.double(), mag=True, **d)
    y32 = chain(x, **ops).double()
    y = run(R, mode, x, ops)
    assert bool(torch.isfinite(y).all()) and 0.05 < float((ref == 0).double().mean()) < 0.95
    yd = y.cpu().double()

    def err(v):
        return float(((v - ref).abs() / scale).max()), float((v - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    (e, r), (e32, r32) = err(yd), err(y32)
    print("DEPTHPRO_HEAD_ERR", dict(mode=mode, C=C, max=e, max_yardstick=e32, max_ratio=e / max(e32, 1e-30), rms=r, rms_yardstick=r32, rms_ratio=r / max(r32, 1e-30)))
    assert e <= max(2.5 * e32, 2.0 ** -21), (e, e32)
    assert r <= 1.5 * r32, (r, r32)
    # same bits from call to call, and frame 0 alone against frame 0 of three
    assert torch.equal(run(R, mode, x, ops), y)
    assert torch.equal(run(R, mode, x[:1], ops), y[:1])


@pytest.mark.parametrize("mode", MODES)
def test_the_statement_is_what_the_kernel_computes(R, mode):
    """depth_pro.head_poly_statement on the kernel's float32 operands against the kernel: the difference is the kernel's arithmetic alone (split operands,
    float32 accumulation) -- inside the same bars against the statement's float64 value."""
    from visiondepth3d_amd import depth_pro
    x, ops = random_case(32, 2, 9, 33, 3)
    st = depth_pro.head_poly_statement(x, ops["wt"], ops["bt"], ops["w3"], ops["b2"], ops["w1"], float(ops["b3"]), operands=torch.float32)
    d = {k: v.double() for k, v in ops.items()}
    scale = chain(x.double(), mag=True, **d)
    e = float(((run(R, mode, x, ops).cpu().double() - st).abs() / scale).max())
    e32 = float(((chain(x, **ops).double() - chain(x.double(), **d)).abs() / scale).max())
    assert e <= max(2.5 * e32, 2.0 ** -21), (e, e32)


@pytest.mark.parametrize("mode", MODES)
def test_refusals_launch_nothing(R, mode):
    x, ops = integer_case(32, 1, 4, 5, 1)
    L, vp, m = R._L, ctypes.c_void_p, R.X3_MODES[mode]
    assert L.vd3d_depthpro_head_weight_bytes(m, 24) < 0 and L.vd3d_depthpro_head_weight_bytes(m, 0) < 0 and L.vd3d_depthpro_head_weight_bytes(2, 32) < 0
    assert L.vd3d_depthpro_head_weight_bytes(m, 32) == 16 * 2 * (3072 if mode == "bf16x3" else 2048) + (0 if mode == "bf16x3" else 128) + 64
    assert R.depthpro_head_pack(torch.zeros(16, 32, 24), mode) is None and R.depthpro_head_pack(torch.zeros(16, 64, 32), mode) is None
    from visiondepth3d_amd import depth_pro
    from visiondepth3d_amd.depth import neck_poly_compose
    img = R.depthpro_head_pack(neck_poly_compose(ops["wt"], None, ops["w3"], 2)[0], mode)
    T = depth_pro.head_poly_table(ops["bt"], ops["w3"], ops["b2"]).cuda()
    w1 = ops["w1"].reshape(-1).cuda().contiguous()
    xb = torch.zeros(1 * 4 * 5 * 32 + 4, device="cuda")
    xc = xb[:640].view(1, 4, 5, 32)
    xc.copy_(x.permute(0, 2, 3, 1))
    out = torch.full((1, 8, 10), -3.0, device="cuda")
    R._enter(xb, img, out)

    def call(X=xc.data_ptr(), cin=32, B=1, h=4, w=5, mode_=m, O=out.data_ptr()):
        return L.vd3d_depthpro_head(R._ctx, mode_, vp(X), B, h, w, cin, vp(img.data_ptr()), vp(T.data_ptr()), vp(w1.data_ptr()), 1.0, vp(O))
    assert call(cin=24) == -4 and b"C_in 24" in L.vd3d_last_error()
    assert call(cin=0) == -4 and b"C_in 0" in L.vd3d_last_error()
    assert call(B=0) == -4 and b"batch" in L.vd3d_last_error()
    assert call(h=0) == -4 and b"coarse map" in L.vd3d_last_error()
    assert call(X=xb.data_ptr() + 4) == -4 and b"aligned" in L.vd3d_last_error()
    assert call(O=xc.data_ptr()) == -4 and b"overlaps" in L.vd3d_last_error()
    assert call(mode_=2) != 0 and b"mode" in L.vd3d_last_error()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
    assert call() == 0
    d = {k: v.double() for k, v in ops.items()}
    assert torch.equal(out.cpu().double(), chain(x.double(), **d))
