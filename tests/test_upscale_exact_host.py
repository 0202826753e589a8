"""CPU checks of tests/upscale_exact.py, the helper behind the bit-exact GPU tests of the fp16 up-scale convolutions: the float64 reference against ATen's
float64 convolution, the exactness preconditions of every data set, the numpy epilogues against the module graph's own float32 evaluation, and the restated
launch policy of vd3d_conv3x3_c64_f16."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upscale_exact as UE  # noqa: E402


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (9, 33)])
@pytest.mark.parametrize("cin,cout,up2", [(64, 64, False), (192, 64, False), (64, 64, True), (192, 32, False)])
def test_ref_acc64_equals_aten_float64_convolution(H, W, cin, cout, up2):
    import torch.nn.functional as F
    x, w = UE.int_data(H, W, cin, cout, seed=H * 100 + W + cin)
    got = UE.ref_acc64(x, w, up2=up2)
    src = UE.nchw(x).double()
    if up2:
        src = F.interpolate(src, scale_factor=2, mode="nearest")
    ref = F.conv2d(src, w.double(), padding=1)
    assert tuple(got.shape) == ((2 * H, 2 * W, cout) if up2 else (H, W, cout))
    assert torch.equal(got, UE.hwc(ref))
    assert float(got.abs().max()) > 0 or H * W == 1
    # and the float32 convolution agrees as well: the data is exact there in any order
    assert torch.equal(got, UE.hwc(F.conv2d(src.float(), w.float(), padding=1)).double())


@pytest.mark.parametrize("scale", sorted(UE.SCALES))
@pytest.mark.parametrize("cin,x_range", UE.DATASETS)
def test_exactness_preconditions_of_every_data_set(cin, x_range, scale):
    ex, ew = UE.SCALES[scale]
    assert UE.acc_bound(cin, x_range) < 2 ** 24                 # every partial sum is an integer float32 holds, times one power of two
    assert -126 <= ex + ew and ex + ew + 24 <= 127              # ... inside float32's normal exponent range
    x, w = UE.int_data(9, 33, cin, 64, seed=cin, x_range=x_range, scale=scale)
    gen = torch.Generator().manual_seed(cin)                    # the same integers, scaled in float64: .half() lost nothing
    xi = torch.randint(x_range[0], x_range[1] + 1, (9, 33, cin), generator=gen, dtype=torch.int8)
    wi = torch.randint(UE.W_RANGE[0], UE.W_RANGE[1] + 1, (64, cin, 3, 3), generator=gen, dtype=torch.int8)
    assert torch.equal(x.double(), xi.double() * 2.0 ** ex) and torch.equal(w.double(), wi.double() * 2.0 ** ew)
    assert int(xi.min()) == x_range[0] and int(xi.max()) == x_range[1] and int(wi.min()) == -2 and int(wi.max()) == 2
    acc = UE.ref_acc64(x, w)
    n = acc * 2.0 ** -(ex + ew)
    assert torch.equal(n, n.round()) and float(n.abs().max()) <= UE.acc_bound(cin, x_range)
    if cin < 64:
        return
    out = UE.expect_c64(acc[..., :64], np.zeros(64, np.float32)).astype(np.float64)
    nz = out != 0
    if scale.startswith("subnormal"):                           # every non-zero output is an fp16 subnormal and exactly the accumulator
        assert np.array_equal(out, acc.numpy()) and float(np.abs(out[nz]).max()) < 2.0 ** -14 and nz.mean() > 0.9
    if scale == "overflow":                                     # a good part overflows, the rest is exact
        inf = np.isinf(out)
        assert 0.2 < inf.mean() < 0.9 and np.array_equal(out[~inf], acc.numpy()[~inf]) and np.all(np.abs(acc.numpy()[inf]) >= 65520)


@pytest.mark.parametrize("cin,cout", [(192, 64), (64, 32)])
def test_expect_dense_equals_the_module_graphs_float32_evaluation(cin, cout):
    """RRDBNet's `x5 * 0.2 + x` and `out * 0.2 + x` (upscale.ResidualDenseBlock / RRDB) evaluated by torch in float32 on the CPU, rounded to fp16 once."""
    import torch.nn.functional as F
    H, W = 9, 33
    x, w = UE.int_data(H, W, cin, cout, seed=7)
    gen = torch.Generator().manual_seed(8)
    b = torch.randn(cout, generator=gen) * 0.37
    r1 = (torch.randn(1, cout, H, W, generator=gen) * 0.7).half()
    r2 = (torch.randn(1, cout, H, W, generator=gen) * 0.7).half()
    conv = F.conv2d(UE.nchw(x).float(), w.float(), padding=1) + b[None, :, None, None]
    acc = UE.ref_acc64(x, w)
    np1, np2 = UE.hwc(r1).numpy(), UE.hwc(r2).numpy()
    none = F.leaky_relu(conv, 0.2)
    one = F.leaky_relu(conv, 0.2) * 0.2 + r1.float()
    two = one * 0.2 + r2.float()
    assert np.array_equal(UE.bits(UE.hwc(none.half())), UE.expect_dense(acc, b.numpy(), 0.2).view(np.int16))
    assert np.array_equal(UE.bits(UE.hwc(one.half())), UE.expect_dense(acc, b.numpy(), 0.2, np1, 0.2).view(np.int16))
    assert np.array_equal(UE.bits(UE.hwc(two.half())), UE.expect_dense(acc, b.numpy(), 0.2, np1, 0.2, np2, 0.2).view(np.int16))
    # the c64 / head epilogue with a per-channel slope against torch's float32 PReLU
    sl = torch.rand(cout, generator=gen) * 0.5
    pre = F.prelu(conv, sl)
    if cout == 64:
        assert np.array_equal(UE.bits(UE.hwc(pre.half())), UE.expect_c64(acc, b.numpy(), sl.numpy()).view(np.int16))


def test_what_the_fp16_output_can_tell_about_the_order_of_slope_and_alpha():
    """With the network's slope == alpha == 0.2 the two orders are the same two multiplications, (v * 0.2) * 0.2, and cannot be told apart.  With slope 0.3
    they differ by one float32 ULP on a part of the negative values, and the fp16 rounding hides that except where it straddles an fp16 rounding boundary
    (about 2^-13 of them): over every negative accumulator value of a 64-channel layer x 64 biases a handful shows, over 9 x 33 pixels none need to.  That
    is why the GPU test runs an epilogue with slope 0.3 and has a 135 x 240 size."""
    gen = torch.Generator().manual_seed(8)
    b = (torch.randn(64, generator=gen) * 0.37).numpy()
    n = UE.acc_bound(64)
    acc = np.broadcast_to(-np.arange(1, n + 1, dtype=np.float64)[None, :, None], (1, n, 64))
    r1 = (torch.randn(1, n, 64, generator=gen) * 0.7).half().numpy()
    for slope, differs in ((0.2, False), (0.3, True)):
        v = (acc.astype(np.float32) + b) * np.float32(0.2)
        swapped = (np.where(v >= 0, v, v * np.float32(slope)) + r1.astype(np.float32)).astype(np.float16)
        same = swapped.view(np.int16) == UE.expect_dense(acc, b, slope, r1, 0.2).view(np.int16)
        assert bool(same.all()) != differs, (slope, int((~same).sum()))


def test_c64_regime_restates_the_launch_policy():
    assert UE.c64_slots(256) == 768 and UE.c64_slots(304) == 912 and UE.c64_slots(257) == 768
    assert UE.c64_regime(540, 960, 256) == ("persistent", 2040, 255, 3)
    assert UE.c64_regime(1080, 1920, 256) == ("tile16", 60 * 68, 0, 1)
    assert UE.c64_regime(1, 1, 256) == ("one-round", 1, 1, 1)
    assert UE.c64_regime(8 * 24, 32 * 32, 256) == ("one-round", 768, 96, 1)        # exactly the slots
    assert UE.c64_regime(8 * 24 + 1, 32 * 32, 256)[0] == "persistent"              # 800 tiles
    assert UE.c64_regime(8 * 70, 330, 256) == ("persistent", 770, 97, 2)           # 11 tile columns, W % 32 == 10
    assert UE.c64_regime(16384, 64, 256) == ("persistent", 4096, 512, 6)
    assert UE.c64_regime(16385, 64, 256) == ("tile16", 2 * 1025, 0, 1)
    for H, W in [(32769, 1), (16385, 33), (1, 131073), (17, 43713), (10929, 65), (10921, 65), (10927, 65)]:
        assert UE.c64_regime(H, W, 256)[0] == "tile16", (H, W)
    assert UE.c64_regime(10913, 65, 256) == ("persistent", 4095, 512, 6)              # one tile row less: still the 32 x 8 kernel
    assert UE.c64_regime(720, 1280, 256)[0] == "persistent" and UE.c64_regime(720, 1280, 256)[1] == 3600
