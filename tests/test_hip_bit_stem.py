"""GPU tests (-m gpu) of the three kernels of csrc/vd3d_bit.hip alone -- vd3d_im2col_nhwc_f32, vd3d_maxpool3x3_s2_nhwc_f32, vd3d_groupnorm_nhwc_f32 -- at the
smallest shapes at which they can still go wrong: 1 x 1 and 2 x 2 maps, odd sides, sides that are no multiple of anything, more than one workgroup, every
padding the BiT prefix uses and the symmetric ones beside them, the scalar (3-channel) and the vector form, one frame and three.

GroupNorm's summation order is stated here in NumPy (``gn_statement``; csrc/vd3d_bit.hip's header comment states the same six steps) and the kernel is held to it
bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F   # noqa: E402

MAPS = ((1, 1), (2, 2), (9, 11), (10, 12), (33, 7))


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _rand(shape, seed):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- im2col
def im2col_statement(x, k, s, pad):
    """x NHWC [B, H, W, C] -> [B, Ho, Wo, Kp]: pad, unfold, permute to (ky, kx, c), zero tail.  On the CPU."""
    pt, pb, pl, pr = pad
    B, H, W, C = x.shape
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    Ho, Wo = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
    cols = F.unfold(xp, k, stride=s).view(B, C, k, k, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(B, Ho, Wo, k * k * C)
    return F.pad(cols, (0, (k * k * C + 15) // 16 * 16 - k * k * C))


@pytest.mark.parametrize("k,s,lo,hi", [(7, 2, 2, 3), (7, 2, 3, 3), (3, 2, 0, 1), (3, 2, 1, 1), (1, 2, 0, 0), (3, 1, 1, 1)])
def test_im2col_is_the_torch_statement_bit_for_bit(R, k, s, lo, hi):
    ran = 0
    for H, W in MAPS:
        for C in (3, 16, 64):
            for B in (1, 3):
                x = _rand((B, H, W, C), 1000 * k + 100 * H + C + B)
                pad = (lo, hi, lo, hi)
                if H + lo + hi < k or W + lo + hi < k:   # no window fits: refused, nothing launched
                    with pytest.raises(ValueError, match="holds no"):
                        R.im2col(x.cuda(), k, s, pad)
                    continue
                exp = im2col_statement(x, k, s, pad)
                out = torch.full(tuple(exp.shape), float("nan"), device="cuda")      # an element the kernel does not write stays NaN
                got = R.im2col(x.cuda(), k, s, pad, out=out)
                assert got is out and torch.equal(got.cpu(), exp), (H, W, C, B)
                kk = k * k * C
                assert bool((got[..., kk:] == 0).all()) and got.shape[-1] % 16 == 0 and got.shape[-1] - kk < 16
                ran += 1
    assert ran >= 18
    # asymmetric per axis: top / bottom and left / right are read apart
    x = _rand((2, 9, 11, 16), 77)
    for pad in ((2, 0, 0, 1), (0, 2, 1, 0)):
        assert torch.equal(R.im2col(x.cuda(), 3, 2, pad).cpu(), im2col_statement(x, 3, 2, pad)), pad


def test_im2col_refusals(R):
    from visiondepth3d_amd._lib import Vd3dError
    x = _rand((1, 8, 8, 16), 1).cuda()
    for k, s, pad in ((5, 1, (0, 0, 0, 0)), (3, 3, (0, 0, 0, 0)), (3, 1, (3, 0, 0, 0)), (1, 2, (0, 1, 0, 0))):
        with pytest.raises(Vd3dError, match="im2col: not built"):
            R.im2col(x, k, s, pad)
    flat = torch.zeros(8 * 8 * 16 + 1, device="cuda")
    with pytest.raises(Vd3dError, match="aligned"):
        R.im2col(flat[1:].view(1, 8, 8, 16), 3, 1, (1, 1, 1, 1))              # C % 4 == 0: 16-byte loads
    ok = torch.zeros(8 * 8 * 3 + 1, device="cuda")[1:].view(1, 8, 8, 3)
    assert R.im2col(ok, 3, 1, (1, 1, 1, 1)).shape == (1, 8, 8, 32)            # the scalar form reads 4-byte aligned floats


# ---------------------------------------------------------------------------------------------------------------- max-pool
def _same_bits(a, b):
    return bool(torch.equal(torch.isnan(a), torch.isnan(b))) and bool(torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))


@pytest.mark.parametrize("lo,hi", [(0, 1), (1, 1), (0, 0)])
def test_maxpool_is_torchs_on_the_padded_map(R, lo, hi):
    ran = 0
    for H, W in MAPS:
        for C in (4, 64):
            for B in (1, 3):
                x = _rand((B, H, W, C), 10 * H + C + B) - 1.0        # mostly negative: the pad value 0 wins many windows
                pad = (lo, hi, lo, hi)
                if H + lo + hi < 3 or W + lo + hi < 3:
                    with pytest.raises(ValueError, match="holds no"):
                        R.maxpool3x3_s2(x.cuda(), pad)
                    continue
                for pv in (0.0, -3.5):
                    exp = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (lo, hi, lo, hi), value=pv), 3, 2).permute(0, 2, 3, 1)
                    got = R.maxpool3x3_s2(x.cuda(), pad, pv)
                    assert got.is_contiguous() and torch.equal(got.cpu(), exp), (H, W, C, B, pv)
                ran += 1
    assert ran >= 12


def test_maxpool_nan_stays_in_its_own_windows(R):
    x = _rand((2, 10, 12, 8), 5)
    x[1, 4, 5, 3] = float("nan")      # row 4 / column 5 with padding 0 / 1: windows (1..2, 2) -- two outputs of channel 3 in frame 1
    exp = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1), value=0.0), 3, 2).permute(0, 2, 3, 1)
    got = R.maxpool3x3_s2(x.cuda(), (0, 1, 0, 1), 0.0).cpu()
    assert int(torch.isnan(exp).sum()) == 2 and _same_bits(got, exp)


def test_maxpool_refusals(R):
    from visiondepth3d_amd._lib import Vd3dError
    with pytest.raises(Vd3dError, match="maxpool3x3_s2: not built"):
        R.maxpool3x3_s2(torch.zeros(1, 8, 8, 6, device="cuda"), (0, 1, 0, 1))
    with pytest.raises(Vd3dError, match="maxpool3x3_s2: not built"):
        R.maxpool3x3_s2(torch.zeros(1, 8, 8, 8, device="cuda"), (3, 0, 0, 0))
    with pytest.raises(Vd3dError, match="maxpool3x3_s2: not built"):
        R.maxpool3x3_s2(torch.zeros(8 * 8 * 8 + 1, device="cuda")[1:].view(1, 8, 8, 8), (0, 1, 0, 1))


# ---------------------------------------------------------------------------------------------------------------- GroupNorm
def _pair(v):
    """Pairwise tree of neighbours over axis 0 (a power of two long): v[0] + v[1], v[2] + v[3], ... until one is left."""
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def _group_total(vals, G):
    """Steps 1 - 5 of the kernel's order for one frame: vals float32 [P, C] (the values, or the centred squares) -> float32 [G]."""
    P, C = vals.shape
    cpg, rows = C // G, 1024 // C
    ch = max(16, (-(-P // 64) + 15) // 16 * 16)                 # 1. chunks of ch pixels, at most 64
    nch = -(-P // ch)
    v = np.zeros((nch * ch, C), np.float32)
    v[:P] = vals                                                  #    (pixels behind the last one add zeros)
    v = v.reshape(nch, ch // rows, rows, C)
    acc = np.zeros((nch, rows, C), np.float32)
    for i in range(ch // rows):                                   # 2. row r: pixels r, r + R, r + 2R, ... one after the other
        acc = acc + v[:, i]
    g = _pair(np.moveaxis(acc.reshape(nch, rows, G, cpg), 3, 0))  # 3. the channels of a group                      -> [nch, rows, G]
    r16 = np.zeros((16, nch, G), np.float32)
    r16[:rows] = np.moveaxis(g, 1, 0)
    part = _pair(r16)                                             # 4. the rows, padded with zeros to 16             -> [nch, G]
    c64 = np.zeros((64, G), np.float32)
    c64[:nch] = part
    return _pair(c64)                                             # 5. the chunks, padded with zeros to 64           -> [G]


def gn_statement(x, G, gamma, beta, eps, res=None, relu=False):
    """vd3d_groupnorm_nhwc_f32 in NumPy, operation for operation in float32: x [B, P, C]."""
    x = np.asarray(x, np.float32)
    B, P, C = x.shape
    cpg = C // G
    n = np.float32(P * cpg)
    out = np.empty_like(x)
    for b in range(B):
        mean = np.repeat(_group_total(x[b], G) / n, cpg)                                   # 6. mean first ...
        d = x[b] - mean
        sq = _group_total(d * d, G)                                                        #    ... then the centred sum of squares
        rstd = 1.0 / np.sqrt(sq.astype(np.float64) / np.float64(n) + np.float64(np.float32(eps)))   # float64 from the float32 sum ...
        scale = (np.repeat(rstd, cpg) * gamma.astype(np.float64)).astype(np.float32)        #    ... one rounding to float32 per channel
        y = (x[b] - mean) * scale + beta
        if res is not None:
            y = y + res[b]
        out[b] = np.where(y < 0, np.float32(0), y) if relu else y
    assert out.dtype == np.float32
    return out


_GN_EPILOGUES = (("relu", False, True), ("plain", False, False), ("residual+relu", True, True))
GN_ERRORS = []


@pytest.mark.parametrize("C", [64, 256, 1024])
@pytest.mark.parametrize("P", [1, 7, 576, 9216])
def test_groupnorm_is_its_numpy_statement_repeats_and_does_not_depend_on_the_batch(R, C, P):
    """Per shape, all three epilogues, one frame and three: bit-identical to gn_statement; frame 0 alone == frame 0 of the batch of three; two runs equal; and
    against float64 the maximum error is at most 2 x that of torch.nn.functional.group_norm in float32 on the CPU (+ residual, ReLU in float32) on the same input."""
    G, eps = 32, 1e-5
    H, W = {1: (1, 1), 7: (7, 1), 576: (24, 24), 9216: (96, 96)}[P]
    x = _rand((3, H, W, C), C + P) * 2.0 + 0.5
    res = _rand((3, H, W, C), C + P + 1)
    gamma, beta = 1.0 + 0.5 * _rand((C,), 3), 0.5 * _rand((C,), 4)
    xg, rg, gg, bg = x.cuda(), res.cuda(), gamma.cuda(), beta.cuda()
    # once per shape, shared by the epilogues and both batch sizes (group_norm works per frame: frame 0 of three is frame 0 alone)
    gn64 = F.group_norm(x.double().permute(0, 3, 1, 2), G, gamma.double(), beta.double(), eps).permute(0, 2, 3, 1)
    gn32 = F.group_norm(x.permute(0, 3, 1, 2), G, gamma, beta, eps).permute(0, 2, 3, 1)
    xn, rn = x.reshape(3, P, C).numpy(), res.reshape(3, P, C).numpy()
    for what, with_res, relu in _GN_EPILOGUES:
        got3 = R.groupnorm(xg, G, gg, bg, eps, residual=rg if with_res else None, relu=relu)
        got1 = R.groupnorm(xg[:1].contiguous(), G, gg, bg, eps, residual=rg[:1].contiguous() if with_res else None, relu=relu)
        again = R.groupnorm(xg, G, gg, bg, eps, residual=rg if with_res else None, relu=relu)
        assert torch.equal(got3, again), what
        assert torch.equal(got1[0], got3[0]), what
        got = got3.cpu()
        exp = gn_statement(xn, G, gamma.numpy(), beta.numpy(), eps, rn if with_res else None, relu)
        assert np.array_equal(got.numpy().reshape(3, P, C), exp), (what, float(np.abs(got.numpy().reshape(3, P, C) - exp).max()))

        def fin(y, r):
            y = y + r if with_res else y
            return torch.relu(y) if relu else y
        truth, yard = fin(gn64, res.double()), fin(gn32, res)
        for B in (1, 3):
            e_k = float((got[:B].double() - truth[:B]).abs().max())
            e_t = float((yard[:B].double() - truth[:B]).abs().max())
            GN_ERRORS.append((C, P, B, what, e_k, e_t))
            print("GN_F64", dict(C=C, P=P, B=B, epilogue=what, err_kernel=e_k, err_torch_cpu=e_t, ratio=e_k / e_t if e_t else float("inf")))
            assert e_k <= 2.0 * e_t, (C, P, B, what, e_k, e_t)


def test_groupnorm_in_place_and_large_common_offset(R):
    """Values 1000 +- 1: the variance is 1 / 3 on a mean of 1000.  A float32 E[x^2] - mean^2 subtracts two numbers near 10^6, whose float32 spacing is 0.0625 -- a
    fifth of the variance; the centred second pass squares values of magnitude 1.  The mean itself carries at most a few float32 spacings of 1000 (6.1e-5 each),
    which moves every normalised value by about that times rstd (1.7): the result is held to 1e-3 of the float64 one, fifty times below what the one-pass formula
    would show.  Also: out = x (in place) gives the same bits."""
    C, G, eps = 256, 32, 1e-5
    x = (torch.from_numpy(np.random.Generator(np.random.PCG64(9)).uniform(-1, 1, (2, 24, 24, C)).astype(np.float32)) + 1000.0)
    gamma, beta = torch.ones(C), torch.zeros(C)
    got = R.groupnorm(x.cuda(), G, gamma.cuda(), beta.cuda(), eps)
    truth = F.group_norm(x.double().permute(0, 3, 1, 2), G, gamma.double(), beta.double(), eps).permute(0, 2, 3, 1)
    err = float((got.cpu().double() - truth).abs().max())
    print("GN_OFFSET_1000", err)
    assert err <= 1e-3, err
    assert np.array_equal(got.cpu().numpy().reshape(2, 576, C), gn_statement(x.reshape(2, 576, C).numpy(), G, gamma.numpy(), beta.numpy(), eps))
    xi = x.cuda()
    assert R.groupnorm(xi, G, gamma.cuda(), beta.cuda(), eps, out=xi) is xi and torch.equal(xi, got)


def test_groupnorm_refusals(R):
    from visiondepth3d_amd._lib import Vd3dError
    ones = lambda c: torch.ones(c, device="cuda")   # noqa: E731
    for C, G in ((96, 32), (64, 64), (2048, 32), (128, 2), (80, 20)):     # C % G; one channel per group; C not built; 64 per group; C not built
        with pytest.raises(NotImplementedError, match="not built"):
            R.groupnorm(torch.zeros(1, 4, 4, C, device="cuda"), G, ones(C), ones(C), 1e-5)
    x = torch.zeros(4 * 4 * 64 + 1, device="cuda")[1:].view(1, 4, 4, 64)
    with pytest.raises(Vd3dError, match="16-byte aligned"):
        R.groupnorm(x, 32, ones(64), ones(64), 1e-5)
    with pytest.raises(Vd3dError, match="16-byte aligned"):
        R.groupnorm(torch.zeros(1, 4, 4, 64, device="cuda"), 32, torch.ones(65, device="cuda")[1:], ones(64), 1e-5)
    with pytest.raises(ValueError, match="residual"):
        R.groupnorm(torch.zeros(1, 4, 4, 64, device="cuda"), 32, ones(64), ones(64), 1e-5, residual=torch.zeros(1, 4, 4, 128, device="cuda"))
