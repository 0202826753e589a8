"""GPU tests (-m gpu) of DepthPro's two encoder-side kernels (csrc/vd3d_depthpro_pyramid.hip) against their NumPy statements in visiondepth3d_amd/depth_pro.py
(patches_statement, merge_statement, themselves held to transformers' own functions in tests/test_depth_pro_host.py): np.array_equal, nothing less.  Input values
carry their own index (distinct small integers, exact in float32 through every sum and the 0.25 of the pyramid), so a wrong order cannot pass; the merge's resize
cases add a non-dyadic fraction so that every rounding of the blend is exercised."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from visiondepth3d_amd import depth_pro   # noqa: E402


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _indexed(shape, fraction=False, bits=22):
    """float32 values that carry their own flat index (modulo 2^bits).  Without ``fraction`` they are integers: below 2^22 every sum of four and its quarter is
    exact, so the pyramid's levels are distinct per position; a plain copy takes 2^24.  With it a per-element non-dyadic fraction is added: blends then round at
    every operation."""
    n = int(np.prod(shape))
    v = (np.arange(n, dtype=np.int64) % (1 << bits)).astype(np.float32)
    if fraction:
        v = (v + np.float32(1) / (np.arange(n, dtype=np.float32) % 7 + np.float32(3))).astype(np.float32)
    return v.reshape(shape)


@pytest.mark.parametrize("S,p,B", [(256, 64, 1), (256, 64, 3), (1536, 384, 1), (80, 20, 2)])
def test_patches_kernel_equals_the_statement(R, S, p, B):
    """(256, 64): MINI, strides 48 / 32; (1536, 384): the published geometry; (80, 20): strides 15 / 10, no 16-byte alignment -- the 4-byte form runs."""
    x = _indexed((B, 3, S, S))
    lv = depth_pro.pyramid_levels(S, p)
    exp = depth_pro.patches_statement(x, p)
    got = R.depthpro_patches(torch.from_numpy(x).cuda(), p, [lv[2][2], lv[1][2], lv[0][2]])
    assert tuple(got.shape) == exp.shape == ((lv[0][3] ** 2 + lv[1][3] ** 2 + lv[2][3] ** 2) * B, 3, p, p)
    assert got.permute(0, 2, 3, 1).is_contiguous()   # the memory Renderer.patchify takes: no copy between the two
    assert np.array_equal(got.cpu().numpy(), exp)
    rows = R.patchify(got, 4).cpu().numpy()           # and patchify does take it: the rows of 4 x 4 patches, F.unfold's column order
    g = p // 4
    ref = exp.reshape(-1, 3, g, 4, g, 4).transpose(0, 2, 4, 1, 3, 5).reshape(exp.shape[0], g * g, 48)
    assert np.array_equal(rows, ref)


MERGE_CASES = [(1, 0, 4), (9, 6, 4), (25, 3, 4), (35, 3, 4), (9, 6, 24), (25, 3, 24), (4, 3, 4), (3, 3, 4)]
_EXPECTED_GEOMETRY = {(1, 0, 4): (1, 0, 4), (9, 6, 4): (3, 1, 8), (25, 3, 4): (5, 1, 12), (35, 3, 4): (5, 1, 12), (9, 6, 24): (3, 6, 48), (25, 3, 24): (5, 3, 96),
                      (4, 3, 4): (2, 1, 6), (3, 3, 4): (1, 0, 4)}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("C", [8, 384, 1024])
@pytest.mark.parametrize("n,padding,g", MERGE_CASES)
def test_merge_kernel_equals_the_statement(R, n, padding, g, C, extra, B):
    """Each (n, padding, g) at out = M (the identity: exact copies) and at out in {M + M // 3, 2 M - 3}.
    (25, 3, 4): the pad clamp engages (min(4 // 4, 3) = 1); (35, 3, 4): ten sequences are never read; (3, 3, 4): pad forced to 0; C = 8: below a wave's vector
    width; T = g^2 + 1: the class token is dropped."""
    side, pad, M = depth_pro.merge_geometry(n, g, padding)
    assert (side, pad, M) == _EXPECTED_GEOMETRY[(n, padding, g)]
    T = g * g + extra
    ident = _indexed((n * B, T, C), bits=24)
    frac = _indexed((n * B, T, C), fraction=True)
    dev_i, dev_f = torch.from_numpy(ident).cuda(), torch.from_numpy(frac).cuda()
    got = R.depthpro_merge(dev_i, B, g, padding, M, M)
    assert tuple(got.shape) == (B, M, M, C) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), depth_pro.merge_statement(ident, B, g, padding, M, M))
    for o in (M + M // 3, 2 * M - 3):
        got = R.depthpro_merge(dev_f, B, g, padding, o, o).cpu().numpy()
        assert np.array_equal(got, depth_pro.merge_statement(frac, B, g, padding, o, o)), o


def test_merge_kernel_takes_a_different_size_per_axis(R):
    """A non-square output, and one whose height alone is the merged size (that axis then takes the identity taps, weights 1 and 0, still multiplied in)."""
    frac = _indexed((9 * 2, 17, 12), fraction=True)
    dev = torch.from_numpy(frac).cuda()
    for oh, ow in ((13, 17), (10, 17), (17, 10)):
        assert np.array_equal(R.depthpro_merge(dev, 2, 4, 6, oh, ow).cpu().numpy(), depth_pro.merge_statement(frac, 2, 4, 6, oh, ow)), (oh, ow)


def test_refusals_launch_nothing(R):
    x = torch.zeros((1, 3, 64, 64), device="cuda")
    with pytest.raises(ValueError, match="depthpro_patches"):
        R.depthpro_patches(x, 32, [32, 16, 8])            # a quarter of 64 holds no 32 x 32 patch
    with pytest.raises(ValueError, match="depthpro_patches"):
        R.depthpro_patches(x[:, :, :62, :62].contiguous(), 8, [8, 4, 6])   # the side is no multiple of 4
    rows = torch.zeros((4, 15, 8), device="cuda")
    with pytest.raises(RuntimeError, match="depthpro_merge"):
        R.depthpro_merge(rows, 1, 4, 1, 6, 6)             # fewer tokens than the grid
