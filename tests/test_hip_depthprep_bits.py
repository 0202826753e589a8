"""GPU tests (-m gpu) of vd3d_depth_preprocess (csrc/vd3d_depthprep.hip: k_depth_prep, the 32 x 8 tile kernel, and k_depth_prep_strip, the strip kernel for
down-scaling), float32 and bf16, on BITS against the NumPy restatement of tests/test_depthprep_host.py (proved there against the float64 operator within a derived
bound, with mutants -- no antialias, a = -0.75, no half-pixel centre, weights not normalised, channels not swapped, xend one short -- that the shared cases catch).
The restatement has no clamp, the kernels clamp silently at four capacities: equal bits on these geometries, and the host sweep of the launcher's arithmetic over
every geometry, are what says the clamps never act.

Random bytes, B = 2, ImageNet mean / std (DPT's 0.5 / 0.5 on one case), forms 0 (the library's choice), 1 (tile) and 2 (strip) wherever form 2 applies:
  headline16   (1080, 320) -> (259, 77)   the headline's own two float32 scales (2160 / 518 = 1080 / 259, 3840 / 924 = 320 / 77) at a sixteenth of the bytes; bands of
                                          32 rows
  band_edge    (327, 64) -> (75, 16)      bands of 32 rows at the least slack of the host sweep: 153 of the 160 filtered rows a band can hold
  hd1080_16    (540, 160) -> (259, 77)    the 1080p scales
  scale5p7     (57, 114) -> (10, 20)      scale 5.7: 22 and 23 taps, the last admitted quarter-step of the tap budget; the strip's pad to 24 in use; bands of 16
  scale5_5p32  (120, 250) -> (24, 47)     scales 5.0 and 5.32; the output width is no multiple of 32
  scale1       (64, 64) -> (64, 64)
  up           (40, 60) -> (70, 126)      up-scaling: the tile kernel only, support 2; forms 0 and 1
  mixed        (108, 54) -> (20, 60)      one axis down, one up: the tile form is the one that runs
  tile_edge    (13, 46) -> (21, 67)       the tile kernel's input tile at the least slack of the host sweep, 3 rows and 3 columns
  small, tiny  (33, 65) -> (8, 16), (7, 9) -> (3, 4)   narrower than a strip or a tile
  tw33         (50, 100) -> (12, 33)      a last tile of one column
  phases       (97, 131) -> (28, 42) on frames[1:] of a stack of three: odd W * 3 and a base that is not 4-aligned, all four byte phases of the strip's dword fetch
and frame 0 of a batch of three against the same frame alone; the same frames inside a larger buffer of zeros and of 255s."""
import os
import sys

import numpy as np
import pytest

from visiondepth3d_amd import _abi, _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_depthprep_host as H  # noqa: E402

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
DOWN = ("headline16", "band_edge", "hd1080_16", "scale5p7", "scale5_5p32", "scale1", "small", "tiny", "tw33")     # both scales >= 1: form 2 applies


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    r = Renderer(0)
    yield r
    r.close()


def _bits(t):
    """The kernel's result [B, 3, th, tw] (channels_last) -> its NHWC storage as uint32 / uint16 bits."""
    t = t.permute(0, 2, 3, 1)
    assert t.is_contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint16)


def _want(name, dtype, mean, std, frames=slice(None)):
    w = H.statement_of_case(name, dtype, mean, std)[frames]
    return w.view(np.uint32) if dtype == "f32" else w


def _run(R, frames, th, tw, mean, std, dtype, form):
    got = R.depth_preprocess(frames, th, tw, mean, std, dtype=TDT[dtype], form=form)
    assert got.shape == (frames.shape[0], 3, th, tw) and got.dtype == TDT[dtype] and got.is_contiguous(memory_format=torch.channels_last)
    return _bits(got)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", DOWN)
def test_down_scaling_has_the_statements_bits_in_every_form(R, name, dtype):
    B, (Hh, W), (th, tw) = H.CASES[name]
    frames = torch.from_numpy(H.frames_u8(name)).cuda()
    norms = [(H.IMAGENET_MEAN, H.IMAGENET_STD)] + ([(H.DPT_MEAN, H.DPT_STD)] if name == "scale5_5p32" else [])
    for mean, std in norms:
        want = _want(name, dtype, mean, std)
        for form in (0, 1, 2):
            assert np.array_equal(_run(R, frames, th, tw, mean, std, dtype, form), want), (name, dtype, form, std)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["up", "mixed", "tile_edge"])
def test_up_scaling_and_mixed_run_the_tile_form(R, name, dtype):
    B, (Hh, W), (th, tw) = H.CASES[name]
    frames = torch.from_numpy(H.frames_u8(name)).cuda()
    want = _want(name, dtype, H.IMAGENET_MEAN, H.IMAGENET_STD)
    for form in (0, 1):
        assert np.array_equal(_run(R, frames, th, tw, H.IMAGENET_MEAN, H.IMAGENET_STD, dtype, form), want), (name, dtype, form)
    with pytest.raises(_lib.Vd3dError) as e:                                              # the strip form does not take an axis that scales up
        R.depth_preprocess(frames, th, tw, H.IMAGENET_MEAN, H.IMAGENET_STD, dtype=TDT[dtype], form=2)
    assert e.value.code == _abi.E_UNSUPPORTED and "strip form" in str(e.value)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_all_four_byte_phases_of_the_strips_dword_fetch(R, dtype):
    """frames[1:] of a stack of three (97, 131): rows of 393 bytes from a base that is 1 mod 4.  Every strip meets every phase."""
    name = "phases"
    B, (Hh, W), (th, tw) = H.CASES[name]
    stack = torch.from_numpy(H.frames_u8(name)).cuda()
    frames = stack[1:]
    assert frames.is_contiguous() and stack.data_ptr() % 4 == 0 and frames.data_ptr() % 4 == 1 and (W * 3) % 2 == 1
    _, _, _, _, xmin, _ = H.axis_windows(W, tw)
    for c_lo in xmin[::32]:                                                               # the first input column of each strip
        for b in range(2):
            phases = {(frames.data_ptr() + ((b * Hh + r) * W + int(c_lo)) * 3) % 4 for r in range(Hh)}
            assert phases == {0, 1, 2, 3}
    want = _want(name, dtype, H.IMAGENET_MEAN, H.IMAGENET_STD, slice(1, None))
    for form in (0, 1, 2):
        assert np.array_equal(_run(R, frames, th, tw, H.IMAGENET_MEAN, H.IMAGENET_STD, dtype, form), want), (dtype, form)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_frame_has_the_same_bits_alone_and_in_a_batch(R, dtype):
    name = "phases"
    B, (Hh, W), (th, tw) = H.CASES[name]
    stack = torch.from_numpy(H.frames_u8(name)).cuda()
    want = _want(name, dtype, H.IMAGENET_MEAN, H.IMAGENET_STD)
    for form in (0, 1, 2):
        three = _run(R, stack, th, tw, H.IMAGENET_MEAN, H.IMAGENET_STD, dtype, form)
        alone = _run(R, stack[:1].clone(), th, tw, H.IMAGENET_MEAN, H.IMAGENET_STD, dtype, form)
        assert np.array_equal(three, want) and np.array_equal(alone, want[:1]) and np.array_equal(three[:1], alone), (dtype, form)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,lead", [("small", 67), ("scale5p7", 64), ("tw33", 130)])
def test_what_surrounds_the_frames_does_not_reach_the_result(R, name, lead, dtype):
    """The same frames as a slice of a larger uint8 buffer, filled with 0 and with 255 around them.  The strip kernel fetches whole dwords around each row and
    multiplies the bytes behind padded taps by +0: neither may show."""
    B, (Hh, W), (th, tw) = H.CASES[name]
    src = torch.from_numpy(H.frames_u8(name)).cuda()
    want = _want(name, dtype, H.IMAGENET_MEAN, H.IMAGENET_STD)
    n = src.numel()
    for fill in (0, 255):
        buf = torch.full((lead + n + 256,), fill, dtype=torch.uint8, device="cuda")
        buf[lead:lead + n] = src.reshape(-1)
        frames = buf[lead:lead + n].view(B, Hh, W, 3)
        assert frames.is_contiguous() and frames.data_ptr() == buf.data_ptr() + lead and frames.data_ptr() % 4 == lead % 4
        for form in (0, 1, 2):
            assert np.array_equal(_run(R, frames, th, tw, H.IMAGENET_MEAN, H.IMAGENET_STD, dtype, form), want), (name, dtype, form, fill)
        assert bool((buf[:lead] == fill).all()) and bool((buf[lead + n:] == fill).all())
