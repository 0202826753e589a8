"""GPU tests (-m gpu) of the three float32 glue kernels of the interpolation network (csrc/vd3d_conv_ifn.hip) on BITS, at the padding, border and flow edges.

vd3d_rife_warp_pack, vd3d_rife_update and vd3d_rife_blend against the NumPy float32 restatements of tests/test_rife_glue_host.py (proved there against the
module's own operations in float64, with mutants that the shared inputs catch), bit for bit: frames 1 x 1, 32 x 64, 33 x 65 and 70 x 100 (no padding, one
padded row / column, a wide strip), batch 3, scales 1, 2, 4, flows of every planted kind (integers, quarter pixels, -2^-30, exactly on and one pixel around
every border, into the padded strip, +-1e30) and the exact family.  Every buffer holds one frame more than N: NaN behind the inputs (read = seen), a sentinel
behind the outputs (written = seen).  Two calls give equal bits, frame 0 alone equals frame 0 of the batch.  NaN / Inf flows read the border pixel and leave
the images finite; refused calls leave every byte as it was."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_rife_glue_host as H  # noqa: E402

SENT = -7.5
N = H.BATCH


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _plus_frame(a, fill):
    """The frames of `a` on the GPU in a buffer of one frame more, which holds `fill`."""
    buf = torch.full((a.shape[0] + 1,) + tuple(a.shape[1:]), fill, dtype=torch.float32, device="cuda")
    buf[:-1] = torch.from_numpy(np.ascontiguousarray(a))
    return buf


def _out(shape):
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), SENT, dtype=torch.float32, device="cuda")


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same_bits(got, want, nan_ok=None):
    """Equal bits; where nan_ok is set (flow channels that carry a non-finite flow through), a NaN matches a NaN of any payload."""
    g, w = got.detach().cpu().numpy(), np.ascontiguousarray(want, dtype=np.float32)
    same = g.view(np.uint32) == w.view(np.uint32)
    if nan_ok is not None:
        same |= nan_ok & np.isnan(g) & np.isnan(w)
    return bool(same.all())


def _pack(R, x6, state, s):
    """Run the pack on buffers of N + 1 frames: the batch twice, then frame 0 alone.  Returns the [N, Hp / s, Wp / s, 16] result."""
    h, w = x6.shape[2:]
    Hp, Wp = H.pad32(h), H.pad32(w)
    xb = _plus_frame(x6, float("nan"))
    sb = None if state is None else _plus_frame(state, float("nan"))
    outs = []
    for n in (N, N, 1):
        ob = _out((N, Hp // s, Wp // s, 16))
        R.rife_warp_pack(xb[:n], None if sb is None else sb[:n], s, ob[:n])
        assert bool((ob[n:] == SENT).all())                          # nothing behind frame n is written
        outs.append(ob)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert np.array_equal(_bits(outs[2][:1]), _bits(outs[0][:1]))
    assert bool((outs[0][:N, ..., 11:] == 0).all())
    return outs[0][:N]


@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("h,w", H.SIZES)
def test_warp_pack_equals_its_restatement_bit_for_bit(R, h, w, s):
    """General and exact family, with a state and without (the first block).  The float64 figures are printed beside the float32 CPU chain's."""
    for fam in (H.family(h, w), H.exact_family(h, w)):
        st = H.make_state(fam["flow"], fam["mask"])
        for state in (st, None):
            got = _pack(R, fam["x6"], state, s)
            assert _same_bits(got, H.warp_pack_restated(fam["x6"], state, s)), (h, w, s, state is None)
    g = H.family(h, w)
    got = H._nchw(_pack(R, g["x6"], H.make_state(g["flow"], g["mask"]), s).cpu().numpy())[:, :11]
    ref, yard = H.pack_module(g["x6"], g["flow"], g["mask"], s, torch.float64).numpy(), H.pack_module(g["x6"], g["flow"], g["mask"], s, torch.float32).numpy()
    sc = np.ones_like(ref)
    sc[:, 7:] = np.maximum(1.0, H._down_abs(g["flow"], s) / s)
    H.bars(f"GPU pack {h}x{w} s{s}", got, ref, yard, sc)
    assert float((np.abs(got.astype(np.float64) - ref) / H.pack_bound(g["flow"], g["mask"], s)).max()) <= 1.0


@pytest.mark.parametrize("pitch", [8, 32])
@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("h,w", H.SIZES)
def test_update_equals_its_restatement_bit_for_bit(R, h, w, s, pitch):
    """t of pitch 8 and 32 with 1e30 in the channels behind the five real ones (read = seen); the state's channels 5 .. 7 start at 9 and end 0."""
    for exact in (False, True):
        t, state = H.update_inputs(h, w, s, pitch, exact)
        assert bool((t[..., 5:] == np.float32(1e30)).all()) and bool((state[..., 5:] == 9.0).all())
        tb = _plus_frame(t, float("nan"))
        for first in (False, True):
            want = H.update_restated(t, state, s, first)
            outs = []
            before = _plus_frame(state, SENT)
            for n in (N, N, 1):
                sb = before.clone()
                R.rife_update(tb[:n], sb[:n], s, first, h, w)
                assert torch.equal(sb[n:], before[n:])                   # the frames behind n, the sentinel frame among them, keep their values
                outs.append(sb)
            assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[2][:1]), _bits(outs[0][:1]))
            assert bool((outs[0][:N, ..., 5:] == 0).all())
            assert _same_bits(outs[0][:N], want), (h, w, s, pitch, exact, first)
            if not exact and pitch == 8:
                ref = H.update_module(t, state, s, first, torch.float64).numpy()
                H.bars(f"GPU update {h}x{w} s{s} first{int(first)}", H._nchw(outs[0][:N].cpu().numpy())[:, :5], ref, H.update_module(t, state, s, first, torch.float32).numpy())


def _blend(R, x6, state):
    h, w = x6.shape[2:]
    xb, sb = _plus_frame(x6, float("nan")), _plus_frame(state, float("nan"))
    outs = []
    for n in (N, N, 1):
        ob = _out((N, 3, h, w))
        R.rife_blend(xb[:n], sb[:n], ob[:n])
        assert bool((ob[n:] == SENT).all())
        outs.append(ob)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[2][:1]), _bits(outs[0][:1]))
    return outs[0][:N]


@pytest.mark.parametrize("h,w", H.SIZES)
def test_blend_equals_its_restatement_on_exact_masks_and_holds_the_float64_bars_on_random_ones(R, h, w):
    """Masks from {0, +104, -104} make sigmoid exactly 0.5, 1, 0 under any correct expf: bit for bit with the restatement, general and exact flows alike.
    Random masks in +-4 go through the device's expf: the usual bars against the float64 module chain."""
    e, g = H.exact_family(h, w), H.family(h, w)
    m = H.sigmoid64(e["mask"]).astype(np.float32)
    for fam in (e, g):
        st = H.make_state(fam["flow"], e["mask"])
        assert _same_bits(_blend(R, fam["x6"], st), H.blend_restated(fam["x6"], st, m)), (h, w)
    got = _blend(R, g["x6"], H.make_state(g["flow"], g["mask4"])).cpu().numpy()
    ref = H.blend_module(g["x6"], g["flow"], g["mask4"], torch.float64).numpy()
    H.bars(f"GPU blend {h}x{w}", got, ref, H.blend_module(g["x6"], g["flow"], g["mask4"], torch.float32).numpy())


@pytest.mark.parametrize("h,w", H.SIZES)
def test_nonfinite_flows_read_the_border_and_leave_the_images_finite(R, h, w):
    """NaN, +Inf and -Inf flows (every index of rf_axis is clamped before use; k_rife_update takes no index from its data): the pack and the blend equal the
    restatement bit for bit -- NaN and -Inf read the left / top border pixel, +Inf the right / bottom one (tests/test_rife_glue_host.py) -- and every image,
    mask and blended value is finite.  The pack's four flow channels carry the flow itself: there a NaN matches a NaN."""
    nf, e = H.nonfinite_family(h, w), H.exact_family(h, w)
    st = H.make_state(nf["flow"], nf["mask"])
    for s in (1, 2, 4):
        got = _pack(R, nf["x6"], st, s)
        want = H.warp_pack_restated(nf["x6"], st, s)
        flows = np.zeros(want.shape, bool)
        flows[..., 7:11] = True
        assert _same_bits(got, want, flows), (h, w, s)
        assert bool(torch.isfinite(got[..., :7]).all()) and bool((got[..., 11:] == 0).all())
    st = H.make_state(nf["flow"], e["mask"])
    got = _blend(R, nf["x6"], st)
    assert _same_bits(got, H.blend_restated(nf["x6"], st, H.sigmoid64(e["mask"]).astype(np.float32)))
    assert bool(torch.isfinite(got).all())


def test_refused_calls_leave_every_byte(R):
    """Scale 3, N = 0, a misaligned pointer, t_stride 6 and 4: VD3D_E_UNSUPPORTED, and neither the outputs nor the state change."""
    from visiondepth3d_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    h, w, Hp, Wp = 33, 65, 64, 96
    x6 = torch.rand(N, 6, h, w, device="cuda")
    state = torch.full((N, Hp, Wp, 8), SENT, device="cuda")
    t = torch.rand(N, Hp, Wp, 8, device="cuda")
    out16, out3 = torch.full((N, Hp, Wp, 16), SENT, device="cuda"), torch.full((N, 3, h, w), SENT, device="cuda")
    R._enter(x6, state, t, out16, out3)
    p = lambda a, off=0: vp(a.data_ptr() + off)      # noqa: E731
    calls = [lambda: L.vd3d_rife_warp_pack(R._ctx, p(x6), p(state), N, h, w, 3, p(out16)),
             lambda: L.vd3d_rife_warp_pack(R._ctx, p(x6), p(state), 0, h, w, 1, p(out16)),
             lambda: L.vd3d_rife_warp_pack(R._ctx, p(x6, 4), p(state), N, h, w, 1, p(out16)),
             lambda: L.vd3d_rife_warp_pack(R._ctx, p(x6), p(state, 8), N, h, w, 1, p(out16)),
             lambda: L.vd3d_rife_warp_pack(R._ctx, p(x6), p(state), N, h, w, 1, p(out16, 4)),
             lambda: L.vd3d_rife_update(R._ctx, p(t), 8, 0, N, h, w, 3, p(state)),
             lambda: L.vd3d_rife_update(R._ctx, p(t), 8, 0, 0, h, w, 1, p(state)),
             lambda: L.vd3d_rife_update(R._ctx, p(t, 4), 8, 0, N, h, w, 1, p(state)),
             lambda: L.vd3d_rife_update(R._ctx, p(t), 8, 0, N, h, w, 1, p(state, 4)),
             lambda: L.vd3d_rife_update(R._ctx, p(t), 6, 0, N, h, w, 1, p(state)),
             lambda: L.vd3d_rife_update(R._ctx, p(t), 4, 1, N, h, w, 1, p(state)),
             lambda: L.vd3d_rife_blend(R._ctx, p(x6), p(state), 0, h, w, p(out3)),
             lambda: L.vd3d_rife_blend(R._ctx, p(x6, 4), p(state), N, h, w, p(out3)),
             lambda: L.vd3d_rife_blend(R._ctx, p(x6), p(state), N, h, w, p(out3, 4))]
    for i, call in enumerate(calls):
        assert call() == -4, i
        assert (b"t_stride" if i in (9, 10) else b"16-byte aligned") in L.vd3d_last_error(), i
    torch.cuda.synchronize()
    assert bool((state == SENT).all()) and bool((out16 == SENT).all()) and bool((out3 == SENT).all())
