"""GPU tests (-m gpu) of vd3d_dpt_head_tail_act_f32 (csrc/vd3d_netops.hip, k_head_tail<LPP, ACT>): the depth head's tail with its last activation as an argument.

act 0 returns the bytes of vd3d_dpt_head_tail_f32; act 1 is sigmoid(v) * scale with v bit for bit the numpy statement of the kernel's order
(tests/test_dpt_metric_self_contained_host.py) and the sigmoid torch's CPU one (Renderer.torch_math); known answers at v = 0 and v = +-200; NaN containment; the
refusals, which launch nothing.  A 256-thread block holds 64 / 32 / 16 pixels for C = 16 / 32 / 64: the pixel counts are one lone pixel and the block edges of
each instantiation.

NaN: the ReLU tail's fmaxf(NaN, 0) is 0 in both of its ReLUs, so vd3d_dpt_head_tail_f32 has always turned a NaN in y into a finite value, and act 0 -- its bytes --
does the same.  The sigmoid tail keeps the NaN: exactly its own pixel comes out NaN."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_dpt_metric_self_contained_host import head_tail_reference, head_tail_v   # noqa: E402

CS = (16, 32, 64)
NS = (1, 15, 16, 17, 33, 64, 65, 1000)
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _operands(C, n, seed=0):
    g = torch.Generator().manual_seed(1000 * C + n + seed)
    y = torch.randn(n, C, generator=g)
    return y, torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.4, 0.3, 20.0


def _call(R, y, b2, w3, b3, scale, act):
    """The C entry point on an [n, C] pixel matrix -> (return code, float32 [n] on the device, pre-filled with -7)."""
    from visiondepth3d_amd import _lib
    yd, bd, wd = y.cuda().contiguous(), b2.cuda().contiguous(), w3.cuda().contiguous()
    out = torch.full((y.shape[0],), -7.0, device="cuda")
    L = _lib.lib()
    if act is None:
        rc = L.vd3d_dpt_head_tail_f32(R._ctx, vp(yd.data_ptr()), vp(bd.data_ptr()), vp(wd.data_ptr()), b3, scale, y.shape[0], y.shape[1], vp(out.data_ptr()))
    else:
        rc = L.vd3d_dpt_head_tail_act_f32(R._ctx, vp(yd.data_ptr()), vp(bd.data_ptr()), vp(wd.data_ptr()), b3, scale, y.shape[0], y.shape[1], act, vp(out.data_ptr()))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("C", CS)
def test_act0_returns_the_bytes_of_the_relu_entry_point(R, C):
    for n in NS:
        ops = _operands(C, n)
        (rc0, old), (rc1, new) = _call(R, *ops, None), _call(R, *ops, 0)
        assert rc0 == 0 and rc1 == 0
        assert np.array_equal(old.cpu().numpy().view(np.uint32), new.cpu().numpy().view(np.uint32)), (C, n)
        assert np.array_equal(new.cpu().numpy(), head_tail_reference(ops[0].numpy(), ops[1].numpy(), ops[2].numpy(), ops[3], ops[4])), (C, n)
        assert n < 15 or (bool((new > 0).any()) and bool((new == 0).any()))
        # Renderer.dpt_head_tail: "relu" (the default) and the channels_last map are the same call
        y4 = ops[0].cuda().view(1, n, 1, C).permute(0, 3, 1, 2)
        assert torch.equal(R.dpt_head_tail(y4, ops[1].cuda(), ops[2].cuda(), ops[3], ops[4]).view(-1), old)


@pytest.mark.parametrize("C", CS)
def test_act1_is_torch_sigmoid_of_the_statements_v_times_scale(R, C):
    for n in NS:
        y, b2, w3, b3, scale = _operands(C, n, seed=1)
        rc, got = _call(R, y, b2, w3, b3, scale, 1)
        assert rc == 0
        v = torch.from_numpy(head_tail_v(y.numpy(), b2.numpy(), w3.numpy(), b3, "sigmoid"))
        want = R.torch_math("sigmoid", v) * scale            # two float32 roundings
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), (C, n, float((got - want).abs().max()))
        assert bool(((got > 0) & (got < scale)).all()) and (n < 15 or float(got.max() - got.min()) > 0.1 * scale)   # not saturated, not flat
        y4 = y.cuda().view(1, n, 1, C).permute(0, 3, 1, 2)
        assert torch.equal(R.dpt_head_tail(y4, b2.cuda(), w3.cuda(), b3, scale, act="sigmoid").view(-1), got)


@pytest.mark.parametrize("C", CS)
def test_act1_known_answers(R, C):
    """Small integers: v is exact.  Pixel 0: v = 0 -> 0.5 scale; pixel 1: v = -200 -> 0; pixel 2: v = +200 -> scale; pixel 3: every channel below the inner
    ReLU -> v = b3."""
    y = torch.zeros(4, C)
    b2 = torch.full((C,), -1.0)
    w3 = torch.ones(C)
    w3[1::2] = -1.0                                   # channel pairs cancel: a row of equal values sums to 0
    y[0] = 3.0                                        # relu(2) * (+1 -1 ...) = 0
    y[1] = 3.0
    y[1, 1] = 203.0                                   # channel 1 (weight -1): relu(202) - relu(2) more on the negative side: v = -200
    y[2] = 3.0
    y[2, 0] = 203.0                                   # v = +200
    y[3] = -5.0                                       # all clipped: v = b3 = 0
    scale = 80.0
    rc, got = _call(R, y, b2, w3, 0.0, scale, 1)
    assert rc == 0
    assert np.array_equal(head_tail_v(y.numpy(), b2.numpy(), w3.numpy(), 0.0), np.array([0, -200, 200, 0], np.float32))
    assert got.cpu().tolist() == [0.5 * scale, 0.0, scale, 0.5 * scale]
    rc, got = _call(R, y, b2, w3, 2.0, scale, 1)     # b3 is added in front of the sigmoid
    assert rc == 0 and got[3].item() == float((R.torch_math("sigmoid", torch.tensor([2.0])) * scale).item())


@pytest.mark.parametrize("C", CS)
def test_one_nan_in_y_makes_exactly_its_own_pixel_nan(R, C):
    n = 65
    y, b2, w3, b3, scale = _operands(C, n, seed=2)
    rc, clean = _call(R, y, b2, w3, b3, scale, 1)
    assert rc == 0
    for pix, ch in ((0, 0), (17, C - 1), (n - 1, C // 2 + 1)):
        bad = y.clone()
        bad[pix, ch] = float("nan")
        rc, got = _call(R, bad, b2, w3, b3, scale, 1)
        assert rc == 0
        hit = torch.zeros(n, dtype=torch.bool, device="cuda")
        hit[pix] = True
        assert torch.equal(torch.isnan(got), hit), (pix, ch)
        assert torch.equal(got[~hit], clean[~hit])
        # act 0 is the ReLU entry point on this input too: its fmaxf turns the NaN into 0 (module docstring)
        (_, old), (_, new) = _call(R, bad, b2, w3, b3, scale, None), _call(R, bad, b2, w3, b3, scale, 0)
        assert np.array_equal(old.cpu().numpy().view(np.uint32), new.cpu().numpy().view(np.uint32)) and not bool(torch.isnan(new).any())


def test_refusals_launch_nothing(R):
    """act 2 is VD3D_E_INVALID; C = 48, a misaligned pointer and n_pix = 0 are refused by both entry points alike; the output keeps its bytes."""
    from visiondepth3d_amd import _abi, _lib
    L = _lib.lib()
    buf = torch.randn(64 * 64 + 4, device="cuda")
    b2, w3 = torch.randn(64, device="cuda"), torch.randn(64, device="cuda")
    out = torch.full((64,), -7.0, device="cuda")
    p, pb, pw, po = buf.data_ptr(), b2.data_ptr(), w3.data_ptr(), out.data_ptr()

    def both(y=p, b=pb, w=pw, n=64, C=64):
        old = L.vd3d_dpt_head_tail_f32(R._ctx, vp(y), vp(b), vp(w), 0.1, 2.0, n, C, vp(po))
        new = [L.vd3d_dpt_head_tail_act_f32(R._ctx, vp(y), vp(b), vp(w), 0.1, 2.0, n, C, act, vp(po)) for act in (0, 1)]
        assert new == [old, old], (old, new)
        return old

    assert L.vd3d_dpt_head_tail_act_f32(R._ctx, vp(p), vp(pb), vp(pw), 0.1, 2.0, 64, 64, 2, vp(po)) == _abi.E_INVALID and b"activation" in L.vd3d_last_error()
    assert L.vd3d_dpt_head_tail_act_f32(R._ctx, vp(p), vp(pb), vp(pw), 0.1, 2.0, 64, 64, -1, vp(po)) == _abi.E_INVALID
    assert both(C=48) == _abi.E_UNSUPPORTED and b"48" in L.vd3d_last_error()
    assert both(y=p + 4) == _abi.E_UNSUPPORTED and b"aligned" in L.vd3d_last_error()
    assert both(b=pb + 4) == _abi.E_UNSUPPORTED
    assert both(w=pw + 8) == _abi.E_UNSUPPORTED
    assert both(n=0) == _abi.E_INVALID
    assert both(y=None) == _abi.E_INVALID
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                  # nothing ran
    with pytest.raises(ValueError, match="act"):
        R.dpt_head_tail(torch.zeros(1, 16, 1, 1, device="cuda").contiguous(memory_format=torch.channels_last), b2[:16], w3[:16], 0.0, 1.0, act="tanh")
    assert both() == 0                                # and the same buffers, well formed, run
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())
