"""GPU tests (-m gpu) of vd3d_add_layernorm (csrc/vd3d_netops.hip), float32 and bf16, on BITS against the NumPy restatements of tests/test_layernorm_host.py
(proved there against float64 F.layer_norm within a derived bound, with mutants -- eps outside the root, the unbiased variance, a one-pass variance, another
gamma layout, statistics of the unrounded bf16 sum -- that the shared cases catch): unit-scale rows, variance near eps, constant rows, a large common offset,
massive channels, a wide dynamic range, a cancelling x + y, outlier gains; 384 / 768 / 1024 columns; 1, 3, 4, 5 and 1237 rows (four rows per block); with y
and without.  The raw entry point runs on buffers one row longer than `rows`: the row behind the outputs holds a sentinel.  NaN and Inf stay in their rows,
two calls give equal bits, refused calls leave the outputs as they were."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_layernorm_host as H  # noqa: E402

ROWS = (1, 3, 4, 5, 1237)
SENT = -7.5
DT_CODE = {"bf16": 0, "f32": 1}          # vd3d_dtype


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    assert (r._dt(torch.float32), r._dt(torch.bfloat16)) == (DT_CODE["f32"], DT_CODE["bf16"])
    yield r
    r.close()


def _dev(a, dtype):
    """A float32 array, or bf16 bits (uint16), on the GPU as a tensor of the kernel's type."""
    if dtype == "f32":
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.bfloat16)


def _host(t, dtype):
    return t.cpu().numpy() if dtype == "f32" else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _raw(R, dtype, x, y, g, b, rows, cols, out_s, out_n, eps=H.EPS):
    from visiondepth3d_amd import _lib
    R._enter(x, y, g, b, out_s, out_n)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    return _lib.lib().vd3d_add_layernorm(R._ctx, DT_CODE[dtype], p(x), p(y), p(g), p(b), float(eps), rows, cols, p(out_s), p(out_n))


def _operands(name, cols, dtype):
    c = H.case(name, cols, max(ROWS))
    return c if dtype == "f32" else H.as_bf16(c)


def _run(R, dtype, x, y, g, b, rows, cols):
    """One call on the first `rows` rows of buffers that hold one row more (NaN behind the inputs, a sentinel behind the outputs) -> (out_sum, out_norm) as
    NumPy arrays of rows + 1 rows."""
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16

    def grow(a):
        buf = torch.full((rows + 1, cols), float("nan"), dtype=tdt, device="cuda")
        buf[:rows] = _dev(a[:rows], dtype)
        return buf
    out_s = None if y is None else torch.full((rows + 1, cols), SENT, dtype=tdt, device="cuda")
    out_n = torch.full((rows + 1, cols), SENT, dtype=tdt, device="cuda")
    assert _raw(R, dtype, grow(x), None if y is None else grow(y), _dev(g, dtype), _dev(b, dtype), rows, cols, out_s, out_n) == 0
    torch.cuda.synchronize()
    return None if out_s is None else _host(out_s, dtype), _host(out_n, dtype)


def _sentinel(dtype):
    return np.float32(SENT) if dtype == "f32" else H.to_bf16(np.float32(SENT))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cols", H.COLS)
@pytest.mark.parametrize("name", H.CASES)
def test_add_layernorm_equals_its_restatement_bit_for_bit(R, name, cols, dtype):
    """Every case, with y and without, at 1, 3, 4, 5 and 1237 rows: out_norm has the restatement's bits, out_sum ATen's x + y, the row behind both keeps the
    sentinel, a second call the same bits.  Printed: the float64 error beside ATen's own float32 CPU layer_norm (the yardstick)."""
    x, y, g, b = _operands(name, cols, dtype)
    restated = H.ln_restated_f32 if dtype == "f32" else H.ln_restated_bf16
    view = (lambda a: a.view(np.uint32)) if dtype == "f32" else (lambda a: a)
    for yy in ((y, None) if y is not None else (None,)):
        want_s, want_n = restated(x, yy, g, b, H.EPS)
        if yy is not None:
            aten = _host(_dev(x, dtype) + _dev(yy, dtype), dtype)
            assert np.array_equal(view(want_s), view(aten))
        for rows in ROWS:
            got_s, got_n = _run(R, dtype, x, yy, g, b, rows, cols)
            assert np.array_equal(view(got_n[:rows]), view(want_n[:rows])), (name, cols, dtype, rows, yy is not None)
            assert bool((got_n[rows] == _sentinel(dtype)).all())
            if yy is not None:
                assert np.array_equal(view(got_s[:rows]), view(want_s[:rows])) and bool((got_s[rows] == _sentinel(dtype)).all())
        again_s, again_n = _run(R, dtype, x, yy, g, b, max(ROWS), cols)
        assert np.array_equal(view(again_n), view(got_n)) and (yy is None or np.array_equal(view(again_s), view(got_s)))
        # the figures against float64
        wide = (lambda a: a.astype(np.float64)) if dtype == "f32" else (lambda a: H.bf2f(a).astype(np.float64))
        s = wide(x) if yy is None else wide(want_s)
        ref = H.reference(s, wide(g), wide(b))
        tt = lambda a: torch.from_numpy(np.asarray(a, np.float32))      # noqa: E731
        yard = torch.nn.functional.layer_norm(tt(s), (cols,), tt(wide(g)), tt(wide(b)), H.EPS)
        if dtype == "bf16":
            yard = yard.to(torch.bfloat16).float()
        e, e32 = float(np.abs(wide(got_n[:-1]) - ref).max()), float(np.abs(yard.numpy().astype(np.float64) - ref).max())
        ratio = float((np.abs(wide(got_n[:-1]) - ref) / H.bound(s, wide(g), wide(b), ref, dtype == "bf16")).max())
        print(f"LN_F64 {name} cols {cols} {dtype} y{int(yy is not None)}: max err {e:.3e} (ATen f32 cpu {e32:.3e}), {ratio:.3f} x the derived bound")
        assert ratio <= 1.0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cols", H.COLS)
def test_nan_and_inf_stay_in_their_rows(R, cols, dtype):
    """A NaN in row 1 (through x) and an Inf in row 6 (through y) of 9 rows: exactly those rows of out_norm are non-finite, every other row keeps the bits
    of the clean run."""
    x, y, g, b = (a if a.ndim == 1 else a[:9].copy() for a in _operands("unit", cols, dtype))
    _, clean = _run(R, dtype, x, y, g, b, 9, cols)
    x[1, 5] = np.float32("nan") if dtype == "f32" else 0x7fc0
    y[6, cols - 1] = np.float32("inf") if dtype == "f32" else 0x7f80
    _, got = _run(R, dtype, x, y, g, b, 9, cols)
    gf = got[:9] if dtype == "f32" else H.bf2f(got[:9])
    bad = ~np.isfinite(gf)
    assert bool(bad[[1, 6]].all()) and not bool(bad[[0, 2, 3, 4, 5, 7, 8]].any())
    keep = [0, 2, 3, 4, 5, 7, 8, 9]
    assert np.array_equal(got[keep].view(np.uint32 if dtype == "f32" else np.uint16), clean[keep].view(np.uint32 if dtype == "f32" else np.uint16))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_refused_calls_leave_the_outputs(R, dtype):
    """cols 512: VD3D_E_UNSUPPORTED; rows 0 and y without out_sum: VD3D_E_INVALID; nothing is written."""
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    x, y = torch.ones(8, 1024, dtype=tdt, device="cuda"), torch.ones(8, 1024, dtype=tdt, device="cuda")
    g, b = torch.ones(1024, dtype=tdt, device="cuda"), torch.zeros(1024, dtype=tdt, device="cuda")
    out_s, out_n = torch.full((8, 1024), SENT, dtype=tdt, device="cuda"), torch.full((8, 1024), SENT, dtype=tdt, device="cuda")
    assert _raw(R, dtype, x, y, g, b, 8, 512, out_s, out_n) == -4
    assert _raw(R, dtype, x, y, g, b, 0, 1024, out_s, out_n) == -1
    assert _raw(R, dtype, x, y, g, b, 8, 1024, None, out_n) == -1
    torch.cuda.synchronize()
    assert bool((out_s == SENT).all()) and bool((out_n == SENT).all())
    assert _raw(R, dtype, x, y, g, b, 8, 1024, out_s, out_n) == 0          # the same buffers are accepted once the arguments are right
    torch.cuda.synchronize()
    assert bool((out_s == 2).all()) and bool((out_n == 0).all())
