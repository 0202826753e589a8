"""Host half of the stream-order tests (tests/stream_order.py): the table covers every function that calls ``_enter``, every device pointer a wrapper hands to the
library is among its ``_enter`` arguments, and every row keeps the safety rule -- only float / uint8 sample data, declared payload by the row, is ever late."""
import os
import shutil
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_order as SO   # noqa: E402

EXCLUDED_AS_WRITTEN = 13   # the exclusion list may not grow


def test_every_enter_caller_has_a_row_or_a_reason():
    assert not SO.completeness_problems(), "\n".join(SO.completeness_problems())
    assert len(SO.EXCLUDED) <= EXCLUDED_AS_WRITTEN and all(len(r) > 20 for r in SO.EXCLUDED.values())
    ids = [r for r, _, _ in SO.ROWS]
    assert len(ids) == len(set(ids))
    callers = SO.enter_callers()
    assert len(callers) > 85 and {"linear_x3", "run_rife", "preview_heatmap", "depth_normalize_pclip"} <= set(callers)


def test_every_pointer_is_ordered_by_enter():
    assert not SO.static_problems(), "\n".join(SO.static_problems())


def _tampered(tmp_path, edit):
    for rel in SO.SOURCES:
        os.makedirs(os.path.dirname(tmp_path / rel), exist_ok=True)
        shutil.copy(os.path.join(SO.ROOT, rel), tmp_path / rel)
    p = tmp_path / "visiondepth3d_amd/render_3d.py"
    src = p.read_text()
    new = edit(src)
    assert new != src
    p.write_text(new)
    return str(tmp_path)


def test_static_check_names_a_pointer_left_out_of_enter(tmp_path):
    """``depth_normalize_pclip`` as it was: ``lo_hi`` handed to the kernel and left out of ``_enter(p, out)``."""
    root = _tampered(tmp_path, lambda s: s.replace("self._enter(p, out, lo_hi)", "self._enter(p, out)"))
    got = SO.static_problems(root)
    assert len(got) == 1 and "depth_normalize_pclip passes 'lo_hi' to the library and leaves it out of _enter(out, p)" in got[0], got
    root = _tampered(tmp_path, lambda s: s.replace("        self._enter(x, w_image, bias, out)\n", ""))
    got = SO.static_problems(root)
    assert len(got) == 1 and "linear_x3 passes device pointers to the library and never calls _enter" in got[0], got
    tail = "1 if gelu else 0, _ptr(out)))\n"
    root = _tampered(tmp_path, lambda s: s.replace("        self._enter(x, w_image, bias, out)\n", "").replace(tail, tail + "        self._enter(x, w_image, bias, out)\n"))
    assert any("linear_x3 takes a device pointer before its first _enter" in m for m in SO.static_problems(root))


def test_completeness_check_names_a_wrapper_without_a_row(tmp_path):
    extra = ("    def brand_new_op(self, x):\n        out = torch.empty_like(x)\n        self._enter(x, out)\n"
             "        _lib.check(self._L.vd3d_torch_math(self._ctx, 2, _ptr(x), 0.0, _ptr(out), x.numel()))\n        return out\n\n")
    root = _tampered(tmp_path, lambda s: s.replace("    def quantiles(self", extra + "    def quantiles(self"))
    got = SO.completeness_problems(root)
    assert len(got) == 1 and "brand_new_op calls _enter and has neither a row" in got[0], got


@pytest.fixture(scope="module")
def stub():
    return SO.stub_renderer()


@pytest.mark.parametrize("rid", [r for r, _, _ in SO.ROWS])
def test_only_declared_float_or_uint8_payload_is_late(stub, rid):
    case = SO.CASES[rid](stub)
    SO.check_late_rule(case, rid)
    for n, t in {**case.late, **case.early}.items():
        assert torch.is_tensor(t) and t.device.type == "cpu", (rid, n)


def test_the_late_rule_refuses_indices_and_undeclared_operands():
    call = lambda R, o: ()   # noqa: E731
    with pytest.raises(AssertionError, match="only float and uint8"):
        SO.check_late_rule(SO.StreamCase({"origins": np.zeros((2, 3), np.int32)}, {}, call, ("origins",)), "t")
    with pytest.raises(AssertionError, match="declared payload"):
        SO.check_late_rule(SO.StreamCase({"x": np.zeros(3, np.float32)}, {}, call, ()), "t")
    SO.check_late_rule(SO.StreamCase({"x": np.zeros(3, np.float32), "f": np.zeros(3, np.uint8)}, {"tab": np.zeros(3, np.int64)}, call, ("x", "f")), "t")
    bf = SO.StreamCase({"x": np.zeros(3, np.int16)}, {}, call, ("x",))   # the arena rows' bf16 operands travel as their int16 bits
    assert bf.late["x"].dtype == torch.bfloat16
    SO.check_late_rule(bf, "t")


def test_depth_pipe_refuses_a_private_stream_renderer():
    """DepthPipe's docstring: a renderer "on the SAME stream as the network".  depth.py orders nothing by hand, so a renderer with a stream of its own would race."""
    from visiondepth3d_amd.depth import DepthPipe
    with pytest.raises(ValueError, match="SAME stream as the network"):
        DepthPipe("depth-anything-v2-small", device="cpu", renderer=types.SimpleNamespace(_private=True))
