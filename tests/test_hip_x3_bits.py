"""GPU test (-m gpu): the tile convolutions reproduce, bit for bit, the outputs recorded in tests/golden/x3_bits.json (tools/record_x3_bits.py: the cases, the
hashed inputs and the recorder).  vd3d_conv3x3_x3 and vd3d_conv_ifn (csrc/vd3d_conv_x3.hip) were recorded with a library built from the commit before the two
kernels were merged into one; vd3d_conv3x3_s2_x3 (vd3d_conv_s2.hip), vd3d_conv3x3_s1_x2 and vd3d_conv3x3_s2_x2 (vd3d_conv_x2t.hip) with one built from the commit
before their launch side was folded into one statement per layer.  One SHA-256 of the raw output bytes per case: ragged and single-pixel tiles, wrapping chunk
buffers, every geometry at every C_out, one and two channel slices, odd and even stride-2 sizes, plain and with slope, residual, padded pitches and an output
slice (whose surroundings are hashed too)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_x3_bits", os.path.join(ROOT, "tools", "record_x3_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
CASES = rec.cases()


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)["cases"]


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(n for n, _ in CASES)


@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_x3_convolution_bits_are_the_recorded_ones(R, golden, name, spec):
    assert rec.run_case(R, spec) == golden[name]
