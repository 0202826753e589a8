"""GPU test (-m gpu): both forms of the exact-float32 attention (csrc/vd3d_attn.hip k_attn_f32<NW, NS>, vd3d_attention_f32_form) reproduce, bit for bit, the
outputs recorded in tests/golden/attn_f32_bits.json (tools/record_attn_f32_bits.py: the cases, the hashed inputs and the recorder), which a library built from
the commit before the tile loop was made lean wrote: scalar-base DMA addresses, the ring stage as a compile-time constant of a loop unrolled over the ring,
and a last tile whose second 32-key half lies past T leaving that half out of both products.  Per case the SHA-256 of the raw output bytes and the first
and last four words; sequence lengths with a last tile of at most 32 live keys, of more, exactly full and a single tile, 3 to 8 tiles (the loop ends behind
every copy of the unrolled body), the two depth-leg lengths, and more (b, h) pairs than one XCD group."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_attn_f32_bits", os.path.join(ROOT, "tools", "record_attn_f32_bits.py"))
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


def test_the_recorded_forms_agree(golden):
    """The parent's two forms were bit-identical: each shape's two digests are one."""
    for name, _ in CASES:
        if name.endswith("-form8"):
            assert golden[name] == golden[name[:-1] + "4"], name


@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_attention_f32_bits_are_the_recorded_ones(R, golden, name, spec):
    got = rec.run_case(R, spec)
    assert got["first"] == golden[name]["first"] and got["last"] == golden[name]["last"], (got, golden[name])
    assert got["sha256"] == golden[name]["sha256"]
