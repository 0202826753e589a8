"""GPU test (-m gpu) of the device currency of the glue entry points: vd3d_add_layernorm, vd3d_upsample_bilinear_nhwc and the three vd3d_rife_* calls make
their context's device current themselves.  One call through Renderer(0), then one through Renderer(1) while device 0 STAYS current in the caller (no
torch.cuda.device(1) around it, unlike tests/test_hip_operand_range.py test_on_a_second_device): equal bits.  Skips with fewer than two GPUs."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_layernorm_host as LN  # noqa: E402
import test_rife_glue_host as RG  # noqa: E402


def _layernorm(dtype):
    def op(r, dev):
        x, y, g, b = (torch.from_numpy(a).to(dev, dtype) for a in LN.case("massive", 768, 5))
        ln = torch.nn.LayerNorm(768, eps=LN.EPS).to(dev, dtype)
        with torch.no_grad():
            ln.weight.copy_(g)
            ln.bias.copy_(b)
            s, n = r.add_layernorm(x, y, ln)
        return torch.cat((s, n)).float()
    return op


def _upsample(r, dev):
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 8, 5, 7)).astype(np.float32)).to(dev).contiguous(memory_format=torch.channels_last)
    return r.upsample_bilinear(x, (11, 13)).contiguous().flatten()


def _rife(r, dev):
    g = RG.family(33, 65)
    x6, st = torch.from_numpy(g["x6"]).to(dev), torch.from_numpy(RG.make_state(g["flow"], g["mask"])).to(dev)
    t, state = (torch.from_numpy(a).to(dev) for a in RG.update_inputs(33, 65, 2))
    pack = r.rife_warp_pack(x6, st, 2, torch.full((RG.BATCH, 32, 48, 16), -7.5, device=dev))
    upd = r.rife_update(t, state, 2, False, 33, 65)
    blend = r.rife_blend(x6, st, torch.full((RG.BATCH, 3, 33, 65), -7.5, device=dev))
    return torch.cat((pack.flatten(), upd.flatten(), blend.flatten()))


OPS = {"add_layernorm_f32": _layernorm(torch.float32), "add_layernorm_bf16": _layernorm(torch.bfloat16), "upsample_bilinear_f32": _upsample, "rife_glue": _rife}


@pytest.mark.parametrize("name", sorted(OPS))
def test_glue_on_a_second_device_while_device_0_is_current(name):
    if torch.cuda.device_count() < 2:
        pytest.skip("only one GPU visible")
    from visiondepth3d_amd.render_3d import Renderer
    outs = []
    for d in (0, 1):
        r = Renderer(d)
        try:
            torch.cuda.set_device(0)
            outs.append(OPS[name](r, f"cuda:{d}").cpu())
        finally:
            r.close()
            torch.cuda.set_device(0)
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
