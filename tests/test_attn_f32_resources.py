"""Register / LDS budget of the exact-float32 attention kernel (k_attn_f32, csrc/vd3d_attn.hip), checked offline from hipcc's own metadata (no GPU needed):
512-thread workgroups, two waves per SIMD, so at most 256 registers per lane, no spills, and the 96 KB ring within the CU's 160 KB of LDS."""
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"


def _census(src):
    spec = importlib.util.spec_from_file_location("_vd3d_kernel_census", os.path.join(HERE, "test_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._census(src)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_attn_f32_fits_two_waves_per_simd():
    k = _census("vd3d_attn.hip")
    a = next(v for n, v in k.items() if n.startswith("_Z10k_attn_f32"))
    assert a["spill"] == 0 and a["vgpr"] <= 256, a
    assert a["lds"] == 0, a   # the ring is dynamic LDS: 3 stages x (16 KB K + 16 KB V) = 96 KB, set per device through the > 64 KB opt-in
