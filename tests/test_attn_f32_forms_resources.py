"""Register / LDS budget of both forms of the exact-float32 attention kernel (k_attn_f32<NW, NS>, csrc/vd3d_attn.hip), checked offline from hipcc's own
metadata (no GPU needed): the 8-wave form is one 512-thread workgroup per CU, the 4-wave form two 256-thread workgroups per CU -- two waves per SIMD either
way, so at most 256 registers per lane and no spills; the rings (96 KB / 64 KB) are dynamic LDS."""
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
def test_both_attn_f32_forms_fit_two_waves_per_simd():
    k = _census("vd3d_attn.hip")
    forms = {n: v for n, v in k.items() if n.startswith("_Z10k_attn_f32")}
    assert len(forms) == 2, sorted(forms)                       # <8, 3> and <4, 2>
    for n, v in forms.items():
        assert v["spill"] == 0 and v["vgpr"] <= 256 and v["lds"] == 0, (n, v)
