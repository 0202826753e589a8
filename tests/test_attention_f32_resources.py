"""Register / LDS budget of the two forms of the exact-float32 attention kernel (csrc/vd3d_attn.hip k_attn_f32<4, 2> and <8, 3>), checked offline from hipcc's
own metadata (no GPU needed).  Neither may spill (no scratch in the tile loop).  Both run two waves per SIMD -- the 4-wave form as two workgroups per CU, the
8-wave form as one -- so each has at most 256 registers per wave.  Their LDS is all dynamic (65 536 and 98 304 bytes, held by static_asserts in the source, which
this compilation evaluates): the static segment is empty, and two 4-wave workgroups fit a CU's 160 KB."""
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
def test_attention_f32_forms_fit_two_waves_per_simd_without_spilling():
    k = _census("vd3d_attn.hip")
    f4 = {n: v for n, v in k.items() if n.startswith("_Z10k_attn_f32ILi4ELi2E")}
    f8 = {n: v for n, v in k.items() if n.startswith("_Z10k_attn_f32ILi8ELi3E")}
    assert len(f4) == 1 and len(f8) == 1, sorted(k)
    for n, v in {**f4, **f8}.items():
        print(n, v)
        assert v["spill"] == 0, (n, v)
        assert v["vgpr"] <= 256, (n, v)          # two waves per SIMD x registers <= 512
        assert v["lds"] == 0, (n, v)             # the ring is the dynamic array, nothing static in front of it
