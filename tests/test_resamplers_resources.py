"""Register / LDS budget of the resampling kernels of the depth leg (csrc/vd3d_handoff.hip k_handoff_sep, csrc/vd3d_depthprep.hip k_depth_prep_strip,
csrc/vd3d_netops.hip k_upsample_bilinear[_bias]_nhwc_f32), checked offline from hipcc's own metadata (no GPU needed).  None may spill.  The strip kernel
is planned for two 256-thread workgroups per CU: its LDS is static, so 2 x LDS <= 160 KB and two waves per SIMD x registers <= 512 are checked here."""
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
def test_handoff_forms_do_not_spill():
    k = _census("vd3d_handoff.hip")
    sep = {n: v for n, v in k.items() if n.startswith("_Z13k_handoff_sep")}
    gen = {n: v for n, v in k.items() if n.startswith("_Z9k_handoffILb")}
    assert len(sep) == 2 and len(gen) == 2, sorted(k)          # <false> (min / max) and <true> (write) of each form
    for n, v in {**sep, **gen}.items():
        assert v["spill"] == 0, (n, v)
    for n, v in sep.items():
        assert v["vgpr"] <= 128 and v["lds"] == 0, (n, v)       # one-wave workgroups, the window in registers: four waves per SIMD and more


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_prep_strip_form_fits_two_workgroups_per_cu():
    k = _census("vd3d_depthprep.hip")
    strip = {n: v for n, v in k.items() if n.startswith("_Z18k_depth_prep_strip")}
    tile = {n: v for n, v in k.items() if n.startswith("_Z12k_depth_prep")}
    assert len(strip) == 2 and len(tile) == 2, sorted(k)        # float32 and bf16 output of each form
    for n, v in {**strip, **tile}.items():
        assert v["spill"] == 0, (n, v)
    for n, v in strip.items():
        assert 2 * v["lds"] <= 160 * 1024, (n, v)               # static LDS: band rows, chunk, weights
        assert 2 * v["vgpr"] <= 512, (n, v)                     # 4 waves per workgroup = one per SIMD; two workgroups = two waves per SIMD


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_upsample_f32_kernels_do_not_spill():
    k = _census("vd3d_netops.hip")
    up = {n: v for n, v in k.items() if "k_upsample_bilinear" in n and "_f32" in n}
    assert len(up) == 4, sorted(up)                             # with / without bias x 32-bit / 64-bit row offsets
    for n, v in up.items():
        assert v["spill"] == 0 and v["vgpr"] <= 64 and v["lds"] == 0, (n, v)
