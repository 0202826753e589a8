"""Register / LDS budget of the fp16x2 tile convolution (k_conv_x2, csrc/vd3d_conv_x2t.hip: vd3d_conv_x3.h's body in MODE 1), checked offline from hipcc's own
metadata (no GPU needed): 512-thread workgroups, two waves per SIMD, so at most 256 registers per lane, nothing spilled, and no static LDS -- the 100 864 bytes
of the plan are dynamic LDS behind the per-device > 64 KB opt-in."""
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
def test_conv_fp16x2_instantiations_fit_two_waves_per_simd():
    k = _census("vd3d_conv_x2t.hip")
    convs = {n: v for n, v in k.items() if n.startswith("_Z9k_conv_x2ILi")}
    # stride 1 with 32 (8 x 1 waves), 64 (4 x 2, one N tile) and 128 / 256 (4 x 2, two N tiles; 256 as two slices) output channels; stride 2 with 128 n
    want = ["_Z9k_conv_x2ILi0ELi8ELi1E", "_Z9k_conv_x2ILi0ELi4ELi1E", "_Z9k_conv_x2ILi0ELi4ELi2E", "_Z9k_conv_x2ILi1ELi4ELi2E"]
    assert len(convs) == 4 and all(sum(n.startswith(w) for n in convs) == 1 for w in want), sorted(k)
    for n, v in convs.items():
        assert v["spill"] == 0 and v["vgpr"] <= 256 and v["lds"] == 0, (n, v)
    assert not any(n.startswith("_Z9k_conv_x3ILi") for n in k), sorted(k)   # the bf16x3 kernels stay in their own translation units
    for n, v in k.items():
        assert v["spill"] == 0, (n, v)                                      # the two packer kernels
