"""Register / LDS budget of the Pillow-exact front end's kernel (csrc/vd3d_pilresample.hip k_pil_resample: the uint8, float32 and bf16 epilogues), checked
offline from hipcc's own metadata (no GPU needed).  None may spill.  The plan: 256-thread workgroups (one wave per SIMD each), FOUR per CU -- the LDS is
static (coefficient rows of 32 columns and 32 rows, 160 filtered rows of 32 packed pixels, a chunk of 16 staged input rows, the 3 x 256 table), so
4 x LDS <= 160 KB, and four waves per SIMD x registers <= 512 (allocated in granules of 8) are checked here."""
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
def test_pil_resample_fits_four_workgroups_per_cu():
    k = _census("vd3d_pilresample.hip")
    forms = {n: v for n, v in k.items() if n.startswith("_Z14k_pil_resampleILi")}
    assert len(forms) == 3 and len(k) == 3, sorted(k)          # uint8, float32 and bf16 epilogue; nothing else in the file
    for n, v in forms.items():
        assert v["spill"] == 0, (n, v)
        assert 4 * v["lds"] <= 160 * 1024, (n, v)
        assert 4 * ((v["vgpr"] + 7) // 8 * 8) <= 512, (n, v)
