"""Register / scratch / LDS census of DepthPro's pyramid and merge kernels (csrc/vd3d_depthpro_pyramid.hip: each in its 16-byte and its 4-byte form), read offline
from hipcc's own metadata with the Makefile's flags (no GPU needed) -- the census of tests/test_depth_pro_resources.py applied to the new file.  None may spill or
use scratch.  All are memory-bound 256-thread workgroups whose launch code assumes nothing but that plenty of them are resident: at most 64 registers keeps eight
workgroups per CU (8 x 64 <= 512).  None declares LDS: 0 bytes.  Resources only -- nothing else in the code object is looked at."""
import os

import pytest

from test_depth_pro_resources import HIPCC, _census

LDS_BYTES = 0   # neither kernel declares shared memory: both are pure gathers


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_pyramid_and_merge_kernels_use_no_scratch_no_lds_and_fit_eight_workgroups_per_cu():
    k = _census("vd3d_depthpro_pyramid.hip")
    names = {"patches_vec": "_Z12k_dp_patchesILb1E", "patches_scalar": "_Z12k_dp_patchesILb0E", "merge_vec": "_Z10k_dp_mergeILb1E", "merge_scalar": "_Z10k_dp_mergeILb0E"}
    assert len(k) == len(names), sorted(k)
    for what, prefix in names.items():
        v = next(v for n, v in k.items() if n.startswith(prefix))
        print("DEPTH_PRO_PYRAMID_RESOURCES", what, v)
        assert v["spill"] == 0 and v["scratch"] == 0, (what, v)
        assert v["vgpr"] <= 64 and 8 * ((v["vgpr"] + 7) // 8 * 8) <= 512, (what, v)
        assert v["lds"] == LDS_BYTES, (what, v)
