"""Register / scratch / LDS census of ZoeDepth's kernels (csrc/vd3d_zoedepth.hip: the front end, the post-process, the attractor step in its "mean" and "sum" form
and the log-binomial tail), read offline from hipcc's own metadata with the Makefile's flags (no GPU needed).  None may spill or use scratch.  All are 256-thread
workgroups; the four memory-bound ones keep at most 64 registers (eight workgroups per CU), the tail -- 32 feature values held per pixel -- at most 128 (four).
Only the front end uses LDS: its 256-entry table of the byte, 1 KB.  Resources only -- nothing else in the code object is looked at."""
import os

import pytest

from test_depth_pro_resources import HIPCC, _census


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_zoedepth_kernels_use_no_scratch():
    k = _census("vd3d_zoedepth.hip")
    names = {"preprocess": "_Z16k_zoe_preprocess", "post": "_Z10k_zoe_post", "attractor_mean": "_Z15k_zoe_attractorILb1E", "attractor_sum": "_Z15k_zoe_attractorILb0E",
             "bins": "_Z10k_zoe_bins"}
    assert len(k) == len(names), sorted(k)
    for what, prefix in names.items():
        v = next(v for n, v in k.items() if n.startswith(prefix))
        print("ZOEDEPTH_RESOURCES", what, v)
        assert v["spill"] == 0 and v["scratch"] == 0, (what, v)
        assert (4 if what == "bins" else 8) * ((v["vgpr"] + 7) // 8 * 8) <= 512, (what, v)
        assert v["lds"] == (256 * 4 if what == "preprocess" else 0), (what, v)
