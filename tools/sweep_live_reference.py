#!/usr/bin/env python3
"""Offline sweeps of the CPU oracle against the LIVE reference (development container only: /root/reference must be present).

    python tools/sweep_live_reference.py shift [first last]     # pixel_shift_cuda, random parameters / sizes   (tests: seeds 0..23 + worst)
    python tools/sweep_live_reference.py loops [first last]     # render_sbs_3d loop, random configurations      (tests: seeds 0..7 + worst)
    python tools/sweep_live_reference.py helpers [first last]   # leaf functions
    python tools/sweep_live_reference.py geometry [first last]  # VR / Full-SBS / preserve-aspect geometry combinations, DOF up to 3.0
    python tools/sweep_live_reference.py fullsize               # pixel_shift_cuda at 1080p and 4K, the 1080p Half-SBS loop

The committed tests (tests/test_oracle_vs_live_reference.py) hold a subset of each sweep plus the worst seeds found here, replayed from
tests/golden/live_sweeps.npz; this script records the reference on other seeds (make_golden.record_live) and runs the same tests on them.  DESIGN.md section 2 quotes its results (round 1: shift 100..399, loops 100..159, helpers 100..199, geometry 0..15).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "tests", "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _run(fn, seeds, *args):
    fails = []
    for seed in seeds:
        try:
            fn(*args, seed)
        except AssertionError as e:
            fails.append((seed, str(e)[:240]))
    print(f"{fn.__name__}: {len(fails)} of {len(seeds)} outside the bars")
    for f in fails[:20]:
        print("  ", f)


def main():
    import make_golden as mg
    import test_oracle_vs_live_reference as T
    from oracle import oracle as O
    what = sys.argv[1] if len(sys.argv) > 1 else "shift"
    lo, hi = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (100, 160)
    if what == "shift":
        _run(T.test_pixel_shift_random_parameters, range(lo, hi), mg.record_live({"shiftrand": range(lo, hi)}), O)
    elif what == "loops":
        _run(T.test_render_loop_random_configurations, range(lo, hi), mg.record_live({"looprand": range(lo, hi)}), O)
    elif what == "helpers":
        _run(T.test_helpers_random_inputs, range(lo, hi), mg.record_live({"helpers": range(lo, hi)}), O)
    elif what == "geometry":
        from conftest import b2_max_bound, u8_diff_stats
        from visiondepth3d_amd import synth
        from visiondepth3d_amd.params import render_kwargs_to_params
        bad = 0
        for seed in range(lo, hi):
            rng = np.random.default_rng(17000 + seed)
            fmt = ["VR", "Full-SBS", "Full-SBS", "Half-SBS"][int(rng.integers(0, 4))]
            sh = int(rng.integers(40, 140)) // 2 * 2
            sw = int(round(sh * [16 / 9, 4 / 3, 2.0, 1.0][int(rng.integers(0, 4))])) // 2 * 2
            oh = int(rng.integers(40, 200)) // 2 * 2
            kw = dict(output_format=fmt, output_height=oh, fg_shift=float(rng.uniform(2, 20)), mg_shift=float(rng.uniform(-6, 2)),
                      bg_shift=float(rng.uniform(-15, 0)), sharpness_factor=float(rng.uniform(0.0, 0.4)),
                      dof_strength=float([0.0, 2.0, 3.0][int(rng.integers(0, 3))]), feather_strength=float(rng.uniform(0, 15)),
                      blur_ksize=int(rng.integers(0, 5)) * 2 + 1, use_subject_tracking=bool(rng.integers(0, 2)),
                      use_floating_window=bool(rng.integers(0, 2)))
            if rng.integers(0, 2) and fmt != "VR":
                kw.update(preserve_original_aspect=True, original_video_width=int(rng.integers(40, 200)) // 2 * 2,
                          original_video_height=int(rng.integers(40, 120)) // 2 * 2)
            mg.LOOP_CASES["_sweep"] = (sh, sw, 3, kw)
            try:
                written = np.stack(mg.run_loop("_sweep"))
            finally:
                del mg.LOOP_CASES["_sweep"]
            frames, depths = synth.synth_clip(3, sh, sw)
            ro = O.RenderOracle(render_kwargs_to_params(sw, sh, **kw))
            ro.new_clip()
            got = np.stack([ro.render(f, synth.depth_to_u8_bgr(d), 1) for f, d in list(zip(frames, depths))[1:]])
            mx, frac, g1 = u8_diff_stats(got, written) if got.shape == written.shape else (999, 1.0, 1.0)
            ok = mx <= b2_max_bound(kw) and g1 < 5e-3 and frac < 1.5e-2
            bad += 0 if ok else 1
            print(seed, "ok" if ok else "DIFF", fmt, (sh, sw, oh), got.shape[1:3], mx, round(frac, 4), round(g1, 4))
        print("outside the bars:", bad)
    elif what == "fullsize":
        T.test_pixel_shift_full_size_1080p(mg.record_live({"full1080": [0]}), O)
        print("1080p pixel_shift_cuda: inside the bars")
        from conftest import u8_diff_stats
        from visiondepth3d_amd import synth
        from visiondepth3d_amd.params import render_kwargs_to_params
        sh, sw = 1080, 1920
        kw = dict(output_format="Half-SBS", output_height=sh, fg_shift=10.0, mg_shift=-2.5, bg_shift=-5.0, sharpness_factor=0.15,
                  dof_strength=2.0, feather_strength=10.0, blur_ksize=9, use_subject_tracking=True, use_floating_window=True)
        mg.LOOP_CASES["_sweep"] = (sh, sw, 3, kw)
        t0 = time.time()
        try:
            written = np.stack(mg.run_loop("_sweep"))
        finally:
            del mg.LOOP_CASES["_sweep"]
        frames, depths = synth.synth_clip(3, sh, sw)
        ro = O.RenderOracle(render_kwargs_to_params(sw, sh, **kw))
        ro.new_clip()
        got = np.stack([ro.render(f, synth.depth_to_u8_bgr(d), 1) for f, d in list(zip(frames, depths))[1:]])
        print("1080p Half-SBS loop (max, differing, > 1 LSB):", [u8_diff_stats(got[i], written[i]) for i in range(len(got))], f"{time.time() - t0:.0f} s")
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
