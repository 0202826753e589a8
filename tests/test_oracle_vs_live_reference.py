"""CPU-only cross-check of the oracle against the reference over seeded random sweeps of ``pixel_shift_cuda`` parameters, render-loop
controls and sizes.  The reference's outputs for exactly these draws (tests/golden/cases.py) were recorded by running the reference itself
(tests/golden/make_golden.py live -> tests/golden/live_sweeps.npz, with cases.LIVE_THREADS torch intra-op threads); each test draws its
case again, checks that it is the recorded one, runs the oracle and compares.  Complements the fixed cases of the other goldens: these
sweeps widen the pinned region.  The recording keeps SHA-256 + row sums of every output the oracle reproduces EXACTLY -- in its default
mode, or in the N-thread ATen mode / dense DOF order where the default mode is held to bars: the tests first check that exact output
against the digest, then measure the default mode against it (the reference's output, bit for bit)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases as C  # noqa: E402
from conftest import b2_max_bound, load_golden, u8_diff_stats  # noqa: E402
from visiondepth3d_amd import synth  # noqa: E402
from visiondepth3d_amd._abi import ShiftParams, State  # noqa: E402

THREADS = C.LIVE_THREADS     # the N of the N-thread ATen mode: the recording reference process's torch.get_num_threads()


@pytest.fixture(scope="module")
def live():
    g = load_golden("live_sweeps.npz")
    assert int(g["threads"]) == THREADS
    return g


def _recorded(live, key, case):
    """The recorded case `key`, after checking that the reference ran on the case this test draws."""
    drawn = json.loads(bytes(live["cases_json"]).decode())[key]
    assert drawn == json.loads(json.dumps(case)), (key, drawn, case)
    return lambda field: live[f"{key}__{field}"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _digest_mismatch(live, key, frames):
    """None if every frame (plane) of `frames` has the recorded SHA-256, else where the first one differs (row sums locate it)."""
    frames = list(frames)
    if len(frames) != int(live[f"{key}__n"]) or tuple(frames[0].shape) != tuple(int(v) for v in live[f"{key}__shape"]):
        return ("shape", len(frames), frames[0].shape, int(live[f"{key}__n"]), tuple(live[f"{key}__shape"]))
    for i, fr in enumerate(frames):
        if _sha(fr) != bytes(live[f"{key}__sha_{i}"]).decode():
            rs = (fr.astype(np.float64) if fr.dtype.kind == "f" else fr.astype(np.int64)).reshape(fr.shape[0], -1).sum(axis=1)
            rows = np.nonzero(rs != live[f"{key}__rowsum_{i}"])[0]
            return ("frame", i, "rows whose sums differ", rows[:10].tolist(), len(rows))
    return None


def _exact_loop(live, oracle, key, case, params, blank=()):
    """The oracle's loop frames in the N-thread ATen mode, checked against the digest of the reference's: the reference's frames, bit for bit."""
    _recorded(live, key, case)
    sh, sw, n = case[:3]
    frames = _oracle_loop(oracle, sh, sw, n, params, blank)
    bad = _digest_mismatch(live, key, frames)
    assert bad is None, (key, bad, case)
    return frames


def _aspect_ratios(live):
    return json.loads(bytes(live["aspect_ratios_json"]).decode())


def _oracle_loop(oracle, sh, sw, n, params, blank=()):
    frames, depths = synth.synth_clip(n, sh, sw)
    ro = oracle.RenderOracle(params)
    ro.new_clip()
    return np.stack([ro.render(f, synth.depth_to_u8_bgr(d), 1, **({"blank": True} if i in blank else {}))
                     for i, (f, d) in enumerate(list(zip(frames, depths))[1:])])


@pytest.mark.parametrize("seed", C.SHIFT_RANDOM_SEEDS)
def test_pixel_shift_random_parameters(live, oracle, seed):
    ih, iw, H, W, fg, mg, bg, kw = case = C.shift_random_case(seed)
    ref = _recorded(live, f"shiftrand{seed}", case)
    bgr, d = synth.synth_frame(seed, ih, iw)
    ft = oracle.frame_to_tensor(bgr)
    # Round 5: the N-thread ATen mode (aten_threads = the reference process's torch.get_num_threads()) restates the two size-dependent ATen code paths these odd
    # sizes hit -- libm on the scalar tails of pow / sigmoid, the premultiplied-weight bilinear kernel for outputs with H + W <= 128 -- and is EXACT here: tracker,
    # shift map, both eyes (offline: 400 of 400 seeds at 1, 3, 4 and 8 threads).
    st_a = State()
    oa = oracle.pixel_shift(ft, d[None], W, H, ShiftParams.defaults(fg, mg, bg, aten_threads=THREADS, **kw), st_a, want_shift=True)
    assert st_a.fw_prev_offset == float(ref("prev_offset")), (seed, kw)
    for nm, got in (("S", oa["shift"]), ("L", oa["left"]), ("R", oa["right"])):
        bad = _digest_mismatch(live, f"shiftrand{seed}_{nm}", [got])
        assert bad is None, (seed, nm, (ih, iw, H, W), bad, kw)
    rl, rr, rs = oa["left"], oa["right"], oa["shift"]    # = the reference's eyes and shift map, bit for bit
    # ... and the default, thread-independent mode (aten_threads = 0: SLEEF values and the nested bilinear form everywhere) stays within the bounds below
    st = State()
    o = oracle.pixel_shift(ft, d[None], W, H, ShiftParams.defaults(fg, mg, bg, **kw), st, want_shift=True)
    assert st.fw_prev_offset == float(ref("prev_offset")), (seed, kw)
    # shift map: on these odd-sized planes ATen runs its SCALAR loop on the last n mod 32 elements (std::pow in double there, not the
    # SLEEF value the oracle restates), so up to 31 elements can differ by an ULP of a layer weight (6e-8), amplified by
    # amp = (1.2 fg + |mg| + 1.1 |bg|) / (W/2) -- above 1 only for the tiny widths of this sweep.  4e-7 * max(1, amp) in normalised
    # units is < 1e-4 pixel.  (The untailed variant of this sweep below is exact.)
    # Outputs with H + W <= 128 (ATen UpSampleKernel.cpp `_use_vectorized_kernel_cond_2d`; also 3-channel inputs when torch runs ONE thread;
    # only in sweeps like this one -- an earlier note here said "below ~4 K elements"): ATen's CPU bilinear kernel switches to a variant with PREMULTIPLIED
    # weights (p01*w01, then fma(p00,w00,.), fma(p10,w10,.), fma(p11,w11,.)) -- identified bit-exactly -- which is 1 ULP away from the
    # nested form it uses for every real frame size (and the oracle uses); a depth edge amplifies that: 1e-6 (worst of 940: 7.3e-7).
    amp = (1.2 * fg + abs(mg) + 1.1 * abs(bg)) / (W / 2)
    tol = (4e-7 if H * W >= 4200 else 1e-6) * max(1.0, amp)
    assert np.max(np.abs(o["shift"] - rs)) < tol, (seed, amp, kw)
    for got, exp, eye in ((o["left"], rl, "L"), (o["right"], rr, "R")):
        mx, frac, _ = u8_diff_stats(got, exp)
        # <= 1 LSB everywhere (the B1 bar); how MANY samples sit on a truncation cliff depends on the content: 940-seed sweep max 0.82 %
        assert mx <= 1 and frac < 1e-2, (seed, eye, mx, frac, kw)




@pytest.mark.parametrize("seed", C.SHIFT_UNTAILED_SEEDS)
def test_pixel_shift_random_parameters_exact_on_untailed_planes(live, oracle, seed):
    """The same sweep on planes whose element count is a multiple of 32 and >= 4200 (every real frame size is): with torch-CPU's
    pow / sigmoid (SLEEF) and sqrt (MKL VML) restated bit for bit in the oracle, the shift map AND both eyes equal the reference's
    EXACTLY.  What the sweep above still tolerates is confined to sizes no video has: ATen's scalar loop on the last n mod 32 elements
    of a worker's chunk (std::pow in double there) and its premultiplied bilinear variant below ~4 K elements."""
    ih, iw, H, W, fg, mg, bg, kw = case = C.shift_untailed_case(seed)
    ref = _recorded(live, f"shiftutl{seed}", case)
    bgr, d = synth.synth_frame(seed, ih, iw)
    ft = oracle.frame_to_tensor(bgr)
    st = State()
    o = oracle.pixel_shift(ft, d[None], W, H, ShiftParams.defaults(fg, mg, bg, **kw), st, want_shift=True)
    assert st.fw_prev_offset == float(ref("prev_offset")), (seed, kw)
    for nm, got in (("S", o["shift"]), ("L", o["left"]), ("R", o["right"])):
        bad = _digest_mismatch(live, f"shiftutl{seed}_{nm}", [got])
        assert bad is None, (seed, nm, bad, kw)


@pytest.mark.parametrize("seed", C.LOOP_RANDOM_SEEDS)
def test_render_loop_random_configurations(live, oracle, seed):
    """The real ``render_sbs_3d`` loop of the reference (fake VideoCapture / VideoWriter of ref_stubs) vs the oracle on
    random configurations; bars of the committed B2 goldens (tests/test_oracle_vs_golden.py)."""
    from visiondepth3d_amd.params import render_kwargs_to_params
    sh, sw, n, kw = case = C.loop_random_case(seed)
    written = _exact_loop(live, oracle, f"looprand{seed}", case, render_kwargs_to_params(sw, sh, aten_sum_threads=THREADS, **kw))
    got = _oracle_loop(oracle, sh, sw, n, render_kwargs_to_params(sw, sh, **kw))
    assert got.shape == written.shape, (got.shape, written.shape, kw)
    mx, frac, frac_gt1 = u8_diff_stats(got, written)
    # >= 99.5 % of the samples within 1 LSB; the maximum is bounded by what grade / sharpen / anaglyph can make of 1 LSB (conftest)
    fb, fb1 = _cliff_bars(kw)
    assert mx <= b2_max_bound(kw) and frac_gt1 < fb1 and frac < fb, (seed, mx, b2_max_bound(kw), frac, frac_gt1, kw)


def _cliff_bars(kw):
    """(fraction of differing samples, fraction differing by > 1 LSB) allowed end to end.  apply_dof_cuda blends level 0 (the pixel
    itself, exactly c/255) with level 1 = gaussian_blur(sigma = max_sigma/4).  Wherever the 4-neighbour Laplacian of the uint8 eye
    is exactly 0 (about 3 % of the samples of the noisy synthetic frames), level 1 equals c/255 up to float32 summation noise --
    for sigma <= 0.25 the corner taps (weight 1e-7) are below that noise as well -- so `(x*255).astype(uint8)` lands on c or c-1
    by accident of the conv's summation order: the reference is not reproducible there (its dense conv vs any other association;
    the float outputs agree to 6e-7, test_helpers_random_inputs).  For max_sigma >= 2 the corner taps (weight 1e-2) break the tie
    for all but ~0.2 % of the samples.  Measured over a 40-configuration offline sweep: <= 2.6 % / 1.1 % at max_sigma = 1."""
    if 0.0 < float(kw.get("dof_strength", 0.0)) < 1.5:
        return 4e-2, 2e-2
    return 1.5e-2, 5e-3


@pytest.mark.parametrize("seed", C.LETTERBOX_SEEDS)
def test_letterbox_aspect_loops_random_configurations(live, oracle, seed):
    """Random letterbox bars x auto_crop_black_bars on / off x the reference's seven aspect-ratio labels x formats x output heights
    through the real loop (40-seed offline sweep: one configuration exceeded the old fixed maximum of 8 -- 1 LSB at the warp output
    turned into 2 by the identity grade's own truncation, then x 8 by the sharpen; b2_max_bound now states that bound)."""
    from visiondepth3d_amd.params import render_kwargs_to_params
    aspect_ratios = _aspect_ratios(live)
    sh, sw, n, top, bottom, label, kw = case = C.letterbox_case(seed, list(aspect_ratios))
    _recorded(live, f"letterbox{seed}", case)
    frames, depth_bgr = synth.letterbox_clip(n, sh, sw, top, bottom)

    def render(**extra):
        ro = oracle.RenderOracle(render_kwargs_to_params(sw, sh, target_ratio=aspect_ratios[label], **extra, **kw))
        ro.new_clip()
        return np.stack([ro.render(f, d, 1) for f, d in list(zip(frames, depth_bgr))[1:]])
    written = render(aten_sum_threads=THREADS)     # the reference's frames, bit for bit:
    bad = _digest_mismatch(live, f"letterbox{seed}", written)
    assert bad is None, (seed, bad, kw, label)
    got = render()
    assert got.shape == written.shape, (got.shape, written.shape, kw, label)
    mx, frac, frac_gt1 = u8_diff_stats(got, written)
    assert mx <= b2_max_bound(kw) and frac_gt1 < 5e-3 and frac < 1.5e-2, (seed, mx, b2_max_bound(kw), frac, frac_gt1, kw, label)


@pytest.mark.parametrize("seed", C.BLANK_RANDOM_SEEDS)
def test_blank_frame_loops_random_configurations(live, oracle, seed):
    """skip_blank_frames in the real loop of the reference (blackdetect list injected) on random configurations, incl. output
    heights that differ from the source (the blank frame keeps the SOURCE size): blank frames bit-exact, the others within the bars."""
    from visiondepth3d_amd.params import render_kwargs_to_params
    sh, sw, n, blank, kw = case = C.blank_random_case(seed)
    written = _exact_loop(live, oracle, f"blankrand{seed}", case, render_kwargs_to_params(sw, sh, aten_sum_threads=THREADS, **kw), blank)
    got = _oracle_loop(oracle, sh, sw, n, render_kwargs_to_params(sw, sh, **kw), blank)
    assert got.shape == written.shape, (got.shape, written.shape, kw)
    fb, fb1 = _cliff_bars(kw)
    for i in range(len(got)):
        mx, frac, frac_gt1 = u8_diff_stats(got[i], written[i])
        if i in blank:
            assert mx == 0, (seed, i, mx, frac, kw)
        else:
            assert mx <= b2_max_bound(kw) and frac_gt1 < fb1 and frac < fb, (seed, i, mx, frac, frac_gt1, kw)


@pytest.mark.parametrize("seed", C.HELPER_SEEDS)
def test_helpers_random_inputs(live, oracle, seed):
    """Leaf functions of the path on random planes / parameters against the reference: order statistics, subject depth,
    dynamic parallax scale and motion metric exact; shaping exact in the N-thread ATen mode (random plane sizes: ATen's scalar tail loop calls libm's pow on
    the last n mod 32 elements; within 1 ULP in the default mode), DOF and grade within 1 LSB (separable vs dense summation)."""
    import torch
    h, w, quant, gamma, mid, focal, ms, sat, con, bri = case = C.helper_case(seed)
    ref = _recorded(live, f"helpers{seed}", case)
    d, d2, bgr = C.helper_planes(seed, h, w, quant)
    dt = torch.from_numpy(d.copy())[None]
    # order statistics (torch.quantile itself) / subject depth: exact
    for q in (0.02, 0.05, 0.5, 0.95, 0.98):
        assert np.float32(oracle.quantile(d, q)) == np.float32(torch.quantile(dt.flatten(), q).item()), (seed, q)
    assert np.float32(oracle.subject_depth(d)) == np.float32(ref("subject_depth")), seed
    # reductions: EXACT since round 5 -- torch.mean is ATen's float32 cascade sum / n, restated for any thread count (vo_sum_aten_2d; torch.var accumulates
    # in float64 and equals the rounded exact variance); the order-free exact mean (aten_threads = 0, the library's default) stays within one float32 ULP
    got = oracle.dynamic_parallax_scale(d, 0.90, 1.15, aten_threads=THREADS)
    exp = float(ref("dyn_scale"))
    assert got == exp, (seed, got, exp)
    assert abs(oracle.dynamic_parallax_scale(d, 0.90, 1.15) - exp) < 2e-6
    mm = oracle.motion_metric(d, d2, aten_threads=THREADS)
    assert mm == float(ref("motion")), seed
    assert abs(oracle.motion_metric(d, d2) - mm) < 2e-6
    # curvature + shaping: exact except the (n mod 32)-element tail, where torch calls libm's pow -> <= 1 ULP of values in [0,1]
    c = oracle.curvature_clamp(d, 0.08)
    c_ref = ref("curv")
    assert np.max(np.abs(c - c_ref)) <= 6e-8, seed
    s0 = float(ref("s0"))
    sh_a = oracle.shape_depth_for_pop(c_ref, s0, 0.05, 0.95, mid, gamma, aten_threads=THREADS)[0]      # round 5: with ATen's scalar tails restated -- exact
    bad = _digest_mismatch(live, f"helpers{seed}__shaped", [sh_a])
    assert bad is None, (seed, bad)
    sh_ref = sh_a
    sh = oracle.shape_depth_for_pop(c_ref, s0, 0.05, 0.95, mid, gamma)[0]
    assert np.max(np.abs(sh - sh_ref)) <= 1.2e-7, (seed, float(np.max(np.abs(sh - sh_ref))))
    # DOF + grade on a small eye: <= 1 LSB after truncation.  The oracle's dense DOF order (the render path's dof_dense_conv) and its grade
    # are the reference's bit for bit:
    tt = oracle.frame_to_tensor(bgr)
    dof_ref = oracle.apply_dof_dense(tt, d, focal, ms)
    out_ref = oracle.tensor_to_frame(oracle.color_grade(dof_ref, sat, con, bri))
    for nm, exact in (("dof", dof_ref), ("graded", out_ref)):
        bad = _digest_mismatch(live, f"helpers{seed}__{nm}", [exact])
        assert bad is None, (seed, nm, bad)
    # float domain: separable symmetric-pair FMA sums (oracle, HIP) vs the dense k x k conv of torchvision: summation noise only
    assert np.max(np.abs(oracle.apply_dof(tt, d, focal, ms) - dof_ref)) < 8e-7, (seed, ms)
    out = oracle.tensor_to_frame(oracle.color_grade(oracle.apply_dof(tt, d, focal, ms), sat, con, bri))
    mx, frac, _ = u8_diff_stats(out, out_ref)
    assert mx <= 1 and frac < 2e-2, (seed, mx, frac)     # separable FMA association vs torch's dense conv: 1-LSB truncation cliffs


def test_pixel_shift_full_size_1080p(live, oracle):
    """BASELINE configs[1] geometry against the reference: eye-size (540 x 960) tensors warped at 1080 x 1920 with the CLI
    defaults.  Tracker state, shift map and both eyes EXACT (torch-CPU's SLEEF pow / sigmoid and MKL sqrt are restated bit for bit)."""
    H, W = 1080, 1920
    bgr, d = synth.synth_frame(0, H // 2, W // 2)
    ft = oracle.frame_to_tensor(bgr)
    kw = dict(blur_ksize=9, feather_strength=10.0, use_subject_tracking=True, enable_floating_window=True, max_pixel_shift_percent=0.02,
              enable_edge_masking=True, enable_feathering=True)
    st = State()
    o = oracle.pixel_shift(ft, d[None], W, H, ShiftParams.defaults(10.0, -2.5, -5.0, **kw), st, want_shift=True)
    assert st.fw_prev_offset == float(live["full1080__prev_offset"])
    for nm, got in (("S", o["shift"]), ("L", o["left"]), ("R", o["right"])):
        assert _digest_mismatch(live, f"full1080_{nm}", [got]) is None, (nm, _digest_mismatch(live, f"full1080_{nm}", [got]))


def test_depth_handoff_normalisation_vs_reference(live, oracle):
    """a24, the per-frame min-max -> uint8 truncation of ``convert_depth_to_grayscale`` (core/render_depth.py:585-611) with the
    resize being the identity (transformers >= 4.4x hands ``predicted_depth`` back at the frame size): the
    oracle's hand-off equals the reference function bit for bit, incl. the degenerate-range and NaN frames it maps to zeros."""
    for i, (h, w, pred) in enumerate(C.handoff_cases()):
        exp = live[f"handoff{i}__u8"]
        got = oracle.depth_handoff(pred, h, w)
        assert np.array_equal(got, exp), (i, np.abs(got.astype(int) - exp.astype(int)).max())
        assert np.array_equal(oracle.depth_handoff(pred, h, w, invert=True), 255 - exp), i     # :1914-1915


def test_depth_handoff_with_bicubic_postprocess_vs_torch_and_reference(live, oracle):
    """The full a24 hand-off: transformers' post_process_depth_estimation (``F.interpolate(..., mode="bicubic",
    align_corners=False)`` to the frame size -- torch is the implementation) followed by the reference's
    ``convert_depth_to_grayscale``.  The oracle restates the bicubic taps in ATen's association: <= 1 LSB after the truncation, and
    only on truncation cliffs (the float planes agree to a few ULP)."""
    worst = 0.0
    for i, (H, W, pred) in enumerate(C.bicubic_cases()):
        exp = live[f"bicubic{i}__u8"]
        got = oracle.depth_handoff(pred, H, W)
        d = np.abs(got.astype(int) - exp.astype(int))
        worst = max(worst, float((d > 0).mean()))
        assert d.max() <= 1 and (d > 0).mean() < 5e-3, (i, d.max(), (d > 0).mean())
    print("hand-off vs torch bicubic + reference normalisation: worst differing fraction", worst)


@pytest.mark.parametrize("k", C.EVEN_BLUR_KS)
def test_even_blur_ksize_window(live, oracle, k):
    """avg_pool2d(kernel k, stride 1, padding k//2) of an EVEN k returns an (H+1) x (W+1) plane that feather_shift_edges crops to
    [:H, :W] (core/render_3d.py:355-369): the window of pixel x is x-k/2 .. x+k/2-1, zero padded, still divided by k*k."""
    bgr, d = synth.synth_frame(k, 40, 64)
    ft = oracle.frame_to_tensor(bgr)
    for H, W in ((40, 64), (80, 128)):
        oa = oracle.pixel_shift(ft, d[None], W, H, ShiftParams.defaults(10.0, -2.5, -5.0, blur_ksize=k, feather_strength=10.0, aten_threads=THREADS), State())
        for nm, exact in (("L", oa["left"]), ("R", oa["right"])):     # the N-thread ATen mode: the reference's eyes, bit for bit
            bad = _digest_mismatch(live, f"evenblur{k}_{H}_{nm}", [exact])
            assert bad is None, (k, H, W, nm, bad)
        o = oracle.pixel_shift(ft, d[None], W, H, ShiftParams.defaults(10.0, -2.5, -5.0, blur_ksize=k, feather_strength=10.0), State())
        for got, exp in ((o["left"], oa["left"]), (o["right"], oa["right"])):
            mx, frac, _ = u8_diff_stats(got, exp)
            assert mx <= 1 and frac < 8e-3, (k, H, W, mx, frac)


@pytest.mark.parametrize("seed", C.DOF_SLIDER_SEEDS)
def test_render_loop_dof_slider_and_formats_exact_on_untailed_planes(live, oracle, seed):
    """Round 4: the reference's ``render_sbs_3d`` loop vs the oracle over the WHOLE DOF slider (0.1 ... 5.0: Gaussians of 3 to 21 taps, the
    strengths where MKL's vsExp is not the rounded exponential among them) in every output format incl. VR, on 16:9 frame sizes whose planes
    are multiples of 32 elements (no ATen scalar tail: every float32 operator is the SLEEF / MKL vector path the DEFAULT mode computes with; on other sizes 3 to 11
    samples of a frame differ by up to 2 levels in that mode -- the N-thread ATen mode of round 5 restates the tails and is exact at any size,
    test_render_loop_any_size_exact_in_aten_mode).  Bar: EXACT."""
    from visiondepth3d_amd.params import render_kwargs_to_params
    sh, sw, n, kw = case = C.dof_slider_case(seed)
    _recorded(live, f"dof{seed}", case)
    got = _oracle_loop(oracle, sh, sw, n, render_kwargs_to_params(sw, sh, **kw))
    bad = _digest_mismatch(live, f"dof{seed}", got)
    assert bad is None, (seed, kw["output_format"], (sh, sw), kw["dof_strength"], bad)


@pytest.mark.parametrize("seed", C.EVERY_CONTROL_SEEDS)
def test_render_loop_every_control_exact_on_untailed_planes(live, oracle, seed):
    """The reference's ``render_sbs_3d`` loop vs the oracle with EVERY control the loop forwards drawn at random -- layer shifts, shift
    bound, zero-parallax strength, static / dynamic convergence, IPD factor, edge masking / feathering on and off, blur sizes 1 ... 13, feather
    strength, subject tracking, floating window, DOF, sharpening, colour grade, original-aspect preservation -- on 16:9 frames whose planes are
    multiples of 32 elements and whose eyes have H + W > 128 (where the DEFAULT mode, aten_sum_threads = 0, already is the reference's arithmetic; the two size-dependent
    ATen code paths outside that rule are restated in the N-thread ATen mode: test_render_loop_any_size_exact_in_aten_mode below), four
    rendered frames each (trackers, EMAs and the floating bar evolve).  Bar: EXACT.  (12 seeds run with the suite; offline runs of seeds
    0 ... 899 at the end of round 4: 900 of 900 exact.)"""
    from visiondepth3d_amd.params import render_kwargs_to_params
    sh, sw, n, kw = case = C.every_control_case(seed)
    _recorded(live, f"every{seed}", case)
    got = _oracle_loop(oracle, sh, sw, n, render_kwargs_to_params(sw, sh, **kw))
    bad = _digest_mismatch(live, f"every{seed}", got)
    assert bad is None, (seed, bad, kw)


@pytest.mark.parametrize("seed", C.BLANK_EXACT_SEEDS)
def test_blank_frame_loops_exact_on_untailed_planes(live, oracle, seed):
    """skip_blank_frames in the reference's loop (blackdetect list injected: blank frames keep the SOURCE frame through sharpen / fit / mux
    and freeze nothing -- the trackers still advance on them) on 16:9 frames, every format incl. output heights that differ from the source (72: eyes of
    64 x 36 that ATen resizes with its premultiplied-weight kernel -- restated since round 5, no size is skipped any more).  Bar: EXACT on every frame since round 5.  (Until round 4 rendered frames were allowed 4 samples /
    2 levels for ONE cause: the dynamic parallax scale rests on a float32 `torch.mean`, whose value is that of ATen's cascade sum -- and above
    32 K elements of its thread partition -- while the oracle used the correctly rounded exact sum; about one frame in 300 got a scale one ULP apart
    (seed 6, frame 1: 0.92083001 / 0.92083007).  The cascade sum is restated now (oracle vo_sum_aten_2d, vd3d_render_params::aten_sum_threads = the
    reference process's torch.get_num_threads()).)"""
    from visiondepth3d_amd.params import render_kwargs_to_params
    sh, sw, n, blank, kw = case = C.blank_exact_case(seed)
    _recorded(live, f"blankx{seed}", case)
    try:
        got = _oracle_loop(oracle, sh, sw, n, render_kwargs_to_params(sw, sh, aten_sum_threads=THREADS, **kw), blank)
    except NotImplementedError:
        pytest.skip("a fit the oracle does not restate")
    bad = _digest_mismatch(live, f"blankx{seed}", got)
    assert bad is None, (seed, blank, bad, kw)


@pytest.mark.parametrize("seed", C.ANY_SIZE_SEEDS)
def test_render_loop_any_size_exact_in_aten_mode(live, oracle, seed):
    """Round 5: NO SIZE RULE.  The reference's ``render_sbs_3d`` loop vs the oracle in the N-thread ATen mode (``aten_sum_threads`` = the
    reference process's torch.get_num_threads()) on source frames of ANY size and aspect -- odd widths and heights, 2:1 and 4:3 sources that the loop crops to
    16:9, thumbnails whose eyes ATen resizes with its premultiplied-weight kernel, planes whose pow / sigmoid tails go through libm -- with every control drawn at
    random, four rendered frames each.  Bar: EXACT.  (10 seeds with the suite; offline at the end of round 5: 1 760 of 1 760 at 1 .. 8 torch threads (tools/sweep_live_any_size.py,
    profiles/r05_parity_sweeps.md).)"""
    from visiondepth3d_amd.params import render_kwargs_to_params
    sh, sw, n, kw = case = C.any_size_loop_case(seed)
    _recorded(live, f"anysize{seed}", case)
    p = render_kwargs_to_params(sw, sh, aten_sum_threads=THREADS, **kw)
    got = _oracle_loop(oracle, sh, sw, n, p)
    bad = _digest_mismatch(live, f"anysize{seed}", got)
    assert bad is None, (seed, kw["output_format"], (sh, sw), (p.eye_h, p.eye_w), (p.warp_h, p.warp_w), bad)


@pytest.mark.parametrize("seed", C.SHIFT_1080P_SEEDS)
def test_pixel_shift_random_parameters_exact_at_1080p(live, oracle, seed):
    """``pixel_shift_cuda`` (B1) at REAL size -- a 1920x1080 warp from a 960x540 eye (Half-SBS geometry) or from a same-size plane -- with every
    keyword drawn at random (blur sizes 1 ... 13, shift bound 0.5 ... 6 % of the width, arbitrary ``depth_pop_gamma`` / ``depth_pop_mid`` /
    ``parallax_balance``: SLEEF ``pow`` with exponents no fixture has, convergence modes, masking / feathering on and off): the float32 shift
    map AND both eyes equal the reference's EXACTLY, and so does the floating-window tracker's state.  (4 seeds with the suite; seeds
    0 ... 323 offline at the end of round 4.)"""
    ih, iw, H, W, fg, mg, bg, kw = case = C.shift_1080p_case(seed)
    ref = _recorded(live, f"shift1080p{seed}", case)
    bgr, d = synth.synth_frame(seed, ih, iw)
    ft = oracle.frame_to_tensor(bgr)
    st = State()
    o = oracle.pixel_shift(ft, d[None], W, H, ShiftParams.defaults(fg, mg, bg, **kw), st, want_shift=True)
    assert st.fw_prev_offset == float(ref("prev_offset")), (seed, kw)
    for nm, got in (("S", o["shift"]), ("L", o["left"]), ("R", o["right"])):
        bad = _digest_mismatch(live, f"shift1080p{seed}_{nm}", [got])
        assert bad is None, (seed, nm, bad, kw)


@pytest.mark.parametrize("case", C.FEATHER0_CASES)
def test_render_loop_feather_strength_zero_exact(live, oracle, case):
    """Round 5: the GUI's own default configuration (VisionDepth3D.py:1405-1453: feather_strength 0.0, blur_ksize 1, Full-SBS) and its neighbours
    (feather 0 behind a 9 x 9 window, a NEGATIVE strength, other formats) against the reference's ``render_sbs_3d`` loop.  With a strength
    <= 0 ``feather_shift_edges`` (core/render_3d.py:328-374) is an exact no-op -- clamp(grad * fs, 0, 1) = 0, its window average 0, shifted * 1 +
    original * 0 -- which the HIP library exploits by not running the mask, window-sum and blend kernels at all (vd3d_api.hip::warp_stage_params;
    tests/test_hip_parity.py::test_feather_strength_zero_takes_the_exact_no_feather_warp compares that path with THIS oracle, which still goes the
    long way).  Bar: EXACT."""
    from visiondepth3d_amd.params import render_kwargs_to_params
    sh, sw, n, kw = drawn = C.feather0_case(case)
    _recorded(live, f"feather0{case}", drawn)
    got = _oracle_loop(oracle, sh, sw, n, render_kwargs_to_params(sw, sh, **kw))
    bad = _digest_mismatch(live, f"feather0{case}", got)
    assert bad is None, (case, kw["output_format"], (sh, sw), bad)
