"""Procedural INPUTS shared by the golden generator (make_golden.py, development container only) and the tests that replay
the fixtures (CPU oracle tests and the -m gpu tests): no reference import here, so this module travels to the GPU box."""
from __future__ import annotations

import numpy as np

from visiondepth3d_amd import synth


def heal_inputs(case):
    """Procedural inputs of the heal_missing_pixels goldens (shared with tests/test_oracle_vs_golden.py / the GPU test)."""
    H, W, shift, with_edge, hs = case
    f, d = synth.synth_frame(7, H, W)
    orig = (f[..., ::-1].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    warped = np.roll(orig, shift, axis=2).copy()
    warped[:, :, :abs(shift)] = 0.0                      # a disoccluded band, like a forward warp leaves behind
    edge = None
    if with_edge:
        gx = np.zeros_like(d); gx[:, 1:] = np.abs(d[:, 1:] - d[:, :-1])
        edge = np.clip(gx * np.float32(8.0), 0, 1).astype(np.float32)[None]
    return warped, orig, edge, hs


HEAL_CASES = [(96, 160, 3, True, 0.5), (96, 160, 5, False, 0.5), (54, 96, 2, True, 1.0), (33, 47, 1, True, 0.25)]


# ------------------------------------------------------------------------------------------
# The seeded sweeps of tests/test_oracle_vs_live_reference.py.  The reference's outputs for exactly these draws are recorded in
# live_sweeps.npz (make_golden.py live); the tests draw the same cases, check them against the recorded ones and replay the outputs.
# ------------------------------------------------------------------------------------------
LIVE_THREADS = 4   # torch intra-op threads of the reference process that recorded live_sweeps.npz (its N-thread ATen mode)

SHIFT_RANDOM_SEEDS = list(range(24)) + [101, 112, 159, 239, 248, 261, 310, 426, 594, 873]   # + the worst of a 940-seed offline sweep
SHIFT_UNTAILED_SEEDS = list(range(24))
LOOP_RANDOM_SEEDS = list(range(8)) + [114, 136, 151, 153]     # + the worst of a 60-seed offline sweep
LETTERBOX_SEEDS = list(range(6))
BLANK_RANDOM_SEEDS = [0, 1, 2, 3, 14, 36]                     # 14, 36: the worst of a 40-seed offline sweep (small-sigma DOF cliffs)
HELPER_SEEDS = list(range(10))
EVEN_BLUR_KS = [2, 4, 8, 12]
DOF_SLIDER_SEEDS = list(range(15))
EVERY_CONTROL_SEEDS = list(range(12))
BLANK_EXACT_SEEDS = list(range(12))
ANY_SIZE_SEEDS = list(range(10))
SHIFT_1080P_SEEDS = list(range(4))
FEATHER0_CASES = list(range(6))
HANDOFF_CASES = 12
BICUBIC_CASES = 8


def _shift_kw(rng, max_blur):
    return dict(blur_ksize=int(rng.integers(0, max_blur)) * 2 + 1, feather_strength=float(rng.uniform(0, 20)),   # odd k: even k changes the plane size in torch
                use_subject_tracking=bool(rng.integers(0, 2)), enable_floating_window=bool(rng.integers(0, 2)),
                max_pixel_shift_percent=float(rng.uniform(0.005, 0.06)), zero_parallax_strength=float(rng.uniform(0, 0.03)),
                enable_edge_masking=bool(rng.integers(0, 3) > 0), enable_feathering=bool(rng.integers(0, 3) > 0),
                convergence_strength=float([0.0, 3.0, -2.0][int(rng.integers(0, 3))]), enable_dynamic_convergence=bool(rng.integers(0, 2)),
                depth_pop_gamma=float(rng.uniform(0.6, 1.3)), depth_pop_mid=float(rng.uniform(0.35, 0.65)),
                parallax_balance=float(rng.uniform(0.5, 1.0)))


def shift_random_case(seed):
    """``pixel_shift_cuda`` at a small, odd size with every keyword drawn: (ih, iw, H, W, fg, mg, bg, kw)."""
    rng = np.random.default_rng(5000 + seed)
    ih, iw = int(rng.integers(24, 80)), int(rng.integers(32, 130))
    if rng.integers(0, 3) == 0:
        H, W = ih, iw
    else:
        H, W = int(rng.integers(24, 120)), int(rng.integers(32, 200))
    kw = _shift_kw(rng, 6)
    fg, mg, bg = float(rng.uniform(0, 30)), float(rng.uniform(-10, 5)), float(rng.uniform(-25, 0))
    return ih, iw, H, W, fg, mg, bg, kw


def shift_untailed_case(seed):
    """shift_random_case on planes whose element count is a multiple of 32 and >= 4200."""
    ih, iw, H, W, fg, mg, bg, kw = shift_random_case(seed)
    same = (H, W) == (ih, iw)
    W = (W + 31) // 32 * 32
    iw = W if same else (iw + 31) // 32 * 32
    if H * W < 4200:
        H = 4200 // W + 1
    if same:
        ih = H
    return ih, iw, H, W, fg, mg, bg, kw


def shift_1080p_case(seed):
    """``pixel_shift_cuda`` at 1920 x 1080 from a 960 x 540 eye or a same-size plane, every keyword drawn."""
    rng = np.random.default_rng(5000 + seed)
    same = bool(rng.integers(0, 2))
    H, W = 1080, 1920
    ih, iw = (H, W) if same else (540, 960)
    kw = _shift_kw(rng, 7)
    fg, mg, bg = float(rng.uniform(0, 30)), float(rng.uniform(-10, 5)), float(rng.uniform(-25, 0))
    return ih, iw, H, W, fg, mg, bg, kw


def _full_sbs_preserve(kw, sw, sh):
    kw.update(preserve_original_aspect=True, original_video_width=sw, original_video_height=sh)


def loop_random_case(seed):
    """(sh, sw, n, kw) of a render loop with random controls at a small size."""
    rng = np.random.default_rng(7000 + seed)
    fmt = ["Half-SBS", "Full-SBS", "Passive Interlaced", "Red-Cyan Anaglyph"][int(rng.integers(0, 4))]
    sh = int(rng.integers(40, 100)) // 2 * 2
    sw = int(round(sh * [16 / 9, 16 / 9, 4 / 3, 2.0][int(rng.integers(0, 4))])) // 2 * 2
    kw = dict(output_format=fmt, output_height=sh, fg_shift=float(rng.uniform(2, 20)), mg_shift=float(rng.uniform(-6, 2)),
              bg_shift=float(rng.uniform(-15, 0)), sharpness_factor=float(rng.uniform(0.0, 0.4)),
              dof_strength=float([0.0, 1.0, 2.0][int(rng.integers(0, 3))]), feather_strength=float(rng.uniform(0, 15)),
              blur_ksize=int(rng.integers(0, 5)) * 2 + 1, use_subject_tracking=bool(rng.integers(0, 2)),
              use_floating_window=bool(rng.integers(0, 2)), ipd_factor=float([1.0, 1.0, 1.2][int(rng.integers(0, 3))]),
              color_saturation=float(rng.uniform(0.9, 1.3)), color_contrast=float(rng.uniform(0.95, 1.1)),
              color_brightness=float(rng.uniform(-0.03, 0.03)))
    if fmt == "Full-SBS":
        _full_sbs_preserve(kw, sw, sh)
    return sh, sw, 4, kw


def letterbox_case(seed, labels):
    """(sh, sw, n, top, bottom, label, kw): letterbox bars x auto-crop x one of the reference's aspect-ratio ``labels`` (in its order)."""
    rng = np.random.default_rng(13000 + [29, 0, 1, 2, 3, 4][seed])
    fmt = ["Half-SBS", "Passive Interlaced", "Red-Cyan Anaglyph", "Full-SBS"][int(rng.integers(0, 4))]
    sh = int(rng.integers(60, 130)) // 2 * 2
    sw = int(round(sh * [16 / 9, 2.0, 4 / 3, 2.39][int(rng.integers(0, 4))])) // 2 * 2
    oh = [sh, int(rng.integers(40, 110)) // 2 * 2][int(rng.integers(0, 2))]
    label = labels[int(rng.integers(0, len(labels)))]
    top, bottom = int(rng.integers(0, sh // 5)), int(rng.integers(0, sh // 5))
    auto = bool(rng.integers(0, 2))
    kw = dict(output_format=fmt, output_height=oh, fg_shift=float(rng.uniform(2, 20)), mg_shift=float(rng.uniform(-6, 2)),
              bg_shift=float(rng.uniform(-15, 0)), sharpness_factor=float(rng.uniform(0.0, 0.4)),
              dof_strength=float([0.0, 2.0][int(rng.integers(0, 2))]), feather_strength=float(rng.uniform(0, 15)),
              blur_ksize=int(rng.integers(0, 5)) * 2 + 1, use_subject_tracking=bool(rng.integers(0, 2)),
              use_floating_window=bool(rng.integers(0, 2)), auto_crop_black_bars=auto)
    if fmt == "Full-SBS":
        _full_sbs_preserve(kw, sw, sh)
    return sh, sw, 4, top, bottom, label, kw


def blank_random_case(seed):
    """(sh, sw, n, blank, kw): skip_blank_frames with random controls and output heights."""
    rng = np.random.default_rng(11000 + seed)
    fmt = ["Half-SBS", "Full-SBS", "Passive Interlaced", "Red-Cyan Anaglyph"][int(rng.integers(0, 4))]
    sh = int(rng.integers(40, 100)) // 2 * 2
    sw = int(round(sh * [16 / 9, 16 / 9, 4 / 3, 2.0][int(rng.integers(0, 4))])) // 2 * 2
    oh = [sh, sh, int(rng.integers(40, 110)) // 2 * 2][int(rng.integers(0, 3))]
    kw = dict(output_format=fmt, output_height=oh, fg_shift=float(rng.uniform(2, 20)), mg_shift=float(rng.uniform(-6, 2)),
              bg_shift=float(rng.uniform(-15, 0)), sharpness_factor=float(rng.uniform(0.0, 0.4)),
              dof_strength=float([0.0, 1.0, 2.0][int(rng.integers(0, 3))]), feather_strength=float(rng.uniform(0, 15)),
              blur_ksize=int(rng.integers(0, 5)) * 2 + 1, use_subject_tracking=bool(rng.integers(0, 2)),
              use_floating_window=bool(rng.integers(0, 2)), ipd_factor=float([1.0, 0.0, 1.2][int(rng.integers(0, 3))]),
              skip_blank_frames=True)
    if fmt == "Full-SBS":
        _full_sbs_preserve(kw, sw, sh)
    n = 7
    blank = sorted(set(int(v) for v in rng.integers(0, n - 1, size=int(rng.integers(1, 4)))))
    return sh, sw, n, blank, kw


def helper_case(seed):
    """Inputs of the leaf-function checks: (h, w, quantised, gamma, mid, focal, max_sigma, sat, con, bri)."""
    rng = np.random.default_rng(9000 + seed)
    h, w = int(rng.integers(20, 70)), int(rng.integers(30, 110))
    gamma, mid = float(rng.uniform(0.6, 1.3)), float(rng.uniform(0.4, 0.6))
    focal, ms = float(rng.uniform(0.2, 0.8)), float([1.0, 2.0, 2.0, 3.0][int(rng.integers(0, 4))])
    sat, con, bri = float(rng.uniform(0.8, 1.4)), float(rng.uniform(0.9, 1.2)), float(rng.uniform(-0.05, 0.05))
    return h, w, seed % 3 == 0, gamma, mid, focal, ms, sat, con, bri


def helper_planes(seed, h, w, quantised):
    """The depth planes and the frame of helper_case(seed)."""
    d = synth.synth_frame(seed, h, w)[1]
    if quantised:     # a quantised plane (an 8-bit depth video): many ties in the order statistics
        d = (np.floor(d * 255) / 255).astype(np.float32)
    d2 = synth.synth_frame(seed + 50, h, w)[1]
    bgr = synth.synth_frame(seed + 7, h, w)[0]
    return d, d2, bgr


def handoff_cases():
    """Depth-net predictions for the hand-off normalisation: [(h, w, pred)], incl. a flat, a NaN and a near-flat plane."""
    rng = np.random.default_rng(77)
    out = []
    for i in range(HANDOFF_CASES):
        h, w = int(rng.integers(8, 70)), int(rng.integers(8, 90))
        pred = synth.synth_frame(i, h, w)[1].astype(np.float32) * np.float32(rng.uniform(0.01, 40.0)) + np.float32(rng.uniform(-5, 5))
        if i == 3:
            pred[:] = 2.5                      # range < 1e-6 -> zeros
        if i == 4:
            pred[h // 2, w // 2] = np.nan      # NaN -> zeros
        if i == 5:
            pred = (pred - pred.min()) * np.float32(1e-7) + 1.0   # range just below / above the 1e-6 gate
        out.append((h, w, pred))
    return out


def bicubic_cases():
    """Low-resolution predictions and the frame size they are resized to: [(H, W, pred)]."""
    rng = np.random.default_rng(78)
    out = []
    for i in range(BICUBIC_CASES):
        ph, pw = int(rng.integers(12, 40)), int(rng.integers(16, 60))
        H, W = int(ph * rng.uniform(1.0, 3.0)), int(pw * rng.uniform(1.0, 3.0))
        pred = synth.synth_frame(i, ph, pw)[1].astype(np.float32) * np.float32(rng.uniform(0.5, 20.0))
        out.append((H, W, pred))
    return out


def dof_slider_case(seed):
    """(sh, sw, n, kw): the whole DOF slider in every format incl. VR, 16:9 sizes whose planes are multiples of 32 elements."""
    rng = np.random.default_rng(9100 + seed)
    fmt = ["Half-SBS", "Full-SBS", "Passive Interlaced", "Red-Cyan Anaglyph", "VR"][seed % 5]
    sh, sw = [(108, 192), (144, 256), (108, 192)][int(rng.integers(0, 3))]
    dof = float(np.round(rng.uniform(0.1, 5.0), 1)) if seed % 3 else float([2.1, 4.2, 3.7, 0.7][seed // 3 % 4])
    kw = dict(output_format=fmt, output_height=sh, fg_shift=float(rng.uniform(2, 20)), mg_shift=float(rng.uniform(-6, 2)),
              bg_shift=float(rng.uniform(-15, 0)), sharpness_factor=float(rng.uniform(0.0, 0.4)), dof_strength=dof,
              feather_strength=float(rng.uniform(0, 15)), blur_ksize=int(rng.integers(0, 5)) * 2 + 1,
              use_subject_tracking=bool(rng.integers(0, 2)), use_floating_window=bool(rng.integers(0, 2)),
              color_saturation=float(rng.uniform(0.9, 1.3)), color_contrast=float(rng.uniform(0.95, 1.1)),
              color_brightness=float(rng.uniform(-0.03, 0.03)))
    if fmt == "Full-SBS":
        _full_sbs_preserve(kw, sw, sh)
    return sh, sw, 3, kw


def every_control_case(seed):
    """(sh, sw, n, kw) with every control the render loop forwards drawn at random, 16:9 untailed sizes."""
    rng = np.random.default_rng(9500 + seed)
    fmt = ["Half-SBS", "Full-SBS", "Passive Interlaced", "Red-Cyan Anaglyph", "VR"][int(rng.integers(0, 5))]
    sh, sw = [(108, 192), (144, 256)][int(rng.integers(0, 2))]
    kw = dict(output_format=fmt, output_height=sh, fg_shift=float(rng.uniform(0, 30)), mg_shift=float(rng.uniform(-10, 5)),
              bg_shift=float(rng.uniform(-25, 0)), sharpness_factor=float(rng.uniform(0.0, 0.6)),
              dof_strength=float([0.0, 1.0, 2.0, 2.0, 3.3][int(rng.integers(0, 5))]), feather_strength=float(rng.uniform(0, 20)),
              blur_ksize=int(rng.integers(0, 7)) * 2 + 1, use_subject_tracking=bool(rng.integers(0, 2)),
              use_floating_window=bool(rng.integers(0, 2)), max_pixel_shift_percent=float(rng.uniform(0.005, 0.06)),
              zero_parallax_strength=float(rng.uniform(0, 0.03)) if rng.integers(0, 2) else 0.0,
              enable_edge_masking=bool(rng.integers(0, 3) > 0), enable_feathering=bool(rng.integers(0, 3) > 0),
              convergence_strength=float([0.0, 3.0, -2.0][int(rng.integers(0, 3))]), enable_dynamic_convergence=bool(rng.integers(0, 2)),
              ipd_factor=float([1.0, 0.0, 1.2, 0.8][int(rng.integers(0, 4))]),
              color_saturation=float(rng.uniform(0.8, 1.4)), color_contrast=float(rng.uniform(0.9, 1.2)),
              color_brightness=float(rng.uniform(-0.05, 0.05)))
    if fmt == "Full-SBS" or rng.integers(0, 3) == 0:
        _full_sbs_preserve(kw, sw, sh)
    return sh, sw, 5, kw


def blank_exact_case(seed):
    """(sh, sw, n, blank, kw): skip_blank_frames on 16:9 untailed sizes, every format, output heights that differ from the source."""
    rng = np.random.default_rng(11500 + seed)
    fmt = ["Half-SBS", "Full-SBS", "Passive Interlaced", "Red-Cyan Anaglyph"][int(rng.integers(0, 4))]
    sh, sw = [(108, 192), (144, 256)][int(rng.integers(0, 2))]
    oh = [sh, sh, 72, 216][int(rng.integers(0, 4))]
    kw = dict(output_format=fmt, output_height=oh, fg_shift=float(rng.uniform(2, 20)), mg_shift=float(rng.uniform(-6, 2)),
              bg_shift=float(rng.uniform(-15, 0)), sharpness_factor=float(rng.uniform(0.0, 0.4)),
              dof_strength=float([0.0, 2.0, 2.0, 3.0][int(rng.integers(0, 4))]), feather_strength=float(rng.uniform(0, 15)),
              blur_ksize=int(rng.integers(0, 5)) * 2 + 1, use_subject_tracking=bool(rng.integers(0, 2)),
              use_floating_window=bool(rng.integers(0, 2)), ipd_factor=float([1.0, 0.0, 1.2][int(rng.integers(0, 3))]),
              skip_blank_frames=True)
    if fmt == "Full-SBS":
        _full_sbs_preserve(kw, sw, sh)
    n = 7
    blank = sorted(set(int(v) for v in rng.integers(0, n - 1, size=int(rng.integers(1, 4)))))
    return sh, sw, n, blank, kw


def any_size_loop_case(seed):
    """(sh, sw, n, kw): source frames of any size and aspect, every control drawn at random."""
    rng = np.random.default_rng(9700 + seed)
    fmt = ["Half-SBS", "Full-SBS", "Passive Interlaced", "Red-Cyan Anaglyph", "VR"][int(rng.integers(0, 5))]
    sh, sw = (int(rng.integers(20, 76)) * 2, int(rng.integers(30, 131)) * 2) if seed % 2 == 0 else (int(rng.integers(40, 150)), int(rng.integers(60, 260)))
    kw = dict(output_format=fmt, output_height=sh, fg_shift=float(rng.uniform(0, 30)), mg_shift=float(rng.uniform(-10, 5)),
              bg_shift=float(rng.uniform(-25, 0)), sharpness_factor=float(rng.uniform(0.0, 0.6)),
              dof_strength=float([0.0, 1.0, 2.0, 2.0, 3.3][int(rng.integers(0, 5))]), feather_strength=float(rng.uniform(0, 20)),
              blur_ksize=int(rng.integers(0, 7)) * 2 + 1, use_subject_tracking=bool(rng.integers(0, 2)),
              use_floating_window=bool(rng.integers(0, 2)), max_pixel_shift_percent=float(rng.uniform(0.005, 0.06)),
              enable_edge_masking=bool(rng.integers(0, 3) > 0), enable_feathering=bool(rng.integers(0, 3) > 0),
              convergence_strength=float([0.0, 3.0, -2.0][int(rng.integers(0, 3))]), enable_dynamic_convergence=bool(rng.integers(0, 2)),
              ipd_factor=float([1.0, 0.0, 1.2, 0.8][int(rng.integers(0, 4))]),
              color_saturation=float(rng.uniform(0.8, 1.4)), color_contrast=float(rng.uniform(0.9, 1.2)),
              color_brightness=float(rng.uniform(-0.05, 0.05)))
    if rng.integers(0, 3) == 0:
        _full_sbs_preserve(kw, sw, sh)
    return sh, sw, 4, kw


# the GUI's own default configuration (VisionDepth3D.py:1405-1453)
GUI_DEFAULTS = dict(output_format="Full-SBS", fg_shift=4.5, mg_shift=-1.5, bg_shift=-6.0, sharpness_factor=0.2, dof_strength=2.0,
                    feather_strength=0.0, blur_ksize=1, use_subject_tracking=True, use_floating_window=True, max_pixel_shift_percent=0.02,
                    auto_crop_black_bars=True, parallax_balance=0.8, zero_parallax_strength=0.01, enable_edge_masking=True,
                    enable_feathering=True, convergence_strength=0.0, enable_dynamic_convergence=True)


def feather0_case(case):
    """(sh, sw, n, kw): the GUI defaults (feather_strength 0) and their neighbours."""
    fmt, (sh, sw), fs, k = [("Full-SBS", (108, 192), 0.0, 1), ("Full-SBS", (144, 256), 0.0, 9), ("Half-SBS", (108, 192), 0.0, 1),
                            ("Passive Interlaced", (108, 192), -3.0, 5), ("Red-Cyan Anaglyph", (144, 256), 0.0, 3), ("VR", (108, 192), 0.0, 1)][case]
    kw = dict(GUI_DEFAULTS, output_format=fmt, output_height=sh, feather_strength=fs, blur_ksize=k)
    if fmt == "Full-SBS":
        _full_sbs_preserve(kw, sw, sh)
    return sh, sw, 4, kw
