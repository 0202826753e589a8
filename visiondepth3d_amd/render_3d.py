"""Host-side mirror of the reference's operator interface for the 2D->3D path
(``core/render_3d.py`` of VisionDepth3D): same function names, argument meaning and error behaviour,
backed by libvd3d_hip.so (hand-written HIP for gfx950).  PyTorch is used only for device memory and
streams.  There is no CPU fallback: without the HIP library / a GPU these functions raise.

    pixel_shift_cuda(frame_tensor, depth_tensor, width, height, fg, mg, bg, **kw)   # core/render_3d.py:561-712
    Renderer.render_frame(frame_bgr_u8, depth, params)                              # loop body :1227-1419
    render_clip(frames, depths, **render_sbs_3d kwargs)                             # loop :1194-1464 (first frame skipped)
    render_sbs_3d(input_path, depth_path, output_path, ...)                         # :933-985, video_io.py (capture / writer shell)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _abi, _lib
from ._abi import DEPTH_BGR_U8, DEPTH_F32, DEPTH_GRAY_U8, DT_BF16, DT_F16, DT_F32, FORMAT_IDS, FrameScalars, LetterboxParams, LetterboxState, RenderParams, ShiftParams, State
from .geometry import aspect_ratios  # noqa: F401  (re-exported like the reference module does)
from .params import reference_aten_threads, render_kwargs_to_params, shift_params_from_kwargs

torch_device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _ptr(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


class Renderer:
    """One vd3d_ctx on one GPU.  Holds the tracker state the reference keeps in module globals."""

    def __init__(self, device: int | torch.device | None = None, private_stream: bool = False, auto_order: bool = True):
        """``private_stream=False`` (default): every call enqueues on the stream that is current in PyTorch AT CALL TIME (the context
        is re-targeted when it changes), so tensor ops and vd3d kernels stay ordered like two torch ops.
        ``private_stream=True``: the context owns a non-blocking stream.  With ``auto_order`` (default) each call first orders that
        stream behind torch's current stream (event) and marks the tensors it touches with ``record_stream`` so the caching allocator
        does not recycle them early; consumers order themselves behind ``Renderer.stream`` (``ordered_after()``).  Callers that
        pipeline by hand (bench.py) pass ``auto_order=False`` and own all the events."""
        if not torch.cuda.is_available():
            raise RuntimeError("visiondepth3d_amd needs a ROCm GPU (MI355X); there is no CPU path")
        L = _lib.lib()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index or 0)
        self._L = L
        self._ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            # default: enqueue on torch's current stream so tensor ops and vd3d kernels stay ordered.  A private stream is taken from
            # PyTorch's stream pool and handed to the context as a caller-owned stream: tensors marked with record_stream() may outlive the
            # renderer, and the caching allocator records an event on that stream when they are freed -- a stream the context had created
            # and destroyed itself would be a dangling handle by then (segfault in hipEventRecord).
            self._own_stream = torch.cuda.Stream(device=self.device) if private_stream else None
            stream = C.c_void_p(self._own_stream.cuda_stream if private_stream else torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(L.vd3d_ctx_create(self.device.index, stream, C.byref(self._ctx)))
            self._private, self._auto_order = bool(private_stream), bool(auto_order)
            self._bound = None if private_stream else int(torch.cuda.current_stream(self.device).cuda_stream)
        self._stream_obj = None

    def _enter(self, *tensors):
        """Order this call against PyTorch's current stream (see __init__)."""
        cur = torch.cuda.current_stream(self.device)
        if not self._private:
            h = int(cur.cuda_stream)
            if h != self._bound:
                _lib.check(self._L.vd3d_ctx_set_stream(self._ctx, C.c_void_p(h)))
                self._bound = h
            return
        if self._auto_order:
            st = self.stream
            ev = torch.cuda.Event()
            ev.record(cur)
            st.wait_event(ev)
            for t in tensors:
                if t is not None and torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(st)

    def to_host(self, t: torch.Tensor) -> torch.Tensor:
        """``t.cpu()`` for a tensor this renderer produced: with a private stream the copy (which runs on torch's current stream)
        is first ordered behind the renderer's stream, so it cannot read an unfinished frame."""
        if self._private:
            self.ordered_after()
        return t.cpu()

    def ordered_after(self, stream=None):
        """Make ``stream`` (default: torch's current stream) wait for everything this renderer has enqueued so far."""
        st = self.stream
        tgt = stream or torch.cuda.current_stream(self.device)
        if int(tgt.cuda_stream) != int(st.cuda_stream):
            ev = torch.cuda.Event()
            ev.record(st)
            tgt.wait_event(ev)

    @property
    def stream(self) -> "torch.cuda.Stream":
        """The HIP stream this renderer enqueues on, as a torch stream object (for events / record_stream)."""
        if self._private:
            return self._own_stream
        ptr = self._L.vd3d_ctx_stream(self._ctx)
        if not ptr:
            return torch.cuda.default_stream(self.device)
        if self._stream_obj is None or int(self._stream_obj.cuda_stream) != int(ptr):
            self._stream_obj = torch.cuda.ExternalStream(int(ptr), device=self.device)
        return self._stream_obj

    @property
    def pixel_stream(self):
        """The second stream (overlapped pixel passes) as a torch stream object, or None before ``set_pixel_overlap(True)``.
        Consumers of the muxed frames (e.g. a D2H copy) order themselves behind it."""
        ptr = self._L.vd3d_ctx_pixel_stream(self._ctx)
        return torch.cuda.ExternalStream(int(ptr), device=self.device) if ptr else None

    @property
    def pixel_streams(self):
        """Every pixel stream created so far (``set_pixel_overlap(n)``), as torch stream objects."""
        out = []
        for k in range(4):
            ptr = self._L.vd3d_ctx_pixel_stream_k(self._ctx, k)
            if ptr:
                out.append(torch.cuda.ExternalStream(int(ptr), device=self.device))
        return out

    def close(self):
        if self._ctx:
            self._L.vd3d_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----
    def reset_state(self):
        _lib.check(self._L.vd3d_state_reset(self._ctx))

    def new_clip(self):
        _lib.check(self._L.vd3d_state_new_clip(self._ctx))

    def export_state(self) -> State:
        s = State()
        _lib.check(self._L.vd3d_state_export(self._ctx, C.byref(s)))
        return s

    def import_state(self, s: State):
        _lib.check(self._L.vd3d_state_import(self._ctx, C.byref(s)))

    def last_scalars(self) -> FrameScalars:
        f = FrameScalars()
        _lib.check(self._L.vd3d_last_scalars(self._ctx, C.byref(f)))
        return f

    def sync(self):
        _lib.check(self._L.vd3d_sync(self._ctx))

    def set_profiling(self, on: bool):
        _lib.check(self._L.vd3d_set_profiling(self._ctx, int(on)))

    def stage_ms(self, name: str) -> float:
        return float(self._L.vd3d_last_stage_ms(self._ctx, name.encode()))

    def stage_calls(self, name: str) -> int:
        return int(self._L.vd3d_stage_calls(self._ctx, name.encode()))

    # ---- B1 ----
    def pixel_shift(self, frame_tensor: torch.Tensor, depth_tensor: torch.Tensor, width, height,
                    params: ShiftParams, want_shift=False):
        """Device-resident form of pixel_shift_cuda: returns (left_u8, right_u8[, shift]) CUDA tensors."""
        W, H = int(width), int(height)
        if frame_tensor.dim() != 3 or frame_tensor.shape[0] != 3:
            raise AssertionError("frame_tensor must be [3,h,w]")
        if depth_tensor.dim() != 3 or depth_tensor.shape[0] != 1:
            raise AssertionError("Depth tensor must be [1, H, W]")
        if frame_tensor.shape[1:] != depth_tensor.shape[1:]:
            raise AssertionError("Shape mismatch")
        ft = frame_tensor.to(self.device, torch.float32).contiguous()
        dt = depth_tensor.to(self.device, torch.float32).contiguous()
        ih, iw = ft.shape[1:]
        L = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
        R = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
        S = torch.empty((1, H, W), dtype=torch.float32, device=self.device) if want_shift else None
        self._enter(ft, dt, L, R, S)
        _lib.check(self._L.vd3d_pixel_shift(self._ctx, _ptr(ft), _ptr(dt), ih, iw, W, H, C.byref(params), _ptr(L), _ptr(R),
                                            _ptr(S) if want_shift else None))
        return (L, R, S) if want_shift else (L, R)

    # ---- B2 ----
    def render_frame(self, frame_bgr: torch.Tensor, depth: torch.Tensor, params: RenderParams,
                     out: torch.Tensor | None = None, blank: bool = False) -> torch.Tensor:
        """One iteration of the render loop on device tensors.  frame_bgr: uint8 [h,w,3]; depth: float32 [h,w]
        (precomputed), uint8 [h,w,3] (depth-video frame) or uint8 [h,w].  ``blank``: the frame is in the
        skip_blank_frames set (core/render_3d.py:1278-1281): the source frame itself becomes both eyes."""
        if frame_bgr.dtype != torch.uint8 or frame_bgr.dim() != 3 or frame_bgr.shape[2] != 3:
            raise AssertionError("frame must be uint8 [h,w,3] BGR")
        if tuple(frame_bgr.shape[:2]) != (params.src_h, params.src_w):
            raise AssertionError("frame size does not match params.src_h/src_w")
        if depth.dtype == torch.float32 and depth.dim() == 2:
            fmt = DEPTH_F32
        elif depth.dtype == torch.uint8 and depth.dim() == 3 and depth.shape[2] == 3:
            fmt = DEPTH_BGR_U8
        elif depth.dtype == torch.uint8 and depth.dim() == 2:
            fmt = DEPTH_GRAY_U8
        else:
            raise AssertionError("depth must be float32 [h,w], uint8 [h,w,3] or uint8 [h,w]")
        if tuple(depth.shape[:2]) != (params.src_h, params.src_w):
            raise AssertionError("depth size does not match the frame")
        f = frame_bgr.to(self.device).contiguous()
        d = depth.to(self.device).contiguous()
        if out is None:
            out = torch.empty((params.out_h, params.out_w, 3), dtype=torch.uint8, device=self.device)
        fn = self._L.vd3d_render_frame_blank if blank else self._L.vd3d_render_frame
        self._enter(f, d, out)
        _lib.check(fn(self._ctx, _ptr(f), _ptr(d), fmt, C.byref(params), _ptr(out)))
        return out

    # ---- frame sharding, three-phase protocol (include/vd3d.h; orchestrated by visiondepth3d_amd.sharded) ----
    def _depth_fmt(self, depth):
        if depth.dtype == torch.float32 and depth.dim() == 2:
            return DEPTH_F32
        if depth.dtype == torch.uint8 and depth.dim() == 3 and depth.shape[2] == 3:
            return DEPTH_BGR_U8
        if depth.dtype == torch.uint8 and depth.dim() == 2:
            return DEPTH_GRAY_U8
        raise AssertionError("depth must be float32 [h,w], uint8 [h,w,3] or uint8 [h,w]")

    def shard_begin(self, params: RenderParams, n_slots: int):
        _lib.check(self._L.vd3d_shard_begin(self._ctx, C.byref(params), int(n_slots)))

    # measure / replay protocol (include/vd3d.h vd3d_shard2_*)
    def shard2_p0(self, frame, params: RenderParams, crop_out: torch.Tensor):
        f = frame.to(self.device).contiguous()
        self._enter(f, crop_out)
        _lib.check(self._L.vd3d_shard2_p0(self._ctx, _ptr(f), C.byref(params), _ptr(crop_out)))

    def shard2_set_crops(self, crops_all: torch.Tensor):
        cr = crops_all.to(self.device, torch.int32).contiguous()
        self._enter(cr)
        _lib.check(self._L.vd3d_shard2_set_crops(self._ctx, _ptr(cr), cr.numel() // 4))

    def shard2_p1(self, frame, depth, params: RenderParams, step_idx: int, slot: int, q_out: torch.Tensor):
        d = depth.to(self.device).contiguous()
        f = frame.to(self.device).contiguous()
        self._enter(f, d, q_out)
        _lib.check(self._L.vd3d_shard2_p1(self._ctx, _ptr(f), _ptr(d), self._depth_fmt(d), C.byref(params), int(step_idx), int(slot),
                                          _ptr(q_out)))

    MAX_BATCH = 16   # VD_MAX_BATCH of libvd3d_hip.so

    def shard2_p1_batch(self, frames, depths, params: RenderParams, step_idx0: int, slot0: int, q_out: torch.Tensor):
        """P1 of n consecutive own frames in two launches (``vd3d_shard2_p1_batch``); ``q_out``: float32 [n, 2] on the device."""
        n = len(frames)
        fs = [f.to(self.device).contiguous() for f in frames]
        ds = [d.to(self.device).contiguous() for d in depths]
        fmt = self._depth_fmt(ds[0])
        if any(self._depth_fmt(d) != fmt for d in ds):
            raise AssertionError("the depth planes of one batch share one format")
        if not q_out.is_contiguous() or q_out.numel() < 2 * n:
            raise AssertionError("q_out: contiguous float32 [n, 2]")
        self._enter(q_out, *fs, *ds)
        fp = (C.c_void_p * n)(*[f.data_ptr() for f in fs])
        dp = (C.c_void_p * n)(*[d.data_ptr() for d in ds])
        _lib.check(self._L.vd3d_shard2_p1_batch(self._ctx, fp, dp, fmt, C.byref(params), int(step_idx0), int(slot0), n, _ptr(q_out)))

    def shard2_p3_batch(self, slot0: int, step_idx0: int, n: int, params: RenderParams, m_out: torch.Tensor):
        """P3 of n consecutive own frames side by side (``vd3d_shard2_p3_batch``); ``m_out``: int64 [n, 4] on the device."""
        if not m_out.is_contiguous() or m_out.numel() < 4 * n:
            raise AssertionError("m_out: contiguous int64 [n, 4]")
        self._enter(m_out)
        _lib.check(self._L.vd3d_shard2_p3_batch(self._ctx, int(slot0), int(step_idx0), int(n), C.byref(params), _ptr(m_out)))

    def tdf_plane_export(self, params: RenderParams, out: torch.Tensor | None = None) -> torch.Tensor:
        """TemporalDepthFilter.prev_depth -> float32 [eye_h, eye_w] tensor (the chunk-boundary hand-off of a sharded clip)."""
        if out is None:
            out = torch.empty((params.eye_h, params.eye_w), dtype=torch.float32, device=self.device)
        self._enter(out)
        _lib.check(self._L.vd3d_tdf_plane_export(self._ctx, _ptr(out), params.eye_h, params.eye_w))
        return out

    def tdf_plane_import(self, plane: torch.Tensor, params: RenderParams, valid: bool = True):
        pl = plane.to(self.device, torch.float32).contiguous()
        self._enter(pl)
        _lib.check(self._L.vd3d_tdf_plane_import(self._ctx, _ptr(pl), params.eye_h, params.eye_w, 1 if valid else 0))

    def shard2_r1(self, q_all: torch.Tensor):
        q = q_all.to(self.device, torch.float32).contiguous()
        self._enter(q)
        _lib.check(self._L.vd3d_shard2_r1(self._ctx, _ptr(q), q.numel() // 2))

    def shard2_p3(self, slot: int, step_idx: int, params: RenderParams, m_out: torch.Tensor):
        self._enter(m_out)
        _lib.check(self._L.vd3d_shard2_p3(self._ctx, int(slot), int(step_idx), C.byref(params), _ptr(m_out)))

    def shard2_r2(self, m_all: torch.Tensor, own_slots, params: RenderParams, blank=None):
        n = len(own_slots)
        arr = (C.c_int * n)(*[int(v) for v in own_slots])
        bl = (C.c_uint8 * n)(*[1 if b else 0 for b in blank]) if blank is not None else None
        m = m_all.to(self.device, torch.int64).contiguous()
        self._enter(m)
        _lib.check(self._L.vd3d_shard2_r2(self._ctx, _ptr(m), arr, bl, n, C.byref(params)))

    def set_pixel_overlap(self, on: bool):
        """Run ``shard_pixels`` on a second stream of the context, behind the measurement chain of the next step
        (``vd3d_set_pixel_overlap``).  Outputs are complete after ``sync()`` / ``join_pixels()``."""
        _lib.check(self._L.vd3d_set_pixel_overlap(self._ctx, int(on)))   # True = one pixel stream, 2 .. 4 = that many (round-robin over frames)

    def join_pixels(self):
        """Order the context's stream after every outstanding overlapped pixel pass."""
        _lib.check(self._L.vd3d_join_pixels(self._ctx))

    def wait_pixels(self, slot: int):
        """Block the host until the overlapped pixel pass of ``slot`` (if any) has written its frame."""
        _lib.check(self._L.vd3d_wait_pixels(self._ctx, int(slot)))

    def shard_pixels(self, slot: int, params: RenderParams, out: torch.Tensor | None = None, blank_frame: torch.Tensor | None = None):
        """Pixel pass of an own frame; ``blank_frame``: the frame is in the skip_blank_frames set -> its source frame is both eyes."""
        if out is None:
            out = torch.empty((params.out_h, params.out_w, 3), dtype=torch.uint8, device=self.device)
        if blank_frame is not None:
            f = blank_frame.to(self.device, torch.uint8).contiguous()
            self._enter(out, f)
            _lib.check(self._L.vd3d_shard_pixels_blank(self._ctx, int(slot), _ptr(f), C.byref(params), _ptr(out)))
            ps = self.pixel_stream
            if ps is not None:   # the overlapped pass reads `f` on a stream torch does not know: keep its memory until that stream is done
                f.record_stream(ps)
                out.record_stream(ps)
            return out
        self._enter(out)
        _lib.check(self._L.vd3d_shard_pixels(self._ctx, int(slot), C.byref(params), _ptr(out)))
        if self._private and self._auto_order:
            for ps in self.pixel_streams:   # the pass may run on any of the pixel streams: `out` must outlive all of them
                out.record_stream(ps)
        return out

    def depth_handoff(self, pred: torch.Tensor, H: int, W: int, invert: bool = False, out: torch.Tensor | None = None, form: int = 0):
        """a24 on device: predictions float32 [B,ph,pw] -> uint8 depth planes [B,H,W] (bicubic + per-frame min-max).
        ``form``: 0 = the library's choice, 1 = the general kernel, 2 = the separable up-scaling kernel (vd3d_depth_handoff_form; the same bytes)."""
        p = pred.to(self.device, torch.float32).contiguous()
        if p.dim() == 2:
            p = p[None]
        B, ph, pw = p.shape
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        self._enter(p, out)
        _lib.check(self._L.vd3d_depth_handoff_form(self._ctx, _ptr(p), B, ph, pw, int(H), int(W), int(bool(invert)), _ptr(out), int(form)))
        return out

    # ---- tiled high-resolution depth (core/render_depth.py:102-194; tables from visiondepth3d_amd.depth_tiles) ----
    def tile_gather_cubic_u8(self, frames_bgr: torch.Tensor, origins: torch.Tensor, ch: int, cw: int, chs: int, cws: int,
                             out: torch.Tensor | None = None) -> torch.Tensor:
        """Apron crops of one shape group -> uint8 [n,chs,cws,3], each ``cv2.resize(crop, (cws, chs), INTER_CUBIC)`` (a copy at equal size).
        ``frames_bgr``: uint8 [B,H,W,3] (or [H,W,3]) on the device, pixels contiguous, any row / frame pitch; ``origins``: int32 device
        tensor [n,3] = (frame, y, x) of every ``ch x cw`` crop."""
        f = frames_bgr if frames_bgr.dim() == 4 else frames_bgr[None]
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3 or f.device != self.device:
            raise AssertionError("tile_gather_cubic_u8 takes uint8 [B,H,W,3] frames on the renderer's device")
        if f.stride(3) != 1 or f.stride(2) != 3:
            f = f.contiguous()
        o = origins.to(self.device, torch.int32).contiguous()
        if o.dim() != 2 or o.shape[1] != 3:
            raise AssertionError("tile_gather_cubic_u8: origins is int32 [n,3] = (frame, y, x)")
        B, H, W, _ = f.shape
        n = int(o.shape[0])
        if out is None:
            out = torch.empty((n, int(chs), int(cws), 3), dtype=torch.uint8, device=self.device)
        self._enter(f, o, out)
        _lib.check(self._L.vd3d_tile_gather_cubic_u8(self._ctx, _ptr(f), int(f.stride(1)), int(f.stride(0)), B, H, W, _ptr(o), n,
                                                     int(ch), int(cw), int(chs), int(cws), _ptr(out)))
        return out

    def tile_blend(self, pred_pool: torch.Tensor, pred_off: torch.Tensor, tile_tab: torch.Tensor, w_pool: torch.Tensor, n_frames: int,
                   tgt_h: int, tgt_w: int, tile: int, pad: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """Hann blend of the tile centres of ``n_frames`` frames in one launch -> float32 [n_frames,tgt_h,tgt_w] (vd3d_tile_blend_f32:
        the reference's accumulation order, no atomics).  ``pred_pool`` float32 1-D, ``pred_off`` int64 [n_frames * n_tiles],
        ``tile_tab`` int32 [n_tiles,8], ``w_pool`` float32 1-D: TilePlan.blend_tables / weight_pool on the device."""
        for t, dt in ((pred_pool, torch.float32), (pred_off, torch.int64), (tile_tab, torch.int32), (w_pool, torch.float32)):
            if t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise AssertionError("tile_blend: float32 pools, int64 offsets, int32 tile table, contiguous, on the renderer's device")
        if out is None:
            out = torch.empty((int(n_frames), int(tgt_h), int(tgt_w)), dtype=torch.float32, device=self.device)
        self._enter(pred_pool, pred_off, tile_tab, w_pool, out)
        _lib.check(self._L.vd3d_tile_blend_f32(self._ctx, _ptr(pred_pool), _ptr(pred_off), _ptr(tile_tab), _ptr(w_pool), int(n_frames),
                                               int(tgt_h), int(tgt_w), int(tile), int(pad), _ptr(out)))
        return out

    def depth_normalize_pclip(self, planes: torch.Tensor, invert: bool = False, pclip=(1.0, 99.0), out: torch.Tensor | None = None,
                              lo_hi: torch.Tensor | None = None) -> torch.Tensor:
        """_normalize_to_u8 (core/render_depth.py:173-193) per frame, without its final resize: float32 [B,H,W] -> uint8 [B,H,W] (numpy's
        percentiles by exact radix select, clip, truncation, optional ``255 -``).  ``lo_hi``: optional float32 [B,2] device tensor that
        receives the two percentiles."""
        p = planes.to(self.device, torch.float32).contiguous()
        if p.dim() == 2:
            p = p[None]
        B, H, W = p.shape
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        if lo_hi is not None and (lo_hi.dtype != torch.float32 or lo_hi.numel() < 2 * B or not lo_hi.is_contiguous() or lo_hi.device != self.device):
            raise AssertionError("depth_normalize_pclip: lo_hi is a contiguous float32 [B,2] tensor on the renderer's device")
        self._enter(p, out, lo_hi)
        _lib.check(self._L.vd3d_depth_normalize_pclip_u8(self._ctx, _ptr(p), B, H, W, float(pclip[0]), float(pclip[1]), int(bool(invert)),
                                                         _ptr(out), None if lo_hi is None else _ptr(lo_hi)))
        return out

    # ---- letterbox handling of the depth pass (core/render_depth.py:280-573,1919-1933; statement: visiondepth3d_amd.letterbox) ----
    def _lb_frames(self, frames: torch.Tensor, what: str) -> torch.Tensor:
        f = torch.as_tensor(frames)
        f = f if f.dim() == 4 else f[None]
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3:
            raise AssertionError(f"{what} takes uint8 [B,H,W,3] BGR frames")
        return f.to(self.device).contiguous()

    def _lb_planes(self, planes: torch.Tensor, what: str) -> torch.Tensor:
        p = torch.as_tensor(planes)
        p = p if p.dim() == 3 else p[None]
        if p.dtype != torch.uint8 or p.dim() != 3:
            raise AssertionError(f"{what} takes uint8 [B,H,W] planes")
        return p.to(self.device).contiguous()

    def letterbox_stats(self, frames_bgr: torch.Tensor, chain: bool = False) -> dict:
        """One statistics pass over uint8 [B,H,W,3] frames (vd3d_letterbox_stats): dict of device tensors ``row_mean`` / ``row_var`` float32
        [B,H], ``row_sat`` int32 [B,H] (integer sums of the HSV saturation), ``gray`` uint8 [B,H,W], ``hist`` int32 [B,64], ``mad_sum`` int64
        [B] (sum |gray_t - gray_(t-1)|; frame 0: against the tracker state's frame when ``chain``, else 0) and ``frame_mean`` float32 [B]."""
        f = self._lb_frames(frames_bgr, "letterbox_stats")
        B, H, W, _ = f.shape
        dev = self.device
        o = dict(row_mean=torch.empty((B, H), dtype=torch.float32, device=dev), row_var=torch.empty((B, H), dtype=torch.float32, device=dev),
                 row_sat=torch.empty((B, H), dtype=torch.int32, device=dev), gray=torch.empty((B, H, W), dtype=torch.uint8, device=dev),
                 hist=torch.empty((B, 64), dtype=torch.int32, device=dev), mad_sum=torch.empty((B,), dtype=torch.int64, device=dev),
                 frame_mean=torch.empty((B,), dtype=torch.float32, device=dev))
        self._enter(f, *o.values())
        _lib.check(self._L.vd3d_letterbox_stats(self._ctx, _ptr(f), B, H, W, int(bool(chain)), _ptr(o["row_mean"]), _ptr(o["row_var"]), _ptr(o["row_sat"]),
                                                _ptr(o["gray"]), _ptr(o["hist"]), _ptr(o["mad_sum"]), _ptr(o["frame_mean"])))
        return o

    def canny_u8(self, gray: torch.Tensor, low: int = 30, high: int = 90, want_counts: bool = False):
        """cv2.Canny(gray, low, high, apertureSize=3, L2gradient=True) per uint8 [B,H,W] plane -> uint8 edge maps [B,H,W]; with ``want_counts``
        also the int32 [B,H] edge pixels per row."""
        g = self._lb_planes(gray, "canny_u8")
        B, H, W = g.shape
        out = torch.empty_like(g)
        cnt = torch.empty((B, H), dtype=torch.int32, device=self.device) if want_counts else None
        self._enter(g, out, *(() if cnt is None else (cnt,)))
        _lib.check(self._L.vd3d_canny_u8(self._ctx, _ptr(g), B, H, W, int(low), int(high), _ptr(out), None if cnt is None else _ptr(cnt)))
        return (out, cnt) if want_counts else out

    def canny_hysteresis_u8(self, classes: torch.Tensor, want_counts: bool = False):
        """Canny's second half on a given class map uint8 [B,H,W] (0 none, 1 weak, 2 strong): 255 on every non-zero pixel 8-connected, through
        non-zero pixels, to a strong one."""
        c = self._lb_planes(classes, "canny_hysteresis_u8")
        B, H, W = c.shape
        out = torch.empty_like(c)
        cnt = torch.empty((B, H), dtype=torch.int32, device=self.device) if want_counts else None
        self._enter(c, out, *(() if cnt is None else (cnt,)))
        _lib.check(self._L.vd3d_canny_hysteresis_u8(self._ctx, _ptr(c), B, H, W, _ptr(out), None if cnt is None else _ptr(cnt)))
        return (out, cnt) if want_counts else out

    def letterbox_track(self, frames_bgr: torch.Tensor, h: int, min_change: int = 8, confirm_needed: int = 3, max_total: int | None = None,
                        cooldown_frames: int = 90, out: torch.Tensor | None = None) -> torch.Tensor:
        """LetterboxTracker.update for the frames of a step, in order, on the tracker state in the context -> int32 [B,2] (top, bottom) on
        the device; no host synchronisation.  ``max_total`` defaults to int(h * 0.35)."""
        f = self._lb_frames(frames_bgr, "letterbox_track")
        B, H, W, _ = f.shape
        p = LetterboxParams(int(min_change), int(confirm_needed), int(int(h) * 0.35) if max_total is None else int(max_total), int(cooldown_frames))
        if out is None:
            out = torch.empty((B, 2), dtype=torch.int32, device=self.device)
        self._enter(f, out)
        _lib.check(self._L.vd3d_letterbox_track(self._ctx, _ptr(f), B, H, W, C.byref(p), _ptr(out)))
        return out

    def letterbox_state_reset(self):
        """A new tracker: no bars (locked_zero), no previous frame."""
        self._enter()
        _lib.check(self._L.vd3d_letterbox_state_reset(self._ctx))

    def letterbox_state_export(self, with_frame: bool = False) -> dict:
        """The tracker state as a dict (synchronises).  ``with_frame``: also ``prev_hist`` (numpy int64 [64]) and ``prev_gray`` (device uint8
        [prev_h, prev_w]) of the frame the next update is compared with, when one is kept."""
        self._enter()
        s = LetterboxState()
        _lib.check(self._L.vd3d_letterbox_state_export(self._ctx, C.byref(s), None, None, 0))
        d = s.as_dict()
        if with_frame and s.have_prev:
            hist = (C.c_uint32 * 64)()
            g = torch.empty((s.prev_h, s.prev_w), dtype=torch.uint8, device=self.device)
            _lib.check(self._L.vd3d_letterbox_state_export(self._ctx, C.byref(s), hist, _ptr(g), g.numel()))
            self.sync()
            d["prev_hist"], d["prev_gray"] = np.asarray(list(hist), np.int64), g
        return d

    def letterbox_state_import(self, state: dict):
        """Restore a tracker state (``letterbox_state_export``'s dict; without ``prev_hist`` / ``prev_gray`` no previous frame is kept)."""
        s = LetterboxState()
        for k, _ in LetterboxState._fields_:
            setattr(s, k, int(state.get(k, 0)))
        g, hist = state.get("prev_gray"), state.get("prev_hist")
        if g is None or hist is None or not s.have_prev:
            s.have_prev = 0
            self._enter()
            _lib.check(self._L.vd3d_letterbox_state_import(self._ctx, C.byref(s), None, None))
            return
        g = g.to(self.device).contiguous()
        s.prev_h, s.prev_w = int(g.shape[0]), int(g.shape[1])
        h64 = (C.c_uint32 * 64)(*[int(v) for v in hist])
        self._enter(g)
        _lib.check(self._L.vd3d_letterbox_state_import(self._ctx, C.byref(s), h64, _ptr(g)))

    def depth_letterbox_fill(self, depth_u8: torch.Tensor, bars, out: torch.Tensor | None = None) -> torch.Tensor:
        """The letterbox handling behind the hand-off (core/render_depth.py:1919-1933) per uint8 [B,H,W] depth plane: squeezed into the picture
        rows with INTER_CUBIC, bars filled with the squeezed plane's median.  ``bars``: a (top, bottom) pair for every frame or an int32 [B,2]
        device tensor (LetterboxTracker.update's result: it never visits the host)."""
        d = self._lb_planes(depth_u8, "depth_letterbox_fill")
        B, H, W = d.shape
        if isinstance(bars, torch.Tensor):
            t = bars.to(self.device, torch.int32).contiguous()
            if t.numel() == 2:
                t, stride = t.reshape(2), 0
            elif tuple(t.shape) == (B, 2):
                stride = 2
            else:
                raise AssertionError("depth_letterbox_fill: bars is a (top, bottom) pair or an int32 [B,2] tensor")
        else:
            t, stride = torch.tensor([int(bars[0]), int(bars[1])], dtype=torch.int32, device=self.device), 0
        if out is None:
            out = torch.empty_like(d)
        self._enter(d, t, out)
        _lib.check(self._L.vd3d_depth_letterbox_fill_u8(self._ctx, _ptr(d), B, H, W, _ptr(t), stride, _ptr(out)))
        return out

    # ---- optional NV12 wire format at the frame I/O boundary ----
    def nv12_to_bgr(self, nv12: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8 [h*3/2, w] NV12 frame (h rows of Y, then h/2 rows of interleaved UV: what ``-pix_fmt nv12`` rawvideo carries) ->
        uint8 BGR [h,w,3]."""
        t = nv12.to(self.device).contiguous()
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] % 3 or t.shape[1] % 2:
            raise AssertionError("nv12_to_bgr takes a uint8 [h*3/2, w] frame with even h and w")
        h, w = int(t.shape[0]) * 2 // 3, int(t.shape[1])
        if h % 2:
            raise AssertionError("nv12_to_bgr takes a uint8 [h*3/2, w] frame with even h and w")
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
        self._enter(t, out)
        _lib.check(self._L.vd3d_nv12_to_bgr(self._ctx, _ptr(t), w, C.c_void_p(t.data_ptr() + h * w), w, h, w, _ptr(out)))
        return out

    def bgr_to_nv12(self, bgr: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8 BGR [h,w,3] -> uint8 [h*3/2, w] NV12 (the frame ``ffmpeg -f rawvideo -pix_fmt nv12`` reads from stdin)."""
        t = bgr.to(self.device).contiguous()
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] % 2 or t.shape[1] % 2:
            raise AssertionError("bgr_to_nv12 takes a uint8 [h,w,3] frame with even h and w")
        h, w = int(t.shape[0]), int(t.shape[1])
        if out is None:
            out = torch.empty((h * 3 // 2, w), dtype=torch.uint8, device=self.device)
        self._enter(t, out)
        _lib.check(self._L.vd3d_bgr_to_nv12(self._ctx, _ptr(t), h, w, _ptr(out), w, C.c_void_p(out.data_ptr() + h * w), w))
        return out

    # ---- uint8 glue shared by the depth hand-off (explicit inference size) and the up-scale stage ----
    def resize_cubic_u8(self, src: torch.Tensor, dh: int, dw: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """cv2.resize(src, (dw, dh), interpolation=cv2.INTER_CUBIC) for uint8 [h,w] / [h,w,3] tensors (core/render_depth.py:1917,
        core/merged_pipeline.py:260-264)."""
        if src.dtype != torch.uint8 or src.dim() not in (2, 3) or (src.dim() == 3 and src.shape[2] != 3):
            raise AssertionError("resize_cubic_u8 takes uint8 [h,w] or [h,w,3]")
        s = src.to(self.device).contiguous()
        cn = 1 if s.dim() == 2 else 3
        if out is None:
            out = torch.empty((int(dh), int(dw)) + ((3,) if cn == 3 else ()), dtype=torch.uint8, device=self.device)
        self._enter(s, out)
        _lib.check(self._L.vd3d_resize_cubic_u8(self._ctx, _ptr(s), int(s.shape[0]), int(s.shape[1]), cn, _ptr(out), int(dh), int(dw)))
        return out

    def resize_linear_u8(self, src: torch.Tensor, dh: int, dw: int) -> torch.Tensor:
        """cv2.resize(src, (dw, dh)) -- INTER_LINEAR, OpenCV's default -- for uint8 BGR [h,w,3] (format_3d_output's VR branch, core/render_3d.py:846-849)."""
        if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
            raise AssertionError("resize_linear_u8 takes uint8 [h,w,3]")
        s = src.to(self.device).contiguous()
        out = torch.empty((int(dh), int(dw), 3), dtype=torch.uint8, device=self.device)
        self._enter(s, out)
        _lib.check(self._L.vd3d_resize_linear_u8(self._ctx, _ptr(s), int(s.shape[0]), int(s.shape[1]), _ptr(out), int(dh), int(dw)))
        return out

    def format_3d_output(self, left: torch.Tensor, right: torch.Tensor, fmt) -> torch.Tensor:
        """format_3d_output(left, right, fmt) (core/render_3d.py:837-860) on the device: uint8 BGR eyes [h,w,3] -> the muxed frame (``fmt``: the
        reference's format string or a VD3D_FMT_* code; unknown strings fall back to side-by-side like the reference)."""
        code = fmt if isinstance(fmt, int) else FORMAT_IDS.get(str(fmt), 1)
        l_, r_ = left.to(self.device).contiguous(), right.to(self.device).contiguous()
        if l_.dtype != torch.uint8 or l_.dim() != 3 or l_.shape[2] != 3 or tuple(l_.shape) != tuple(r_.shape):
            raise AssertionError("format_3d_output takes two uint8 [h,w,3] eyes of one size")
        h, w = int(l_.shape[0]), int(l_.shape[1])
        shape = (1600, 2880, 3) if code == 2 else ((h, 2 * w, 3) if code in (0, 1) else (h, w, 3))
        out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self._enter(l_, r_, out)
        _lib.check(self._L.vd3d_format_3d_output(self._ctx, _ptr(l_), _ptr(r_), h, w, int(code), _ptr(out)))
        return out

    def resize_area_u8(self, src: torch.Tensor, dh: int, dw: int) -> torch.Tensor:
        """cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) for uint8 BGR [h,w,3] (core/merged_pipeline.py:246-248)."""
        if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
            raise AssertionError("resize_area_u8 takes uint8 [h,w,3]")
        s = src.to(self.device).contiguous()
        out = torch.empty((int(dh), int(dw), 3), dtype=torch.uint8, device=self.device)
        self._enter(s, out)
        _lib.check(self._L.vd3d_resize_area_u8(self._ctx, _ptr(s), int(s.shape[0]), int(s.shape[1]), _ptr(out), int(dh), int(dw)))
        return out

    def esr_preprocess(self, frame_bgr: torch.Tensor, y0=0, x0=0, h=None, w=None, dtype=torch.float32, channels_last=True):
        """preprocess_esr (core/merged_pipeline.py:219-223) of the [y0:y0+h, x0:x0+w] crop of a uint8 BGR frame: a [1,3,h,w] RGB
        tensor scaled by 1/255 (channels_last memory by default -- what the convolutions want)."""
        f = frame_bgr.to(self.device).contiguous()
        H, W = int(f.shape[0]), int(f.shape[1])
        h = H - y0 if h is None else int(h)
        w = W - x0 if w is None else int(w)
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
            raise AssertionError("esr_preprocess takes a uint8 [H,W,3] frame and a crop inside it")
        out = torch.empty((1, 3, h, w), dtype=dtype, device=self.device)
        if channels_last:
            out = out.contiguous(memory_format=torch.channels_last)
        self._enter(f, out)
        base = f.data_ptr() + (y0 * W + x0) * 3
        _lib.check(self._L.vd3d_esr_preprocess(self._ctx, {torch.float32: DT_F32, torch.bfloat16: DT_BF16, torch.float16: DT_F16}[dtype], C.c_void_p(base), 3 * W, h, w,
                                               int(bool(channels_last)), _ptr(out)))
        return out

    def esr_postprocess(self, pred: torch.Tensor, out: torch.Tensor | None = None, window=None, dst_yx=(0, 0)) -> torch.Tensor:
        """postprocess_esr (core/merged_pipeline.py:225-229): [1,3,h,w] RGB float -> uint8 BGR.  ``window`` = (cy, cx, ch, cw) of the
        prediction is written at ``dst_yx`` of ``out`` (the tile placement of _esrgan_tiled :266-284); default the whole prediction."""
        p = pred.to(self.device, torch.float32)
        if p.dim() != 4 or p.shape[0] != 1 or p.shape[1] != 3:
            raise AssertionError("esr_postprocess takes a [1,3,h,w] prediction")
        hwc = p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous()
        if not hwc:
            p = p.contiguous()
        h, w = int(p.shape[2]), int(p.shape[3])
        cy, cx, ch, cw = (0, 0, h, w) if window is None else [int(v) for v in window]
        if out is None:
            out = torch.empty((ch, cw, 3), dtype=torch.uint8, device=self.device)
        dy, dx = int(dst_yx[0]), int(dst_yx[1])
        OH, OW = int(out.shape[0]), int(out.shape[1])
        if out.dtype != torch.uint8 or not out.is_contiguous() or dy < 0 or dx < 0 or dy + ch > OH or dx + cw > OW:
            raise AssertionError("esr_postprocess: the window does not fit the output")
        self._enter(p, out)
        _lib.check(self._L.vd3d_esr_postprocess(self._ctx, _ptr(p), h, w, int(hwc), cy, cx, ch, cw,
                                                C.c_void_p(out.data_ptr() + (dy * OW + dx) * 3), 3 * OW))
        return out

    def conv3x3_c64(self, x: torch.Tensor, w_frag: torch.Tensor, bias: torch.Tensor, slope: torch.Tensor | None,
                    out: torch.Tensor | None = None) -> torch.Tensor:
        """One body layer of the up-scale network on the matrix cores (``vd3d_conv3x3_c64_f16``): ``x`` is a [1,64,H,W] fp16 tensor in
        channels_last memory; returns PReLU(conv3x3(x) + bias) in the same form.  ``w_frag``: ``upscale.conv_weight_fragments(weight)``."""
        if (x.dtype != torch.float16 or x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != 64
                or not x.is_contiguous(memory_format=torch.channels_last)):
            raise AssertionError("conv3x3_c64 takes a [1,64,H,W] fp16 tensor in channels_last memory")
        H, W = int(x.shape[2]), int(x.shape[3])
        if out is None:
            out = torch.empty_like(x, memory_format=torch.channels_last)
        self._enter(x, w_frag, bias, slope, out)
        _lib.check(self._L.vd3d_conv3x3_c64_f16(self._ctx, _ptr(x), H, W, _ptr(w_frag), _ptr(bias), _ptr(slope) if slope is not None else None,
                                                _ptr(out)))
        return out

    def conv3x3_head(self, x: torch.Tensor, w27: torch.Tensor, bias: torch.Tensor, slope: torch.Tensor | None) -> torch.Tensor:
        """Head layer of the compact up-scale networks (``vd3d_conv3x3_head_f16``): ``x`` [1,3,H,W] fp16 channels_last ->
        PReLU(conv3x3(x) + bias) as [1,64,H,W] fp16 channels_last.  ``w27``: ``upscale.head_weight_matrix(weight)`` (float32 [27,64])."""
        if (x.dtype != torch.float16 or x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != 3
                or not x.is_contiguous(memory_format=torch.channels_last)):
            raise AssertionError("conv3x3_head takes a [1,3,H,W] fp16 tensor in channels_last memory")
        H, W = int(x.shape[2]), int(x.shape[3])
        out = torch.empty((1, 64, H, W), dtype=torch.float16, device=self.device).contiguous(memory_format=torch.channels_last)
        self._enter(x, w27, bias, slope, out)
        _lib.check(self._L.vd3d_conv3x3_head_f16(self._ctx, _ptr(x), H, W, _ptr(w27), _ptr(bias), _ptr(slope) if slope is not None else None, _ptr(out)))
        return out

    def esr_tail(self, t: torch.Tensor, x: torch.Tensor, r: int) -> torch.Tensor:
        """pixel_shuffle(r) of the tail convolution's output ``t`` ([1,64,H,W] fp16 channels_last, channels >= 3 r^2 zero) + the nearest-neighbour
        up-sampled network input ``x`` ([1,3,H,W] fp16 channels_last) -> the float32 planar prediction [1,3,rH,rW] (``vd3d_esr_tail_f32``)."""
        H, W = int(x.shape[2]), int(x.shape[3])
        if t.dtype != torch.float16 or tuple(t.shape) != (1, 64, H, W) or not t.is_contiguous(memory_format=torch.channels_last):
            raise AssertionError("esr_tail takes the [1,64,H,W] fp16 channels_last output of the tail convolution")
        out = torch.empty((1, 3, H * r, W * r), dtype=torch.float32, device=self.device)
        self._enter(t, x, out)
        _lib.check(self._L.vd3d_esr_tail_f32(self._ctx, _ptr(t), _ptr(x), H, W, int(r), _ptr(out)))
        return out

    def conv3x3_dense(self, x: torch.Tensor, cin: int, w_frag: torch.Tensor, bias: torch.Tensor, cout: int, out: torch.Tensor, out_offset: int = 0,
                      slope: float = 1.0, r1: torch.Tensor | None = None, alpha: float = 1.0, r2: torch.Tensor | None = None, beta: float = 1.0,
                      up2: bool = False) -> torch.Tensor:
        """One convolution of the RRDB up-scale network on the matrix cores (``vd3d_conv3x3_dense_f16``, include/vd3d.h).  ``x``, ``out``, ``r1``, ``r2``
        are [1,C,H,W] fp16 tensors in channels_last memory, C being the pixel stride: the first ``cin`` channels of ``x`` are read, channels
        ``out_offset .. out_offset + cout`` of ``out`` are written -- ``out`` may be ``x`` itself when that slice lies behind ``cin`` (a dense block in
        one 192-channel buffer).  Result: ``leaky(conv + bias, slope)``, then ``* alpha + r1[:, :cout]`` and ``* beta + r2[:, :cout]`` where given, all in
        float32.  ``up2``: ``x`` has half the size of ``out`` and is read through a nearest x2 up-sampling.  ``w_frag``:
        ``upscale.dense_weight_fragments(weight)``; ``bias`` float32 [cout].  Returns ``out``."""
        for t in (x, out, r1, r2):
            if t is not None and (t.dtype != torch.float16 or t.dim() != 4 or t.shape[0] != 1 or not t.is_cuda
                                  or not t.is_contiguous(memory_format=torch.channels_last)):
                raise AssertionError("conv3x3_dense takes [1,C,H,W] fp16 tensors in channels_last memory")
        H, W = int(out.shape[2]), int(out.shape[3])
        if (int(x.shape[2]), int(x.shape[3])) != ((H // 2, W // 2) if up2 else (H, W)) or (up2 and (H % 2 or W % 2)):
            raise AssertionError("conv3x3_dense: input and output sizes do not match")
        for r in (r1, r2):
            if r is not None and (int(r.shape[2]), int(r.shape[3])) != (H, W):
                raise AssertionError("conv3x3_dense: a residual has the output's size")
        if (tuple(w_frag.shape) != (int(cin) // 32 * 18, int(cout) // 32, 64, 8) or w_frag.dtype != torch.float16 or not w_frag.is_contiguous()
                or bias.dtype != torch.float32 or bias.numel() != int(cout)):
            raise AssertionError("conv3x3_dense: w_frag is dense_weight_fragments(weight) of a [cout,cin,3,3] weight, bias float32 [cout]")
        self._enter(x, w_frag, bias, r1, r2, out)
        _lib.check(self._L.vd3d_conv3x3_dense_f16(self._ctx, _ptr(x), H, W, int(x.shape[1]), int(cin), _ptr(w_frag), _ptr(bias), int(cout),
                                                  float(slope), float(alpha), _ptr(r1) if r1 is not None else None, int(r1.shape[1]) if r1 is not None else 0,
                                                  float(beta), _ptr(r2) if r2 is not None else None, int(r2.shape[1]) if r2 is not None else 0,
                                                  int(bool(up2)), _ptr(out), int(out.shape[1]), int(out_offset)))
        return out

    def nhwc_f16_to_planar3(self, t: torch.Tensor) -> torch.Tensor:
        """Channels 0..2 of a [1,32,H,W] fp16 channels_last map -> the float32 planar prediction [1,3,H,W] (``vd3d_nhwc_f16_to_planar3_f32``): the tail
        behind the RRDB network's ``conv_last``, which runs on ``conv3x3_dense`` zero-padded to 32 output channels."""
        if (t.dtype != torch.float16 or t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 32 or not t.is_contiguous(memory_format=torch.channels_last)):
            raise AssertionError("nhwc_f16_to_planar3 takes a [1,32,H,W] fp16 tensor in channels_last memory")
        H, W = int(t.shape[2]), int(t.shape[3])
        out = torch.empty((1, 3, H, W), dtype=torch.float32, device=self.device)
        self._enter(t, out)
        _lib.check(self._L.vd3d_nhwc_f16_to_planar3_f32(self._ctx, _ptr(t), H, W, _ptr(out)))
        return out

    def add_weighted_u8(self, a: torch.Tensor, alpha: float, b: torch.Tensor, beta: float, gamma: float = 0.0) -> torch.Tensor:
        """cv2.addWeighted on uint8 tensors of one shape (blend_images, core/merged_pipeline.py:231-236)."""
        a = a.to(self.device).contiguous()
        b = b.to(self.device).contiguous()
        if a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.shape != b.shape:
            raise AssertionError("add_weighted_u8 takes two uint8 tensors of one shape")
        out = torch.empty_like(a)
        self._enter(a, b, out)
        _lib.check(self._L.vd3d_add_weighted_u8(self._ctx, _ptr(a), float(alpha), _ptr(b), float(beta), float(gamma), a.numel(), _ptr(out)))
        return out

    def heal_missing_pixels(self, warped_frame, original_frame, edge_mask=None, heal_strength=0.5) -> torch.Tensor:
        """a23 (core/render_3d.py:431-459) on device: float32 [3,H,W] tensors (+ optional [1,H,W] edge mask) -> healed [3,H,W]."""
        if warped_frame.dim() != 3 or warped_frame.shape[0] != 3 or warped_frame.shape != original_frame.shape:
            raise AssertionError("warped_frame and original_frame must both be [3,H,W]")
        w = warped_frame.to(self.device, torch.float32).contiguous()
        o = original_frame.to(self.device, torch.float32).contiguous()
        H, W = int(w.shape[1]), int(w.shape[2])
        e = None
        if edge_mask is not None:
            if edge_mask.numel() != H * W:
                raise AssertionError("edge_mask must be [1,H,W]")
            e = edge_mask.to(self.device, torch.float32).contiguous()
        out = torch.empty_like(w)
        self._enter(w, o, e, out)
        _lib.check(self._L.vd3d_heal_missing_pixels(self._ctx, _ptr(w), _ptr(o), _ptr(e) if e is not None else None, H, W,
                                                    float(heal_strength), _ptr(out)))
        return out

    def finish_frame(self, left, right, depth_norm, params: RenderParams, focal_depth, bar_width=0, bar_side=0):
        out = torch.empty((params.out_h, params.out_w, 3), dtype=torch.uint8, device=self.device)
        dn = depth_norm.to(self.device, torch.float32).contiguous()
        eh, ew = dn.shape[-2:]
        left, right = left.to(self.device).contiguous(), right.to(self.device).contiguous()
        self._enter(left, right, dn, out)
        _lib.check(self._L.vd3d_finish_frame(self._ctx, _ptr(left), _ptr(right), _ptr(dn), eh, ew,
                                             C.byref(params), float(focal_depth), int(bar_width), int(bar_side), _ptr(out)))
        return out

    # ---- exact reductions (test / diagnostic entry points) ----
    def torch_math(self, op: str, x: torch.Tensor, param: float = 0.0) -> torch.Tensor:
        """torch.pow(x, param) / torch.sigmoid(x) / torch.sqrt(x) with the values torch's CPU kernels give (SLEEF / MKL VML), as the
        chain's kernels evaluate them (core/render_3d.py:517, 620, 209, 206)."""
        t = x.to(self.device, torch.float32).contiguous()
        o = torch.empty_like(t)
        self._enter(t, o)
        _lib.check(self._L.vd3d_torch_math(self._ctx, {"pow": 0, "sigmoid": 1, "sqrt": 2}[op], _ptr(t), float(param), _ptr(o), t.numel()))
        return o

    def torch_math_aten(self, op: str, x: torch.Tensor, param: float = 0.0, aten_threads: int = 0) -> torch.Tensor:
        """``torch_math`` for "pow" / "sigmoid" with ATen's scalar tails for a torch process of ``aten_threads`` intra-op threads (libm on the last
        ``len mod 32`` elements of every thread's chunk; < 0: on every element) -- include/vd3d.h vd3d_torch_math_aten."""
        t = x.to(self.device, torch.float32).contiguous()
        o = torch.empty_like(t)
        self._enter(t, o)
        _lib.check(self._L.vd3d_torch_math_aten(self._ctx, {"pow": 0, "sigmoid": 1}[op], _ptr(t), float(param), _ptr(o), t.numel(), int(aten_threads)))
        return o

    def quantiles(self, plane: torch.Tensor, qs):
        p = plane.to(self.device, torch.float32).contiguous()
        q = (C.c_float * len(qs))(*[float(np.float32(v)) for v in qs])
        o = (C.c_float * len(qs))()
        self._enter(p)
        _lib.check(self._L.vd3d_quantiles(self._ctx, _ptr(p), p.numel(), q, len(qs), o))
        return [float(v) for v in o]

    def subject_depth(self, plane: torch.Tensor) -> float:
        p = plane.to(self.device, torch.float32).contiguous()
        H, W = p.shape[-2:]
        o = C.c_float()
        self._enter(p)
        _lib.check(self._L.vd3d_subject_depth(self._ctx, _ptr(p), H, W, C.byref(o)))
        return float(o.value)

    @staticmethod
    def _dt(dtype) -> int:
        if dtype == torch.float32:
            return DT_F32
        if dtype == torch.bfloat16:
            return DT_BF16
        raise TypeError(f"depth-net glue kernels are built for float32 and bfloat16, not {dtype}")

    def depth_preprocess(self, frames_bgr: torch.Tensor, th: int, tw: int, mean, std, dtype=torch.float32, form: int = 0) -> torch.Tensor:
        """DPT image-processor front end fused in one launch: uint8 BGR [B,H,W,3] -> ``dtype`` tensor of logical shape
        [B,3,th,tw] in channels_last memory (antialiased bicubic resize, 1/255, ImageNet normalise).
        ``form``: 0 = the library's choice, 1 = the general tile kernel, 2 = the strip kernel for down-scaling (vd3d_depth_preprocess_form; the same bits)."""
        f = frames_bgr.to(self.device, torch.uint8).contiguous()
        B, H, W, _ = f.shape
        out = torch.empty((B, th, tw, 3), dtype=dtype, device=self.device)
        m = (C.c_float * 3)(*[float(v) for v in mean]); s = (C.c_float * 3)(*[float(v) for v in std])
        self._enter(f, out)
        _lib.check(self._L.vd3d_depth_preprocess_form(self._ctx, _ptr(f), B, H, W, int(th), int(tw), m, s, self._dt(dtype), _ptr(out), int(form)))
        return out.permute(0, 3, 1, 2)   # NCHW view of NHWC storage == torch.channels_last

    pil_route = None   # where the last resize_pil_bicubic_u8 / depth_preprocess_pil ran: "kernel" | "statement"

    def resize_pil_bicubic_u8(self, frames: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """``Image.fromarray(f).resize((w, h), Image.BICUBIC)`` of every uint8 [B,H,W,3] frame (a single [H,W,3] frame comes back as one), on the
        device, the same bytes (vd3d_resize_pil_bicubic_u8).  A geometry past the kernel's tap budget runs the integer statement of the same operator
        (``pil_resample.resize``) on the device instead: the same values.  ``pil_route`` says which of the two ran."""
        f = frames.to(self.device)
        if f.dtype != torch.uint8 or f.dim() not in (3, 4) or f.shape[-1] != 3:
            raise TypeError("resize_pil_bicubic_u8 takes uint8 [B,H,W,3] frames")
        single = f.dim() == 3
        f = (f[None] if single else f).contiguous()
        B, H, W, _ = f.shape
        out = torch.empty((B, int(h), int(w), 3), dtype=torch.uint8, device=self.device)
        self._enter(f, out)
        rc = self._L.vd3d_resize_pil_bicubic_u8(self._ctx, _ptr(f), B, H, W, _ptr(out), int(h), int(w))
        if rc == -4:   # VD3D_E_UNSUPPORTED
            from . import pil_resample
            out = pil_resample.resize(f, int(w), int(h))
            self.pil_route = "statement"
        else:
            _lib.check(rc)
            self.pil_route = "kernel"
        return out[0] if single else out

    def depth_preprocess_pil(self, frames_bgr: torch.Tensor, th: int, tw: int, mean, std, dtype=torch.float32, inference_size=None) -> torch.Tensor:
        """The reference's own input path, exact: uint8 BGR [B,H,W,3] -> what ``DPTImageProcessor`` makes of the PIL image (Pillow's 8-bit bicubic
        resize to (th, tw), 1/255, normalise), ``dtype`` tensor of logical shape [B,3,th,tw] in channels_last memory, in one launch
        (vd3d_depth_preprocess_pil; stage ``depth_prep_pil``).  ``inference_size`` = (W', H'): ``img.resize(inference_size, Image.BICUBIC)`` first, a
        second launch.  Past the tap budget the integer statement (``pil_resample.pixel_values``) runs on the device; ``pil_route`` says which ran."""
        f = frames_bgr.to(self.device)
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3:
            raise TypeError("depth_preprocess_pil takes uint8 [B,H,W,3] BGR frames")
        f = f.contiguous()
        B, H, W, _ = f.shape
        mw, mh = (0, 0) if inference_size is None else (int(inference_size[0]), int(inference_size[1]))
        if inference_size is not None and (mw < 1 or mh < 1):
            raise ValueError("inference_size is (W', H') with positive sides")
        out = torch.empty((B, int(th), int(tw), 3), dtype=dtype, device=self.device)
        m = (C.c_float * 3)(*[float(v) for v in mean]); s = (C.c_float * 3)(*[float(v) for v in std])
        self._enter(f, out)
        rc = self._L.vd3d_depth_preprocess_pil(self._ctx, _ptr(f), B, H, W, mh, mw, int(th), int(tw), m, s, self._dt(dtype), _ptr(out))
        if rc == -4:   # VD3D_E_UNSUPPORTED
            from . import pil_resample
            out = pil_resample.pixel_values(f, int(th), int(tw), mean, std, dtype, inference_size)
            self.pil_route = "statement"
        else:
            _lib.check(rc)
            self.pil_route = "kernel"
        return out.permute(0, 3, 1, 2)   # NCHW view of NHWC storage == torch.channels_last

    def add_layernorm(self, x: torch.Tensor, y, norm: torch.nn.LayerNorm):
        """(x + y, LayerNorm(x + y)) for contiguous float32 / bf16 [..., cols] tensors in one launch; y=None -> (x, LayerNorm(x))."""
        cols = x.shape[-1]
        rows = x.numel() // cols
        out_n = torch.empty_like(x)
        out_s = torch.empty_like(x) if y is not None else x
        self._enter(x, y, out_s, out_n)
        _lib.check(self._L.vd3d_add_layernorm(self._ctx, self._dt(x.dtype), _ptr(x), _ptr(y) if y is not None else None, _ptr(norm.weight),
                                              _ptr(norm.bias), float(norm.eps), rows, cols, _ptr(out_s) if y is not None else None, _ptr(out_n)))
        return out_s, out_n

    X3_MODES = {"bf16x3": 0, "fp16x2": 1}
    TILE_CONVS = {("bf16x3", 1): "x3", ("bf16x3", 2): "s2_x3", ("fp16x2", 1): "s1_x2", ("fp16x2", 2): "s2_x2"}   # (mode, stride) -> vd3d_conv3x3_<family>

    def gemm_x3_pack(self, weight: torch.Tensor, mode: str = "bf16x3") -> torch.Tensor:
        """Split + pack a float32 Linear weight [N, K] once for ``linear_x3`` in ``mode`` (include/vd3d.h vd3d_gemm_x3_pack_weights); returns the opaque image (uint8)."""
        w = weight.detach().to(self.device, torch.float32).contiguous()
        N, K = w.shape
        m = self.X3_MODES[mode]
        nb = int(self._L.vd3d_gemm_x3_weight_bytes(N, K, m))
        if nb < 0:
            raise NotImplementedError(f"gemm_x3: K = {K} is not a positive multiple of 16")
        img = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._enter(w, img)
        _lib.check(self._L.vd3d_gemm_x3_pack_weights(self._ctx, _ptr(w), N, K, m, _ptr(img)))
        return img

    def linear_x3(self, x: torch.Tensor, w_image: torch.Tensor, N: int, bias: torch.Tensor | None = None, gelu: bool = False, mode: str = "bf16x3") -> torch.Tensor:
        """F.linear(x, W, bias) (+ exact GELU) for contiguous float32 x [..., K] with W given as ``gemm_x3_pack(W, mode)``: split-operand MFMA GEMM, float32 accumulation."""
        K = x.shape[-1]
        M = x.numel() // K
        out = torch.empty(x.shape[:-1] + (int(N),), dtype=torch.float32, device=x.device)
        self._enter(x, w_image, bias, out)
        _lib.check(self._L.vd3d_gemm_x3(self._ctx, _ptr(x), M, K, _ptr(w_image), int(N), self.X3_MODES[mode], _ptr(bias) if bias is not None else None,
                                        1 if gelu else 0, _ptr(out)))
        return out

    def attention_x3(self, qkv: torch.Tensor, n_heads: int, scale: float, mode: str = "bf16x3") -> torch.Tensor:
        """softmax(q k^T * scale) v for the contiguous float32 output ``qkv`` [B, T, 3 * H * 64] of a fused QKV linear (q / k / v = the three [H, 64] blocks of
        a token) -> [B, T, H * 64] float32; both products as split-operand MFMA work (include/vd3d.h vd3d_attention_x3)."""
        B, T, C3 = qkv.shape
        D = C3 // (3 * n_heads)
        if qkv.dtype != torch.float32 or not qkv.is_contiguous() or D * 3 * n_heads != C3:
            raise AssertionError("qkv must be contiguous float32 [B, T, 3 * H * D]")
        m = self.X3_MODES[mode]
        nb = int(self._L.vd3d_attention_x3_workspace_bytes(B, T, n_heads, D, m))
        if nb < 0:
            raise NotImplementedError(f"attention_x3: head size {D} not built")
        ws = getattr(self, "_attn_ws", None)
        if ws is None or ws.numel() < nb:   # one workspace per renderer, grown on demand (calls are ordered on the renderer's stream)
            ws = self._attn_ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        out = torch.empty((B, T, n_heads * D), dtype=torch.float32, device=self.device)
        self._enter(qkv, ws, out)
        _lib.check(self._L.vd3d_attention_x3(self._ctx, _ptr(qkv), B, T, n_heads, D, float(scale), m, _ptr(ws), ws.numel(), _ptr(out)))
        return out

    def attention_f32(self, qkv: torch.Tensor, n_heads: int, scale: float, form: int = 0) -> torch.Tensor:
        """softmax(q k^T * scale) v for the contiguous float32 output ``qkv`` [B, T, 3 * H * 64] of a fused QKV linear -> [B, T, H * 64] float32, in exact
        float32: both products on the float32-input matrix cores, float32 online softmax (include/vd3d.h vd3d_attention_f32).  No workspace.
        ``form``: waves per workgroup, 4 or 8, or 0 = the library's choice (vd3d_attention_f32_form; the same bits either way)."""
        B, T, C3 = qkv.shape
        D = C3 // (3 * n_heads)
        if qkv.dtype != torch.float32 or not qkv.is_contiguous() or D * 3 * n_heads != C3:
            raise AssertionError("qkv must be contiguous float32 [B, T, 3 * H * D]")
        if D != 64:
            raise NotImplementedError(f"attention_f32: head size {D} not built")
        out = torch.empty((B, T, n_heads * D), dtype=torch.float32, device=self.device)
        self._enter(qkv, out)
        _lib.check(self._L.vd3d_attention_f32_form(self._ctx, _ptr(qkv), B, T, n_heads, D, float(scale), _ptr(out), int(form)))
        return out

    def _conv3x3_pack(self, fam: str, weight: torch.Tensor):
        """The pack of every vd3d_conv3x3_<fam> (_lib.py: one signature): the opaque image, or ``None`` where the kernel is not 3 x 3 or the shape is not built."""
        w = weight.detach().to(self.device, torch.float32).contiguous()
        Cout, Cin, kh, kw = w.shape
        nb = int(getattr(self._L, f"vd3d_conv3x3_{fam}_weight_bytes")(Cin, Cout)) if (kh, kw) == (3, 3) else -1
        if nb < 0:
            return None
        img = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._enter(w, img)
        _lib.check(getattr(self._L, f"vd3d_conv3x3_{fam}_pack_weights")(self._ctx, _ptr(w), Cin, Cout, _ptr(img)))
        return img

    def _conv3x3(self, fam: str, x: torch.Tensor, w_image: torch.Tensor, Cout: int) -> torch.Tensor:
        """The run of every vd3d_conv3x3_<fam>: padding 1, stride 2 for the ``s2_`` families (output (H+1)//2 x (W+1)//2), else stride 1."""
        B, Cin, H, W = x.shape
        if x.dtype != torch.float32 or not x.is_contiguous(memory_format=torch.channels_last):
            raise AssertionError(f"conv3x3_{fam}: float32 channels_last input")
        Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if fam.startswith("s2_") else (H, W)
        out = torch.empty((B, int(Cout), Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        self._enter(x, w_image, out)
        _lib.check(getattr(self._L, f"vd3d_conv3x3_{fam}")(self._ctx, _ptr(x), B, H, W, Cin, _ptr(w_image), int(Cout), _ptr(out)))
        return out

    def conv3x3_tile_pack(self, weight: torch.Tensor, mode: str = "bf16x3", stride: int = 1):
        """Pack a float32 3 x 3 convolution weight [Cout, Cin, 3, 3] for ``conv3x3_tile`` in ``mode`` at ``stride`` (``TILE_CONVS``: the 8 x 32 tile kernel's four
        members); ``None`` when the member does not build the shape.  Goes through the member's public method, looked up per call, like ``conv3x3_tile``."""
        return getattr(self, f"conv3x3_{self.TILE_CONVS[mode, stride]}_pack")(weight)

    def conv3x3_tile(self, x: torch.Tensor, w_image: torch.Tensor, Cout: int, mode: str = "bf16x3", stride: int = 1) -> torch.Tensor:
        """F.conv2d(x, W, None, stride, padding 1) for a float32 channels_last tensor with W given as ``conv3x3_tile_pack(W, mode, stride)``: the call of the
        member's public method, looked up per call (a wrapper put on ``conv3x3_x3`` to count its calls sees DepthPipe's)."""
        return getattr(self, f"conv3x3_{self.TILE_CONVS[mode, stride]}")(x, w_image, Cout)

    EPI_RELU_IN, EPI_RELU = 1, 2   # include/vd3d.h VD3D_EPI_*

    def conv3x3_epi(self, x: torch.Tensor, w_image: torch.Tensor, Cout: int, mode: str = "bf16x3", bias=None, r1=None, r2=None, relu_in: bool = False,
                    relu: bool = False, want_relu_copy: bool = False):
        """``bias_act(conv3x3_tile([relu](x), w_image, Cout, mode), bias, r1, r2, relu, want_relu_copy)`` as ONE launch with the same bits
        (``vd3d_conv3x3_epi``, include/vd3d.h): the stride-1 tile convolution of ``mode`` on the image of ``conv3x3_tile_pack(W, mode)`` with
        ``vd3d_nhwc_bias_act_f32``'s chain in its epilogue.  ``relu_in``: the convolution reads relu(x) (a NaN stays a NaN).  Returns y, or (y, relu(y))."""
        self._nhwc_f32(x, r1, r2)
        B, Cin, H, W = x.shape
        for r in (r1, r2):
            if r is not None and tuple(r.shape) != (B, int(Cout), H, W):
                raise ValueError("conv3x3_epi: r1 and r2 have the output's shape")
        if bias is not None and (bias.dtype != torch.float32 or bias.numel() != int(Cout) or not bias.is_contiguous()):
            raise ValueError("conv3x3_epi: bias is a contiguous float32 [Cout]")
        out = torch.empty((B, int(Cout), H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        ro = torch.empty_like(out) if want_relu_copy else None
        self._enter(x, w_image, bias, r1, r2, out, ro)
        flags = (self.EPI_RELU_IN if relu_in else 0) | (self.EPI_RELU if relu else 0)
        _lib.check(self._L.vd3d_conv3x3_epi(self._ctx, {"bf16x3": 0, "fp16x2": 1}[mode], _ptr(x), B, H, W, Cin, _ptr(w_image), int(Cout), flags,
                                            _ptr(bias) if bias is not None else None, _ptr(r1) if r1 is not None else None,
                                            _ptr(r2) if r2 is not None else None, _ptr(out), _ptr(ro) if ro is not None else None))
        return (out, ro) if want_relu_copy else out

    def depthpro_head_pack(self, blocks: torch.Tensor, mode: str = "bf16x3"):
        """Split + pack the 16 composed blocks ``[16, 32, Cin]`` of ``neck_poly_compose(wt, None, w3, 2)`` for ``depthpro_head`` in ``mode``; ``None`` when the shape is
        not built (Cin % 16, 32 output channels)."""
        w = blocks.detach().to(self.device, torch.float32).contiguous()
        if w.dim() != 3 or tuple(w.shape[:2]) != (16, 32):
            return None
        nb = int(self._L.vd3d_depthpro_head_weight_bytes(self.X3_MODES[mode], int(w.shape[2])))
        if nb < 0:
            return None
        img = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._enter(w, img)
        _lib.check(self._L.vd3d_depthpro_head_pack_weights(self._ctx, self.X3_MODES[mode], _ptr(w), int(w.shape[2]), _ptr(img)))
        return img

    def depthpro_head(self, x: torch.Tensor, w_image: torch.Tensor, table: torch.Tensor, w3: torch.Tensor, b3: float, mode: str = "bf16x3") -> torch.Tensor:
        """DepthPro's head behind ``head.layers.0`` in one launch on the coarse map (``vd3d_depthpro_head``, include/vd3d.h; ``depth_pro.head_poly_statement``):
        float32 channels_last ``x`` [B, Cin, h, w] -> [B, 2h, 2w].  ``table``: float32 [3, 3, 32] (``depth_pro.head_poly_table``), ``w3``: float32 [32]."""
        self._nhwc_f32(x)
        B, Cin, h, w = x.shape
        if table.dtype != torch.float32 or tuple(table.shape) != (3, 3, 32) or not table.is_contiguous() or w3.dtype != torch.float32 or w3.numel() != 32 or not w3.is_contiguous():
            raise ValueError("depthpro_head: table is contiguous float32 [3, 3, 32], w3 float32 [32]")
        out = torch.empty((B, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
        self._enter(x, w_image, table, w3, out)
        _lib.check(self._L.vd3d_depthpro_head(self._ctx, self.X3_MODES[mode], _ptr(x), B, h, w, Cin, _ptr(w_image), _ptr(table), _ptr(w3), float(b3), _ptr(out)))
        return out

    def conv3x3_x2_pack(self, weight: torch.Tensor):
        """Split + pack a float32 3 x 3 convolution weight [Cout, Cin, 3, 3] for ``conv3x3_x2``; ``None`` when the shape is not built (Cin % 16, Cout in {32, 64, 128})."""
        return self._conv3x3_pack("x2", weight)

    def conv3x3_x2(self, x: torch.Tensor, w_image: torch.Tensor, Cout: int) -> torch.Tensor:
        """F.conv2d(x, W, None, stride 1, padding 1) for a float32 channels_last [B, Cin, H, W] tensor with W given as ``conv3x3_x2_pack(W)``: fp16x2 MFMA arithmetic,
        float32 accumulation (include/vd3d.h vd3d_conv3x3_x2); returns a channels_last [B, Cout, H, W] tensor."""
        return self._conv3x3("x2", x, w_image, Cout)

    def conv3x3_x3_pack(self, weight: torch.Tensor):
        """Split + pack a float32 3 x 3 convolution weight [Cout, Cin, 3, 3] for ``conv3x3_x3``; ``None`` when the shape is not built (Cin % 16, Cout in {32, 64, 128, 256})."""
        return self._conv3x3_pack("x3", weight)

    def conv3x3_x3(self, x: torch.Tensor, w_image: torch.Tensor, Cout: int) -> torch.Tensor:
        """F.conv2d(x, W, None, stride 1, padding 1) for a float32 channels_last [B, Cin, H, W] tensor with W given as ``conv3x3_x3_pack(W)``: bf16x3 MFMA arithmetic
        (three bf16 terms per operand, six products per MAC), float32 accumulation (include/vd3d.h vd3d_conv3x3_x3); returns a channels_last [B, Cout, H, W] tensor."""
        return self._conv3x3("x3", x, w_image, Cout)

    def conv3x3_s2_x3_pack(self, weight: torch.Tensor):
        """Split + pack a float32 3 x 3 convolution weight [Cout, Cin, 3, 3] for ``conv3x3_s2_x3``; ``None`` when the shape is not built (Cin % 16, Cout a multiple of
        128 up to 1024)."""
        return self._conv3x3_pack("s2_x3", weight)

    def conv3x3_s2_x3(self, x: torch.Tensor, w_image: torch.Tensor, Cout: int) -> torch.Tensor:
        """F.conv2d(x, W, None, stride 2, padding 1) for a float32 channels_last [B, Cin, H, W] tensor with W given as ``conv3x3_s2_x3_pack(W)``: bf16x3 MFMA
        arithmetic, float32 accumulation (include/vd3d.h vd3d_conv3x3_s2_x3); returns a channels_last [B, Cout, (H+1)//2, (W+1)//2] tensor."""
        return self._conv3x3("s2_x3", x, w_image, Cout)

    def conv3x3_s1_x2_pack(self, weight: torch.Tensor):
        """Scale, split + pack a float32 3 x 3 convolution weight [Cout, Cin, 3, 3] for ``conv3x3_s1_x2``; ``None`` when the shape is not built (Cin % 16, Cout in
        {32, 64, 128, 256})."""
        return self._conv3x3_pack("s1_x2", weight)

    def conv3x3_s1_x2(self, x: torch.Tensor, w_image: torch.Tensor, Cout: int) -> torch.Tensor:
        """F.conv2d(x, W, None, stride 1, padding 1) for a float32 channels_last [B, Cin, H, W] tensor with W given as ``conv3x3_s1_x2_pack(W)``: fp16x2 MFMA arithmetic
        (two fp16 terms per operand, three products per MAC, |x| < 65 504), float32 accumulation, on the 8 x 32 tile kernel that takes every map size
        (include/vd3d.h vd3d_conv3x3_s1_x2); returns a channels_last [B, Cout, H, W] tensor."""
        return self._conv3x3("s1_x2", x, w_image, Cout)

    def conv3x3_s2_x2_pack(self, weight: torch.Tensor):
        """Scale, split + pack a float32 3 x 3 convolution weight [Cout, Cin, 3, 3] for ``conv3x3_s2_x2``; ``None`` when the shape is not built (Cin % 16, Cout a
        multiple of 128 up to 1024)."""
        return self._conv3x3_pack("s2_x2", weight)

    def conv3x3_s2_x2(self, x: torch.Tensor, w_image: torch.Tensor, Cout: int) -> torch.Tensor:
        """F.conv2d(x, W, None, stride 2, padding 1) for a float32 channels_last [B, Cin, H, W] tensor with W given as ``conv3x3_s2_x2_pack(W)``: fp16x2 MFMA
        arithmetic, float32 accumulation (include/vd3d.h vd3d_conv3x3_s2_x2); returns a channels_last [B, Cout, (H+1)//2, (W+1)//2] tensor."""
        return self._conv3x3("s2_x2", x, w_image, Cout)

    def conv_ifn_pack(self, kind: int, weight: torch.Tensor):
        """Split + pack a float32 weight for ``conv_ifn``: ``[Cout, Cin, 3, 3]`` for ``_abi.IFN_K3S1`` / ``IFN_K3S2``, ``[Cin, Cout, 4, 4]`` (ConvTranspose2d's layout) for
        ``IFN_T4S2``; ``None`` when the shape is not built (Cin % 16, Cout in {32, 64, 96})."""
        w = weight.detach().to(self.device, torch.float32).contiguous()
        if kind == _abi.IFN_T4S2:
            Cin, Cout, kh, kw = w.shape
            ok = (kh, kw) == (4, 4)
        else:
            Cout, Cin, kh, kw = w.shape
            ok = (kh, kw) == (3, 3)
        nb = int(self._L.vd3d_conv_ifn_weight_bytes(int(kind), Cin, Cout)) if ok else -1
        if nb < 0:
            return None
        img = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._enter(w, img)
        _lib.check(self._L.vd3d_conv_ifn_pack_weights(self._ctx, int(kind), _ptr(w), Cin, Cout, _ptr(img)))
        return img

    def conv_ifn(self, kind: int, x: torch.Tensor, cin: int, w_image: torch.Tensor, bias: torch.Tensor, slope, cout: int, out: torch.Tensor,
                 out_offset: int = 0, residual=None) -> torch.Tensor:
        """One convolution of the interpolation network in the bf16x3 arithmetic (``vd3d_conv_ifn``, include/vd3d.h).  ``x``, ``out``, ``residual``: float32
        channels_last ``[B, C, H, W]`` tensors whose C is the pixel pitch; channels ``[0, cin)`` of ``x`` are read and ``[out_offset, out_offset + cout)`` of ``out``
        written.  ``out`` has the kind's output size (same, halved rounding up, doubled).  ``bias``: float32 ``[cout]``; ``slope``: per-channel PReLU slopes or None;
        ``residual``: added after the activation, or None.  Returns ``out``."""
        for t in (x, out, residual):
            if t is not None and (t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last)):
                raise AssertionError("conv_ifn takes float32 [B,C,H,W] tensors in channels_last memory")
        B, _, H, W = x.shape
        Ho, Wo = {_abi.IFN_K3S1: (H, W), _abi.IFN_K3S2: ((H + 1) // 2, (W + 1) // 2), _abi.IFN_T4S2: (2 * H, 2 * W)}[int(kind)]
        if out.shape[0] != B or tuple(out.shape[2:]) != (Ho, Wo) or (residual is not None and (residual.shape[0] != B or tuple(residual.shape[2:]) != (Ho, Wo))):
            raise AssertionError("conv_ifn: the output and the residual have the kind's output size")
        if bias.dtype != torch.float32 or bias.numel() != cout or (slope is not None and (slope.dtype != torch.float32 or slope.numel() != cout)):
            raise AssertionError("conv_ifn: bias and slope are float32 [cout]")
        self._enter(x, w_image, bias, slope, residual, out)
        _lib.check(self._L.vd3d_conv_ifn(self._ctx, int(kind), _ptr(x), B, H, W, int(x.shape[1]), int(cin), _ptr(w_image), _ptr(bias),
                                         _ptr(slope) if slope is not None else None, int(cout), _ptr(residual) if residual is not None else None,
                                         int(residual.shape[1]) if residual is not None else 0, _ptr(out), int(out.shape[1]), int(out_offset)))
        return out

    @staticmethod
    def _rife_pad(h: int, w: int):
        return (h + 31) // 32 * 32, (w + 31) // 32 * 32

    def rife_warp_pack(self, x6: torch.Tensor, state, scale: int, out: torch.Tensor) -> torch.Tensor:
        """The 16-channel input of one IFBlock (``vd3d_rife_warp_pack``): ``x6`` contiguous float32 ``[N, 6, h, w]``, ``state`` ``[N, Hp, Wp, 8]`` (flow, mask) or None for
        the first block, ``out`` ``[N, Hp/scale, Wp/scale, 16]`` (NHWC memory, i.e. a channels_last ``[N, 16, ., .]`` tensor permuted)."""
        N, _, h, w = x6.shape
        Hp, Wp = self._rife_pad(h, w)
        if x6.dtype != torch.float32 or x6.shape[1] != 6 or not x6.is_contiguous() or not out.is_contiguous() or tuple(out.shape) != (N, Hp // scale, Wp // scale, 16):
            raise AssertionError("rife_warp_pack: x6 contiguous float32 [N,6,h,w], out [N,Hp/s,Wp/s,16]")
        if state is not None and (tuple(state.shape) != (N, Hp, Wp, 8) or not state.is_contiguous()):
            raise AssertionError("rife_warp_pack: state is [N,Hp,Wp,8]")
        self._enter(x6, state, out)
        _lib.check(self._L.vd3d_rife_warp_pack(self._ctx, _ptr(x6), _ptr(state) if state is not None else None, N, h, w, int(scale), _ptr(out)))
        return out

    def rife_update(self, t: torch.Tensor, state: torch.Tensor, scale: int, first: bool, h: int, w: int) -> torch.Tensor:
        """``state[..., :4] += up(t[..., :4]) * scale; state[..., 4] += up(t[..., 4])`` (``vd3d_rife_update``; ``first``: written instead of added).  ``t``: contiguous
        ``[N, Hp/scale, Wp/scale, C]`` (C the pitch), ``state`` ``[N, Hp, Wp, 8]`` for an ``h x w`` frame."""
        Hp, Wp = self._rife_pad(h, w)
        N = state.shape[0]
        if tuple(state.shape) != (N, Hp, Wp, 8) or tuple(t.shape[:3]) != (N, Hp // scale, Wp // scale) or not t.is_contiguous() or not state.is_contiguous():
            raise AssertionError("rife_update: t [N,Hp/s,Wp/s,C], state [N,Hp,Wp,8]")
        self._enter(t, state)
        _lib.check(self._L.vd3d_rife_update(self._ctx, _ptr(t), int(t.shape[3]), 1 if first else 0, N, int(h), int(w), int(scale), _ptr(state)))
        return state

    def rife_blend(self, x6: torch.Tensor, state: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """The network's output (``vd3d_rife_blend``): both frames warped by the final flow, blended by sigmoid(mask), cropped: ``out`` contiguous ``[N, 3, h, w]``."""
        N, _, h, w = x6.shape
        Hp, Wp = self._rife_pad(h, w)
        if tuple(state.shape) != (N, Hp, Wp, 8) or tuple(out.shape) != (N, 3, h, w) or not out.is_contiguous() or not x6.is_contiguous() or x6.dtype != torch.float32:
            raise AssertionError("rife_blend: x6 [N,6,h,w], state [N,Hp,Wp,8], out [N,3,h,w], float32 contiguous")
        self._enter(x6, state, out)
        _lib.check(self._L.vd3d_rife_blend(self._ctx, _ptr(x6), _ptr(state), N, h, w, _ptr(out)))
        return out

    def upsample_bilinear(self, x: torch.Tensor, size) -> torch.Tensor:
        """F.interpolate(x, size, mode="bilinear", align_corners=True) for a float32 / bf16 channels_last [B,C,h,w] tensor."""
        B, Cc, ih, iw = x.shape
        oh, ow = int(size[0]), int(size[1])
        out = torch.empty((B, Cc, oh, ow), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        self._enter(x, out)
        _lib.check(self._L.vd3d_upsample_bilinear_nhwc(self._ctx, self._dt(x.dtype), _ptr(x), _ptr(out), B, ih, iw, oh, ow, Cc))
        return out

    # ---- float32 glue between the library convolutions of the DPT neck / head (vd3d_netops.hip); tensors are channels_last [B,C,h,w]
    @staticmethod
    def _nhwc_f32(*ts):
        for t in ts:
            if t is not None and not (t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
                raise ValueError("float32 channels_last [B,C,h,w] tensors expected")

    def bias_act(self, y, bias=None, r1=None, r2=None, relu=False, want_relu_copy=False):
        """In place on ``y``: y = [relu](r2 + ((y + bias[c]) + r1)); returns y, or (y, relu(y)) with ``want_relu_copy``."""
        self._nhwc_f32(y, r1, r2)
        B, Cc, h, w = y.shape
        ro = torch.empty_like(y) if want_relu_copy else None
        self._enter(y, bias, r1, r2, ro)
        _lib.check(self._L.vd3d_nhwc_bias_act_f32(self._ctx, _ptr(y), _ptr(bias) if bias is not None else None, _ptr(r1) if r1 is not None else None,
                                                  _ptr(r2) if r2 is not None else None, int(bool(relu)), B * h * w, Cc, _ptr(y),
                                                  _ptr(ro) if ro is not None else None))
        return (y, ro) if want_relu_copy else y

    def upsample_bilinear_bias(self, x, size, bias):
        """upsample_bilinear(x, size) + bias[c] (the bias of the convolution that produced x, run without it)."""
        self._nhwc_f32(x)
        B, Cc, ih, iw = x.shape
        oh, ow = int(size[0]), int(size[1])
        out = torch.empty((B, Cc, oh, ow), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        self._enter(x, bias, out)
        _lib.check(self._L.vd3d_upsample_bilinear_bias_nhwc_f32(self._ctx, _ptr(x), _ptr(bias), _ptr(out), B, ih, iw, oh, ow, Cc))
        return out

    def dpt_head_tail(self, y, b2, w3, b3: float, scale: float, act: str = "relu"):
        """[B,C,h,w] (conv2 WITHOUT its bias) -> [B,h,w]: act(b3 + sum_c w3[c] relu(y + b2[c])) * scale.  ``act``: ``"relu"`` (default;
        vd3d_dpt_head_tail_f32) or ``"sigmoid"`` (the metric Depth-Anything heads; vd3d_dpt_head_tail_act_f32, torch.sigmoid's CPU values)."""
        if act not in ("relu", "sigmoid"):
            raise ValueError("dpt_head_tail: act must be 'relu' or 'sigmoid'")
        self._nhwc_f32(y)
        B, Cc, h, w = y.shape
        out = torch.empty((B, h, w), dtype=torch.float32, device=y.device)
        self._enter(y, b2, w3, out)
        if act == "relu":
            _lib.check(self._L.vd3d_dpt_head_tail_f32(self._ctx, _ptr(y), _ptr(b2), _ptr(w3), float(b3), float(scale), B * h * w, Cc, _ptr(out)))
        else:
            _lib.check(self._L.vd3d_dpt_head_tail_act_f32(self._ctx, _ptr(y), _ptr(b2), _ptr(w3), float(b3), float(scale), B * h * w, Cc,
                                                          _abi.HEAD_ACT_SIGMOID, _ptr(out)))
        return out

    def dpt_head_conv_pack(self, weight: torch.Tensor):
        """Pack a float32 3 x 3 convolution weight [Cout, Cin, 3, 3] for ``dpt_head_conv``; ``None`` when the shape is not built (Cin 32 | 64 | 128 -> Cout 32
        with the tail, Cin 128 -> Cout 64 plain)."""
        w = weight.detach().to(self.device, torch.float32).contiguous()
        Cout, Cin, kh, kw = w.shape
        nb = int(self._L.vd3d_dpt_head_conv_weight_bytes(Cin, Cout)) if (kh, kw) == (3, 3) else -1
        if nb < 0:
            return None
        img = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._enter(w, img)
        _lib.check(self._L.vd3d_dpt_head_conv_pack_weights(self._ctx, _ptr(w), Cin, Cout, _ptr(img)))
        return img

    def head_conv_gather_pack(self, Wt: torch.Tensor, bc: torch.Tensor):
        """Lay ``depth.head_conv2_compose``'s tap-major weight ``Wt`` [9 * 32, Cin] and bias ``bc`` [9 * 32] out for ``dpt_head_conv(form="gather")`` -> (image, bc on
        the device, Cin); ``None`` when Cin is not built (32 | 64 | 128)."""
        if Wt.dim() != 2 or Wt.shape[0] != 288 or tuple(bc.shape) != (288,):
            raise ValueError(f"head_conv_gather_pack: Wt {tuple(Wt.shape)} / bc {tuple(bc.shape)} are not [288, Cin] and [288]")
        Cin = int(Wt.shape[1])
        nb = int(self._L.vd3d_head_conv_gather_weight_bytes(Cin))
        if nb < 0:
            return None
        w = Wt.detach().to(self.device, torch.float32).contiguous()
        b = bc.detach().to(self.device, torch.float32).contiguous().clone()
        img = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._enter(w, img)
        _lib.check(self._L.vd3d_head_conv_gather_pack_weights(self._ctx, _ptr(w), Cin, _ptr(img)))
        return img, b, Cin

    def head_conv_gather_tile(self, in_size, size, Cin: int):
        """The fine tile (th, tw) ``dpt_head_conv(form="gather")`` cuts an ``in_size`` -> ``size`` map into; ``None`` where the launch would be refused."""
        th, tw = C.c_int(0), C.c_int(0)
        if self._L.vd3d_head_conv_gather_tile(int(in_size[0]), int(in_size[1]), int(size[0]), int(size[1]), int(Cin), C.byref(th), C.byref(tw)) != 0:
            return None
        return th.value, tw.value

    def dpt_head_conv(self, x, b_in, size, w_image, b2=None, w3=None, b3: float = 0.0, scale: float = 1.0, Cout=None, form: str = "conv"):
        """conv3x3(upsample_bilinear_bias(x, size, b_in)) in one exact-float32 kernel (include/vd3d.h vd3d_dpt_head_conv_f32), W given as
        ``dpt_head_conv_pack(W)``.  With ``b2`` and ``w3`` (Cout 32): -> [B,h,w] = relu(b3 + sum_c w3[c] relu(y + b2[c])) * scale, ``dpt_head_tail``'s function;
        without (Cout 64): -> channels_last [B,Cout,h,w], the convolution without a bias.
        ``form="gather"``: the same function with the tail as coarse GEMM + fine gather in one launch (vd3d_head_conv_gather_f32; close, not equal bits): ``w_image``
        is then ``head_conv_gather_pack(...)``, whose composed bias already holds ``b_in`` (``b_in`` itself is not read)."""
        self._nhwc_f32(x)
        if form == "gather":
            if b2 is None or w3 is None or w_image is None:
                raise ValueError("dpt_head_conv: the gather form needs the tail's b2 and w3 and a packed image (head_conv_gather_pack)")
            img, bc, Cin = w_image
            B, Cx, ih, iw = x.shape
            oh, ow = int(size[0]), int(size[1])
            if Cx != Cin:
                raise ValueError(f"dpt_head_conv: the map has {Cx} channels, the packed weights take {Cin}")
            for name, t in (("b2", b2), ("w3", w3)):
                if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 32):
                    raise ValueError(f"dpt_head_conv: {name} must be 32 contiguous float32 values")
            out = torch.empty((B, oh, ow), dtype=torch.float32, device=x.device)
            self._enter(x, img, bc, b2, w3, out)
            _lib.check(self._L.vd3d_head_conv_gather_f32(self._ctx, _ptr(x), B, ih, iw, oh, ow, Cin, _ptr(img), _ptr(bc), _ptr(b2), _ptr(w3), float(b3), float(scale),
                                                         _ptr(out)))
            return out
        if form != "conv":
            raise ValueError(f"dpt_head_conv: form {form!r} is not 'conv' or 'gather'")
        if (b2 is None) != (w3 is None):
            raise ValueError("dpt_head_conv: b2 and w3 go together")
        B, Cin, ih, iw = x.shape
        oh, ow = int(size[0]), int(size[1])
        tail = b2 is not None
        Cout = int(Cout) if Cout is not None else (32 if tail else 64)
        for name, t, n in (("b_in", b_in, Cin), ("b2", b2, Cout), ("w3", w3, Cout)):
            if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
                raise ValueError(f"dpt_head_conv: {name} must be {n} contiguous float32 values")
        if w_image is None or w_image.numel() != int(self._L.vd3d_dpt_head_conv_weight_bytes(Cin, Cout)):
            raise ValueError(f"dpt_head_conv: the weight image does not belong to a built {Cin} -> {Cout} convolution")
        if tail:
            out = torch.empty((B, oh, ow), dtype=torch.float32, device=x.device)
        else:
            out = torch.empty((B, Cout, oh, ow), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        self._enter(x, b_in, w_image, b2, w3, out)
        _lib.check(self._L.vd3d_dpt_head_conv_f32(self._ctx, _ptr(x), _ptr(b_in), B, ih, iw, oh, ow, Cin, _ptr(w_image), Cout,
                                                  _ptr(b2) if tail else None, _ptr(w3) if tail else None, float(b3), float(scale), _ptr(out)))
        return out

    def neck_poly_pack(self, Wc: torch.Tensor, bc: torch.Tensor, f: int):
        """Lay the composed blocks of ``depth.neck_poly_compose`` (Wc [blocks, Cout, Cin], bc [blocks, Cout]) out for ``neck_poly_conv`` -> (image, bc on the device,
        Cin, Cout, f); ``None`` when (Cin, Cout, f) is not built ((96, 128, 4), (192, 128, 2), (48, 64, 4), (96, 64, 2))."""
        f = int(f)
        if Wc.dim() != 3 or bc.dim() != 2 or Wc.shape[0] != (f + 2) ** 2 or tuple(bc.shape) != tuple(Wc.shape[:2]):
            raise ValueError(f"neck_poly_pack: Wc {tuple(Wc.shape)} / bc {tuple(bc.shape)} are not [{(f + 2) ** 2}, Cout, Cin] and [{(f + 2) ** 2}, Cout]")
        Cout, Cin = int(Wc.shape[1]), int(Wc.shape[2])
        nb = int(self._L.vd3d_neck_poly_weight_bytes(Cin, Cout, f))
        if nb < 0:
            return None
        w = Wc.detach().to(self.device, torch.float32).contiguous()
        b = bc.detach().to(self.device, torch.float32).contiguous().clone()
        img = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._enter(w, img)
        _lib.check(self._L.vd3d_neck_poly_pack_f32(self._ctx, _ptr(w), Cin, Cout, f, _ptr(img)))
        return img, b, Cin, Cout, f

    def neck_poly_conv(self, x, packed):
        """conv3x3(ConvTranspose2d_{kernel = stride = f}(x) + bias) on the coarse channels_last float32 map ``x`` [B, Cin, h, w] in one exact-float32 kernel
        (include/vd3d.h vd3d_neck_poly_conv_f32) -> channels_last [B, Cout, f h, f w]; ``packed`` = ``neck_poly_pack(...)``."""
        self._nhwc_f32(x)
        if packed is None:
            raise ValueError("neck_poly_conv: the shape is not built (neck_poly_pack returned None)")
        img, b, Cin, Cout, f = packed
        B, Cx, h, w = x.shape
        if Cx != Cin:
            raise ValueError(f"neck_poly_conv: the map has {Cx} channels, the packed weights take {Cin}")
        out = torch.empty((B, Cout, f * h, f * w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        self._enter(x, img, b, out)
        _lib.check(self._L.vd3d_neck_poly_conv_f32(self._ctx, _ptr(x), B, h, w, Cin, _ptr(img), _ptr(b), Cout, f, _ptr(out)))
        return out

    def head_upconv_gather(self, z, size, Cout: int):
        """The fine half of conv3x3(upsample_bilinear(conv1x1(x) + b)) in "coarse GEMM + fine gather" form (include/vd3d.h vd3d_head_upconv_gather_f32): contiguous
        float32 ``z`` [B, h, w, 9 * Cout] (or [B, h, w, 9, Cout]; ``depth.head_upconv_compose``'s channels, tap-major) -> channels_last [B, Cout, H, W], the sum of the
        9 taps' bilinear samples per fine pixel: the convolution WITHOUT its bias.  Cout 64 | 32."""
        Cout, H, W = int(Cout), int(size[0]), int(size[1])
        if not (torch.is_tensor(z) and z.dtype == torch.float32 and z.dim() in (4, 5) and z.is_contiguous() and z.numel() == z.shape[0] * z.shape[1] * z.shape[2] * 9 * Cout):
            raise ValueError(f"head_upconv_gather: a contiguous float32 [B, h, w, 9 * {Cout}] tensor expected")
        B, h, w = (int(v) for v in z.shape[:3])
        out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=z.device, memory_format=torch.channels_last)
        self._enter(z, out)
        _lib.check(self._L.vd3d_head_upconv_gather_f32(self._ctx, _ptr(z), B, h, w, H, W, Cout, _ptr(out)))
        return out

    def depth_to_space_bias(self, y, B: int, H: int, W: int, s: int, bias=None):
        """The scatter of a kernel == stride ConvTranspose2d run as a GEMM: contiguous float32 ``y`` [B*H*W, s*s*C] (columns in (i, j, c) order) ->
        channels_last [B, C, H*s, W*s] with out[b, c, y*s+i, x*s+j] = y[(b*H+y)*W+x, (i*s+j)*C+c] + bias[c] (include/vd3d.h vd3d_depth_to_space_bias_nhwc_f32)."""
        P, N = y.shape
        Cc = N // (s * s)
        if y.dtype != torch.float32 or not y.is_contiguous() or P != B * H * W or Cc * s * s != N:
            raise ValueError("y must be contiguous float32 [B*H*W, s*s*C]")
        out = torch.empty((B, Cc, H * s, W * s), dtype=torch.float32, device=y.device, memory_format=torch.channels_last)
        self._enter(y, bias, out)
        _lib.check(self._L.vd3d_depth_to_space_bias_nhwc_f32(self._ctx, _ptr(y), _ptr(bias) if bias is not None else None, int(B), int(H), int(W), int(s), Cc,
                                                             _ptr(out)))
        return out

    def patchify(self, x: torch.Tensor, p: int) -> torch.Tensor:
        """The rows of a patch embedding run as a GEMM: float32 ``x`` of logical shape [B, 3, th, tw] in channels_last memory (what ``depth_preprocess`` returns) ->
        contiguous [B, (th // p) * (tw // p), Kp], column (c * p + ky) * p + kx = x[b, c, gy * p + ky, gx * p + kx] (``F.unfold``'s order), Kp = 3 p^2 rounded up
        to a multiple of 16 with the tail written as zeros (include/vd3d.h vd3d_patchify_f32)."""
        B, Cc, th, tw = x.shape
        if x.dtype != torch.float32 or Cc != 3 or not x.permute(0, 2, 3, 1).is_contiguous():
            raise ValueError("patchify: a float32 [B, 3, th, tw] tensor in channels_last memory expected")
        p = int(p)
        if p < 1 or th < p or tw < p:
            raise ValueError(f"patchify: a {th} x {tw} image holds no {p} x {p} patch")
        kp = (3 * p * p + 15) // 16 * 16
        out = torch.empty((B, (th // p) * (tw // p), kp), dtype=torch.float32, device=x.device)
        self._enter(x, out)
        _lib.check(self._L.vd3d_patchify_f32(self._ctx, _ptr(x), B, th, tw, p, _ptr(out)))
        return out

    # ---- the BiT ResNet prefix of DPT-Hybrid (vd3d_bit.hip); tensors are contiguous float32 NHWC [B, H, W, C]
    @staticmethod
    def _nhwc_rows(*ts):
        for t in ts:
            if t is not None and not (t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
                raise ValueError("contiguous float32 NHWC [B, H, W, C] tensors expected")

    def im2col(self, x: torch.Tensor, k: int, stride: int, pad, out=None) -> torch.Tensor:
        """The rows of a k x k convolution run as a GEMM: contiguous float32 NHWC ``x`` [B, H, W, C], ``pad`` = (top, bottom, left, right) zeros ->
        [B, Ho, Wo, Kp], column (ky * k + kx) * C + c (``im2col_gemm_weight``'s order), Kp = k k C rounded up to a multiple of 16 with a zero tail
        (include/vd3d.h vd3d_im2col_nhwc_f32).  ``out``: the rows' buffer, every element of which is written."""
        self._nhwc_rows(x)
        B, H, W, Cc = x.shape
        pt, pb, pl, pr = (int(v) for v in pad)
        k, stride = int(k), int(stride)
        if stride < 1 or H + pt + pb < k or W + pl + pr < k:
            raise ValueError(f"im2col: a {H} x {W} map padded by {tuple(pad)} holds no {k} x {k} window")
        Ho, Wo = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
        shape = (B, Ho, Wo, (k * k * Cc + 15) // 16 * 16)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"im2col: out must be a contiguous float32 tensor of shape {shape}")
        self._enter(x, out)
        _lib.check(self._L.vd3d_im2col_nhwc_f32(self._ctx, _ptr(x), B, H, W, Cc, k, stride, pt, pb, pl, pr, _ptr(out)))
        return out

    def maxpool3x3_s2(self, x: torch.Tensor, pad, pad_value: float = 0.0) -> torch.Tensor:
        """F.max_pool2d(F.pad(x, pad, value=pad_value), 3, 2) for a contiguous float32 NHWC [B, H, W, C] tensor, ``pad`` = (top, bottom, left, right)
        (include/vd3d.h vd3d_maxpool3x3_s2_nhwc_f32)."""
        self._nhwc_rows(x)
        B, H, W, Cc = x.shape
        pt, pb, pl, pr = (int(v) for v in pad)
        if H + pt + pb < 3 or W + pl + pr < 3:
            raise ValueError(f"maxpool3x3_s2: a {H} x {W} map padded by {tuple(pad)} holds no 3 x 3 window")
        out = torch.empty((B, (H + pt + pb - 3) // 2 + 1, (W + pl + pr - 3) // 2 + 1, Cc), dtype=torch.float32, device=x.device)
        self._enter(x, out)
        _lib.check(self._L.vd3d_maxpool3x3_s2_nhwc_f32(self._ctx, _ptr(x), B, H, W, Cc, pt, pb, pl, pr, float(pad_value), _ptr(out)))
        return out

    def groupnorm(self, x: torch.Tensor, groups: int, weight: torch.Tensor, bias: torch.Tensor, eps: float, residual=None, relu: bool = False, out=None) -> torch.Tensor:
        """[relu](group_norm(x, groups, weight, bias, eps) [+ residual]) for contiguous float32 NHWC [B, H, W, C] tensors: mean first, then the centred sum of
        squares, in one fixed summation order -- a frame's values do not depend on its batch (include/vd3d.h vd3d_groupnorm_nhwc_f32).  ``out`` may be ``x``."""
        self._nhwc_rows(x, residual, out)
        B, H, W, Cc = x.shape
        if residual is not None and residual.shape != x.shape:
            raise ValueError("groupnorm: the residual must have x's shape")
        nb = int(self._L.vd3d_groupnorm_nhwc_f32_workspace_bytes(B, H * W, Cc, int(groups)))
        if nb < 0:
            raise NotImplementedError(f"groupnorm: {Cc} channels in {groups} groups (batch {B}, {H * W} pixels) not built")
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        out = torch.empty_like(x) if out is None else out
        self._enter(x, residual, weight, bias, ws, out)
        _lib.check(self._L.vd3d_groupnorm_nhwc_f32(self._ctx, _ptr(x), _ptr(residual) if residual is not None else None, _ptr(weight), _ptr(bias), float(eps),
                                                   _abi.GN_RELU if relu else 0, B, H * W, Cc, int(groups), _ptr(ws), nb, _ptr(out)))
        return out

    # ---- DepthPro (vd3d_depthpro.hip; depth_pro.py holds the statements)
    def depthpro_preprocess(self, frames_bgr: torch.Tensor, size: int, mean, std) -> torch.Tensor:
        """DepthProImageProcessor in one launch: uint8 BGR [B, H, W, 3] -> contiguous float32 pixel_values [B, 3, size, size] -- rescale and normalise as a
        table of the byte, then the bilinear resize without antialias (include/vd3d.h vd3d_depthpro_preprocess_u8; ``depth_pro.preprocess_statement``)."""
        f = frames_bgr.to(self.device)
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3:
            raise TypeError("depthpro_preprocess takes uint8 [B,H,W,3] BGR frames")
        f = f.contiguous()
        B, H, W, _ = f.shape
        out = torch.empty((B, 3, int(size), int(size)), dtype=torch.float32, device=self.device)
        m = (C.c_float * 3)(*[float(v) for v in mean]); s = (C.c_float * 3)(*[float(v) for v in std])
        self._enter(f, out)
        _lib.check(self._L.vd3d_depthpro_preprocess_u8(self._ctx, _ptr(f), B, H, W, int(size), m, s, _ptr(out)))
        return out

    def depthpro_post(self, pred: torch.Tensor, fov, oH: int, oW: int, out=None) -> torch.Tensor:
        """DepthPro's post-process in one launch: float32 [B, S, S] and the field of view (float32 [B] on the device, degrees, or None) -> inverse depth
        [B, oH, oW]: scale by oW / focal, bilinear resize (skipped for oH == oW == S), clamp to [1e-4, 1e4], reciprocal.  The field of view is read by the
        kernel: no host synchronisation (include/vd3d.h vd3d_depthpro_post_f32; ``depth_pro.post_statement``)."""
        if pred.dtype != torch.float32 or pred.dim() != 3 or pred.shape[1] != pred.shape[2] or not pred.is_contiguous():
            raise ValueError("depthpro_post: a contiguous float32 [B, S, S] prediction expected")
        B, S, _ = pred.shape
        if fov is not None:
            fov = fov.to(pred.device, torch.float32).reshape(-1).contiguous()
            if fov.numel() != B:
                raise ValueError("depthpro_post: one field of view per frame expected")
        if out is None:
            out = torch.empty((B, int(oH), int(oW)), dtype=torch.float32, device=pred.device)
        self._enter(pred, fov, out)
        _lib.check(self._L.vd3d_depthpro_post_f32(self._ctx, _ptr(pred), _ptr(fov) if fov is not None else None, B, S, int(oH), int(oW), _ptr(out)))
        return out

    # ---- ZoeDepth (vd3d_zoedepth.hip; zoedepth.py holds the statements)
    def zoedepth_preprocess(self, frames_bgr: torch.Tensor, pads, target, mean, std, table: torch.Tensor) -> torch.Tensor:
        """ZoeDepthImageProcessor in one launch: uint8 BGR [B, H, W, 3] -> float32 pixel_values [B, 3, th, tw] in channels_last memory -- the rescale as the
        256-entry ``table`` of the byte (``zoedepth.rescale_table``, on the device), the reflect padding by ``pads`` = (pad_h, pad_w) folded into the gather, the
        align_corners=True bilinear resize to ``target`` = (th, tw), then (v - mean) / std (include/vd3d.h vd3d_zoedepth_preprocess_u8;
        ``zoedepth.preprocess_statement``)."""
        f = frames_bgr.to(self.device)
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3:
            raise TypeError("zoedepth_preprocess takes uint8 [B,H,W,3] BGR frames")
        if table.dtype != torch.float32 or table.numel() != 256 or not table.is_contiguous() or table.device != f.device:
            raise ValueError("zoedepth_preprocess: the rescale table is 256 contiguous float32 values on the frames' device")
        f = f.contiguous()
        B, H, W, _ = f.shape
        th, tw = int(target[0]), int(target[1])
        out = torch.empty((B, th, tw, 3), dtype=torch.float32, device=self.device)
        m = (C.c_float * 3)(*[float(v) for v in mean]); s = (C.c_float * 3)(*[float(v) for v in std])
        self._enter(f, table, out)
        _lib.check(self._L.vd3d_zoedepth_preprocess_u8(self._ctx, _ptr(f), _ptr(table), B, H, W, int(pads[0]), int(pads[1]), th, tw, m, s, _ptr(out)))
        return out.permute(0, 3, 1, 2)

    def zoedepth_post(self, pred: torch.Tensor, H: int, W: int, pads, out=None) -> torch.Tensor:
        """ZoeDepth's post-process in one launch: float32 [B, th, tw] -> [B, H, W], the bicubic resize to (H + 2 pad_h, W + 2 pad_w) evaluated inside the crop only
        (include/vd3d.h vd3d_zoedepth_post_f32; ``zoedepth.post_statement``)."""
        if pred.dtype != torch.float32 or pred.dim() != 3 or not pred.is_contiguous():
            raise ValueError("zoedepth_post: a contiguous float32 [B, th, tw] prediction expected")
        B, th, tw = pred.shape
        if out is None:
            out = torch.empty((B, int(H), int(W)), dtype=torch.float32, device=pred.device)
        self._enter(pred, out)
        _lib.check(self._L.vd3d_zoedepth_post_f32(self._ctx, _ptr(pred), B, th, tw, int(H), int(W), int(pads[0]), int(pads[1]), _ptr(out)))
        return out

    def zoedepth_attractor(self, attractors: torch.Tensor, prev_bins: torch.Tensor, kind: str = "mean") -> torch.Tensor:
        """ZoeDepthAttractorLayerUnnormed behind its MLP in one launch: contiguous float32 NHWC attractor points [B, h, w, nA] (after softplus) and previous bins
        [B, hp, wp, nb] -> new bins [B, h, w, nb] (include/vd3d.h vd3d_zoedepth_attractor_f32; ``zoedepth.attractor_statement``)."""
        if kind not in ("mean", "sum"):
            raise ValueError("zoedepth_attractor: kind is 'mean' or 'sum'")
        for t in (attractors, prev_bins):
            if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
                raise ValueError("zoedepth_attractor: contiguous float32 [B, h, w, C] maps expected")
        B, h, w, nA = attractors.shape
        if prev_bins.shape[0] != B:
            raise ValueError("zoedepth_attractor: one batch size expected")
        _, hp, wp, nb = prev_bins.shape
        out = torch.empty((B, h, w, nb), dtype=torch.float32, device=attractors.device)
        self._enter(attractors, prev_bins, out)
        _lib.check(self._L.vd3d_zoedepth_attractor_f32(self._ctx, _ptr(attractors), _ptr(prev_bins), B, h, w, hp, wp, nA, nb, int(kind == "mean"), _ptr(out)))
        return out

    def zoedepth_bins(self, last: torch.Tensor, rel, wrel, P: torch.Tensor, bins: torch.Tensor, w1_last: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                      b2: torch.Tensor, table: torch.Tensor, min_temp: float, max_temp: float) -> torch.Tensor:
        """The conditional log-binomial tail of ZoeDepth's metric head in one launch: contiguous float32 NHWC ``last`` [B, H, W, 32], the optional relative-depth
        plane ``rel`` [B, H, W] with its weight column ``wrel`` [Ch], ``P`` = W1_e . e [B, hc, wc, Ch], ``bins`` [B, hc, wc, nb], ``w1_last`` [Ch, 32], ``b1`` [Ch],
        ``w2`` [4, Ch], ``b2`` [4] and the module's float32 log-binomial ``table`` [nb] -> metric depth [B, H, W] (include/vd3d.h vd3d_zoedepth_bins_f32;
        ``zoedepth.bins_statement``)."""
        ts = [last, P, bins, w1_last, b1, w2, b2, table] + ([rel, wrel] if rel is not None else [])
        if (rel is None) != (wrel is None) or any(t.dtype != torch.float32 or not t.is_contiguous() for t in ts) or last.dim() != 4 or P.dim() != 4 or bins.dim() != 4:
            raise ValueError("zoedepth_bins: contiguous float32 tensors expected, the plane and its weight column together or not at all")
        B, H, W, cl = last.shape
        _, hc, wc, Ch = P.shape
        nb = bins.shape[3]
        if cl != 32 or tuple(bins.shape[:3]) != (B, hc, wc) or P.shape[0] != B or tuple(w1_last.shape) != (Ch, 32) or b1.numel() != Ch or tuple(w2.shape) != (4, Ch) \
                or b2.numel() != 4 or table.numel() != nb or (rel is not None and (tuple(rel.shape) != (B, H, W) or wrel.numel() != Ch)):
            raise ValueError(f"zoedepth_bins: shapes {tuple(last.shape)} / {tuple(P.shape)} / {tuple(bins.shape)} / {tuple(w1_last.shape)} / {tuple(w2.shape)} do not fit "
                             "[B,H,W,32] / [B,hc,wc,Ch] / [B,hc,wc,nb] / [Ch,32] / [4,Ch]")
        out = torch.empty((B, H, W), dtype=torch.float32, device=last.device)
        self._enter(*ts, out)
        p = lambda t: _ptr(t) if t is not None else None   # noqa: E731
        _lib.check(self._L.vd3d_zoedepth_bins_f32(self._ctx, _ptr(last), p(rel), p(wrel), _ptr(P), _ptr(bins), _ptr(w1_last), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(table),
                                                  float(min_temp), float(max_temp), B, H, W, hc, wc, Ch, nb, _ptr(out)))
        return out

    def depthpro_patches(self, pixel_values: torch.Tensor, p: int, strides) -> torch.Tensor:
        """DepthProPatchEncoder's patch pyramid in one launch: contiguous float32 pixel_values [B, 3, S, S] (S a multiple of 4) -> the stack its ViT sees,
        logical shape [(n1 + n2 + n4) B, 3, p, p] in channels_last memory (what ``patchify`` takes): full-resolution patches first, then the half level, then the
        quarter level, patch-major and batch-minor inside a level.  ``strides``: (full, half, quarter), each int(p (1 - overlap))
        (include/vd3d.h vd3d_depthpro_patches_f32; ``depth_pro.patches_statement``)."""
        x = pixel_values
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or not x.is_contiguous():
            raise ValueError("depthpro_patches: contiguous float32 [B, 3, S, S] pixel values expected")
        B, _, S, _ = x.shape
        p, st = int(p), [int(v) for v in strides]
        n = int(self._L.vd3d_depthpro_patches_count(S, p, *st))
        if n < 1:
            raise ValueError(f"depthpro_patches: a {S} x {S} image (a multiple of 4 expected) holds no {p} x {p} patch at a quarter of its size, or a stride of {st} is below 1")
        out = torch.empty((n * B, p, p, 3), dtype=torch.float32, device=x.device)
        self._enter(x, out)
        _lib.check(self._L.vd3d_depthpro_patches_f32(self._ctx, _ptr(x), B, S, p, *st, _ptr(out)))
        return out.permute(0, 3, 1, 2)   # NCHW view of NHWC storage == torch.channels_last

    def depthpro_merge(self, rows: torch.Tensor, B: int, g: int, padding: int, oh: int, ow: int) -> torch.Tensor:
        """reconstruct_feature_maps in one launch: contiguous float32 token rows [n B, T, C] (T >= g^2: the leading tokens are dropped) -> contiguous NHWC
        [B, oh, ow, C]: the patches merged with ``min(g // 4, padding)`` tokens trimmed on every edge that meets another patch, then ATen's bilinear resize, skipped
        where the merged size is the output size (include/vd3d.h vd3d_depthpro_merge_f32; ``depth_pro.merge_statement``)."""
        if rows.dtype != torch.float32 or rows.dim() != 3 or not rows.is_contiguous() or rows.shape[0] % int(B):
            raise ValueError("depthpro_merge: contiguous float32 token rows [n B, T, C] expected")
        nB, T, Cc = rows.shape
        out = torch.empty((int(B), int(oh), int(ow), Cc), dtype=torch.float32, device=rows.device)
        self._enter(rows, out)
        _lib.check(self._L.vd3d_depthpro_merge_f32(self._ctx, _ptr(rows), nB // int(B), int(B), T, Cc, int(g), int(padding), int(oh), int(ow), _ptr(out)))
        return out

    def detect_black_bars(self, frame_bgr: torch.Tensor):
        """detect_black_bars(frame_to_tensor(frame)) (core/render_3d.py:293-316) on a uint8 BGR frame -> (top, bottom)."""
        f = frame_bgr.to(self.device, torch.uint8).contiguous()
        t, b = C.c_int(), C.c_int()
        self._enter(f)
        _lib.check(self._L.vd3d_detect_black_bars(self._ctx, _ptr(f), f.shape[0], f.shape[1], C.byref(t), C.byref(b)))
        return t.value, b.value

    def debug_planes(self, H, W, eh=None, ew=None):
        """Copies of the internal planes of the last call (tests only)."""
        ptrs = [C.c_void_p() for _ in range(6)]
        self._L.vd3d_debug_planes(self._ctx, *[C.byref(p) for p in ptrs])
        self.sync()

        def view(ptr, shape, dtype):
            t = torch.empty(shape, dtype=dtype, device=self.device)
            _lib.check(self._L.vd3d_stream_copy(self._ctx, ptr, _ptr(t), t.numel() * t.element_size()))
            return t

        out = {"D": view(ptrs[0], (H, W), torch.float32), "S": view(ptrs[1], (H, W), torch.float32),
               "L": view(ptrs[2], (H, W, 3), torch.uint8), "R": view(ptrs[3], (H, W, 3), torch.uint8)}
        if eh:
            out["rgb_eye"] = view(ptrs[4], (3, eh, ew), torch.float32)
            out["dn"] = view(ptrs[5], (eh, ew), torch.float32)
        self.sync()
        return out


# ---------------------------------------------------------------------------------------------------
# module-level functions with the reference's names
# ---------------------------------------------------------------------------------------------------
_default: Renderer | None = None


def default_renderer() -> Renderer:
    """The module-level renderer plays the role of the reference's module singletons."""
    global _default
    if _default is None:
        _default = Renderer()
    return _default


def frame_to_tensor(frame):  # core/render_3d.py:135-138: BGR->RGB, /255.0 ON THE HOST (true division), then upload
    t = torch.from_numpy(np.ascontiguousarray(frame[..., ::-1])).float().permute(2, 0, 1) / 255.0
    return t.to(torch_device)


def pixel_shift_cuda(frame_tensor, depth_tensor, width, height, fg_shift, mg_shift, bg_shift, return_shift_map=True, **kw):
    """Same signature and returns as the reference (core/render_3d.py:561-712): host uint8 BGR arrays
    (+ the float32 shift map on CPU when ``return_shift_map``).  Mutates the default renderer's
    FloatingWindowTracker exactly like the reference mutates its module global.  Extension keyword ``aten_threads`` (default: this process's
    ``torch.get_num_threads()`` / ``VD3D_ATEN_THREADS``, ``params.reference_aten_threads``; 0 = thread-independent arithmetic)."""
    p = shift_params_from_kwargs(fg_shift, mg_shift, bg_shift, **kw)
    r = default_renderer()
    res = r.pixel_shift(frame_tensor, depth_tensor, width, height, p, want_shift=bool(return_shift_map))
    if return_shift_map:
        return r.to_host(res[0]).numpy(), r.to_host(res[1]).numpy(), r.to_host(res[2])
    return r.to_host(res[0]).numpy(), r.to_host(res[1]).numpy()


def format_3d_output(left, right, fmt):
    """Same signature as the reference (core/render_3d.py:837): NumPy BGR eyes in, the muxed NumPy frame out."""
    r = default_renderer()
    out = r.format_3d_output(torch.from_numpy(np.ascontiguousarray(left)), torch.from_numpy(np.ascontiguousarray(right)), fmt)
    return r.to_host(out).numpy()


def generate_anaglyph_3d(left_frame, right_frame):
    """Same signature as the reference (core/render_3d.py:862): Dubois-style red-cyan anaglyph of two BGR frames."""
    return format_3d_output(left_frame, right_frame, "Red-Cyan Anaglyph")


def heal_missing_pixels(warped_frame, warped_depth, original_frame, edge_mask, heal_strength=0.5):
    """Same signature as the reference (core/render_3d.py:431): ``warped_depth`` is accepted and unused, exactly like there."""
    return default_renderer().heal_missing_pixels(warped_frame, original_frame, edge_mask, heal_strength)


def render_clip(frames, depths, **kw):
    """The render_sbs_3d frame loop over in-memory frames (uint8 BGR arrays/tensors) and depths
    (float32 [h,w] or uint8 depth-video frames).  Yields muxed frames.  Mirrors the reference's read
    order: the first frame of the clip is consumed before the loop and never rendered (:1026,1184,1222).
    Keywords: see ``render_pairs``."""
    return render_pairs(zip(frames, depths), **kw)


def render_pairs(pairs, *, renderer: Renderer | None = None, target_ratio=16 / 9, keep_on_device=False,
                 blank_frames=None, start_frame_idx=0, skip_first=True, batch=8, aten_sum_threads=None, **kw):
    """``render_clip`` over ONE iterable of (frame, depth) pairs.  ``skip_first=False``: the caller has already consumed the
    clip's first frame (render_sbs_3d's capture shell does, like the reference).

    ``skip_blank_frames=True`` uses ``blank_frames`` (absolute frame indices, what the reference's
    ``detect_black_white_frames`` returns; tested as ``start_frame_idx + loop index`` like :1063,1278); without a
    list it renders every frame, which is what the reference does when its detection fails (:1058-1060).

    ``batch`` > 1 (default 8): frames go through the renderer in STEPS of ``batch`` frames (``sharded.ChunkSharder`` at world 1: the
    select chain of a step in a dozen launches instead of eight per frame, its pixel kernels on two streams behind the next step's
    chain) -- bit-identical to the frame-by-frame loop (``batch=1``: one ``vd3d_render_frame`` per pair), frames are yielded in order,
    up to two steps (``2 * batch`` frames) late.  Cost of the default: ``2 * batch`` slots of seven float32 planes each stay allocated
    on the device (about 4 GB at 3840x2160 with ``batch=8``).

    ``aten_sum_threads`` (extension; default ``None`` = ``params.reference_aten_threads()``: ``torch.get_num_threads()`` of this process, or
    ``VD3D_ATEN_THREADS``): the N of the N-thread ATen mode -- the reference's two ``torch.mean`` sums, its ``pow`` / ``sigmoid`` scalar tails and its
    small-output bilinear kernel as torch computes them with N intra-op threads (core/render_3d.py:418,928,209,517,595-596).  0 = the
    thread-independent arithmetic (the C ABI's default).  The generator puts the renderer into overlapped mode; ``close()`` it
    (or exhaust it) to return the renderer to sequential mode -- a consumer that stops early should not wait for garbage collection."""
    r = renderer or default_renderer()
    blank = set(blank_frames or ()) if kw.get("skip_blank_frames") else set()
    # the reference's thread-dependent float32 arithmetic by default (round 6): this loop stands in for the reference's own, in its process
    kw["aten_sum_threads"] = reference_aten_threads() if aten_sum_threads is None else int(aten_sum_threads)
    it = iter(pairs)
    if skip_first and next(it, None) is None:
        return
    if int(batch) > 1 and hasattr(r, "shard2_p1_batch"):   # a renderer without the step entry points (a test double) takes the frame-by-frame loop
        yield from _render_pairs_batched(r, it, int(batch), target_ratio, keep_on_device, blank, start_frame_idx, kw)
        return
    params = None
    for idx, (f, d) in enumerate(it):
        if params is None:
            params = render_kwargs_to_params(int(f.shape[1]), int(f.shape[0]), target_ratio=target_ratio, **kw)
            r.new_clip()
        ft = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f))
        dt = d if torch.is_tensor(d) else torch.from_numpy(np.ascontiguousarray(d))
        out = r.render_frame(ft.to(r.device, non_blocking=True), dt.to(r.device, non_blocking=True), params,
                             blank=(start_frame_idx + idx) in blank)
        if getattr(r, "_private", False):   # the consumer (a D2H copy below, or the caller's own kernels on torch's stream) runs behind the renderer's stream
            r.ordered_after()
        yield out if keep_on_device else out.cpu().numpy()


def _render_pairs_batched(r, it, B, target_ratio, keep_on_device, blank, start_frame_idx, kw):
    """The loop of ``render_pairs`` in steps of B frames on two alternating slot sets (module docstring of ``sharded``)."""
    from .sharded import ChunkSharder, HipChunkBackend
    sets, params, pending, idx0 = None, None, [], 0

    def drain(step):
        sh, outs = step
        for j, o in enumerate(outs):
            r.wait_pixels(sh.slot_base + j)      # host wait: the frame's pixel pass has written it
            yield o if keep_on_device else o.cpu().numpy()
    k = 0
    try:
        while True:
            chunk = []
            for f, d in it:
                chunk.append((f, d))
                if len(chunk) == B:
                    break
            if not chunk:
                break
            if params is None:
                f0 = chunk[0][0]
                params = render_kwargs_to_params(int(f0.shape[1]), int(f0.shape[0]), target_ratio=target_ratio, **kw)
                r.new_clip()
                be = HipChunkBackend(r, params)
                first = ChunkSharder(be, 0, 1, B)
                sets = [first, ChunkSharder(be, 0, 1, B, slot_base=B, twin_of=first)]
                r.set_pixel_overlap(2)
            T = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(r.device, non_blocking=True)
            fl, dl = [T(f) for f, _ in chunk], [T(d) for _, d in chunk]
            flags = [(start_frame_idx + idx0 + j) in blank for j in range(len(chunk))] if blank else None
            sh = sets[k % 2]
            outs = sh.render_step(fl, dl, n_valid=len(chunk), blank=flags, first_step=(k == 0), more_steps=True)
            pending.append((sh, outs))
            if len(pending) == 2:                 # step k - 1 is complete once step k has been enqueued behind it
                yield from drain(pending.pop(0))
            idx0 += len(chunk)
            k += 1
        for step in pending:
            yield from drain(step)
        pending = []
    finally:
        if sets is not None:
            r.set_pixel_overlap(0)               # joins whatever is still in flight; the renderer is back in sequential mode
            if getattr(r, "_private", False):
                r.ordered_after()


from .video_io import render_sbs_3d  # noqa: E402,F401  (the reference module exports it, core/render_3d.py:933)
