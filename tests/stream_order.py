"""Stream order: every public wrapper that enqueues work, run behind a producer that is LATE on purpose.

The rest of the suite calls the wrappers with operands that were finished long before the call, on the default stream.  There a wrapper that forgets ``_enter``, or
leaves a tensor out of it, or a lost hand-over event in ``vd3d_ctx_set_stream``, changes nothing.  Here the operands of a call arrive behind a measured delay:

  1. reference -- the call in ordinary placement (operands complete, default stream), synchronised; the other tests hold that result to its statement;
  2. the LATE operands are allocated on the device pre-filled bytewise with 0x47 (tests/arena.py's finite, large fill: 51015.28 as float32, 71 as uint8);
  3. on the producer stream: the delay, then ``copy_(non_blocking=True)`` of the true operands from pinned host memory;
  4. the wrapper is called;
  5. the consumer stream is ordered as the placement prescribes and clones every output;
  6. after one synchronisation every clone is bit-identical to step 1.  A kernel that was not ordered behind the producer has read the fill.

Safety rule: only sample data is ever late -- pixels, activations, float weights, all of a floating or uint8 dtype and each declared ``payload`` by its row.  Every
tensor a kernel takes addresses from is EARLY (complete before the delay starts): tile origins and tables, plan tensors, letterbox bars, look-up tables, packed
images, workspaces, tracker state, and also the float planes that drive a warp (the depth of ``pixel_shift`` / ``render_frame`` / ``finish_frame``, the flow state of
the RIFE glue, the shift map of the arrow overlay) and the class map of the Canny hysteresis.  ``check_late_rule`` asserts it for every row, on the host.

The delay is ``torch.cuda._sleep`` calibrated with a pair of events (a ``torch.matmul`` chain where ``_sleep`` is missing), at least 5 ms, 20 x the row's own
duration (a) and 100 x the enqueue-to-completion time of an empty kernel on a side stream (b, an upper bound of its enqueue-to-start latency); at most 100 ms.  A
run also checks that the producer was still busy when the wrapper returned (``host_sync`` rows excepted: they wait for their own result), so a delay that ran out
under a slow host is reported as the harness's failure, not the library's.

The table (``ROWS``): one row per public wrapper, at the smallest ragged shape of the wrapper's own test; operand builders of tests/test_hip_arena.py where they
fit.  ``EXCLUDED`` lists, with a reason each, the functions that call ``_enter`` and have no row.  ``enter_callers`` / ``static_problems`` are the host checks
(tests/test_stream_order_host.py)."""
from __future__ import annotations

import ast
import os
import statistics
import sys
import time
import types
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hip_arena as A   # noqa: E402
import test_rife_glue_host as RG   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x47
MIN_DELAY_MS, MAX_DELAY_MS = 5.0, 100.0
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ---------------------------------------------------------------------------------------------------------------- a row
@dataclass
class StreamCase:
    late: dict                     # name -> CPU tensor / array: arrives behind the delay
    early: dict                    # name -> CPU tensor / array: complete before the delay starts
    call: object                   # call(R, ops) -> tuple of output tensors; ops[name] = the operand on the device; public wrappers only
    payload: tuple = ()            # the names the builder declares sample data (must be exactly the late ones)
    host_sync: bool = False        # the wrapper waits for its own result on the host (returns host values)

    def __post_init__(self):
        self.late = {n: _cpu(a) for n, a in self.late.items()}
        self.early = {n: _cpu(a) for n, a in self.early.items()}


def _cpu(a):
    if torch.is_tensor(a):
        return a.detach().cpu().contiguous()
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.copy())
    return t.view(torch.bfloat16) if a.dtype == np.int16 else t   # tests/test_hip_arena.py carries bf16 operands as their int16 bits


def check_late_rule(case: StreamCase, rid: str = ""):
    """Every late operand is declared payload by its builder and has a floating or uint8 dtype; nothing else is declared."""
    assert set(case.payload) == set(case.late), f"stream_order row {rid}: late operands {sorted(case.late)} are not the declared payload {sorted(case.payload)}"
    for n, t in case.late.items():
        assert t.dtype.is_floating_point or t.dtype == torch.uint8, (f"stream_order row {rid}: late operand '{n}' is {t.dtype}: only float and uint8 sample data may "
                                                                     "arrive late (an unfinished index could send a kernel outside its buffers)")
        assert n not in case.early, f"stream_order row {rid}: operand '{n}' is both late and early"


def poisoned_like(t: torch.Tensor, device) -> torch.Tensor:
    d = torch.empty(t.shape, dtype=t.dtype, device=device)
    d.view(_INT_OF[t.element_size()]).fill_(int.from_bytes(bytes([POISON]) * t.element_size(), "little"))
    return d


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    a, b = a.cpu(), b.cpu()
    return bool(torch.equal(a.view(_INT_OF[a.element_size()]), b.view(_INT_OF[b.element_size()])))


# ---------------------------------------------------------------------------------------------------------------- the harness
@dataclass
class Ref:
    outs: tuple
    a_ms: float


class Harness:
    """Delay, the two measured figures, and the run of one row in one placement."""

    def __init__(self, device=0):
        self.device = torch.device("cuda", device)
        self.bad_stream = torch.cuda.Stream(self.device)
        self._mm = None
        self._bad_ref = None
        self.delay_kind = "_sleep" if hasattr(torch.cuda, "_sleep") else "matmul"
        try:
            self.units_per_ms = self._calibrate()
        except RuntimeError:
            if self.delay_kind == "matmul":
                raise
            self.delay_kind = "matmul"
            self.units_per_ms = self._calibrate()
        self.launch_ms = self._launch_latency()
        got = self._timed(lambda: self.sleep(MIN_DELAY_MS))
        assert 0.8 * MIN_DELAY_MS <= got <= 3 * MIN_DELAY_MS, f"stream_order harness: a {MIN_DELAY_MS} ms delay ({self.delay_kind}) took {got:.3f} ms: the calibration is off"

    # -- the delay
    def _spin(self, units: int):
        if self.delay_kind == "_sleep":
            torch.cuda._sleep(int(units))
            return
        if self._mm is None:
            self._mm = torch.full((1024, 1024), 1.0 / 1024, device=self.device), torch.empty((1024, 1024), device=self.device)
        for _ in range(int(units)):
            torch.matmul(self._mm[0], self._mm[0], out=self._mm[1])

    def _timed(self, fn) -> float:
        s = torch.cuda.Stream(self.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return float(e0.elapsed_time(e1))

    def _calibrate(self) -> float:
        probe = 1_000_000 if self.delay_kind == "_sleep" else 20
        self._timed(lambda: self._spin(probe))   # the first launch loads the code object
        ms = self._timed(lambda: self._spin(probe))
        assert ms > 0.01, f"stream_order harness: {probe} delay units took {ms} ms"
        if ms < 1.0:   # a second, longer probe: the first is launch overhead more than spin
            probe = int(probe * 4.0 / ms)
            ms = self._timed(lambda: self._spin(probe))
        return probe / ms

    def sleep(self, ms: float):
        """Enqueue a delay of ``ms`` on the current stream: a bounded spin, never more than MAX_DELAY_MS."""
        assert 0 < ms <= MAX_DELAY_MS
        self._spin(max(1, int(ms * self.units_per_ms)))

    def _launch_latency(self) -> float:
        """(b): host time from the enqueue of an empty kernel on an idle side stream to its completion, median of 20 (>= its enqueue-to-start latency)."""
        s, t, ev = torch.cuda.Stream(self.device), torch.zeros(1, device=self.device), torch.cuda.Event()
        vals = []
        for i in range(24):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(s):
                t.zero_()
                ev.record()
            ev.synchronize()
            vals.append((time.perf_counter() - t0) * 1e3)
        return float(statistics.median(vals[4:]))

    def delay_for(self, a_ms: float) -> float:
        d = max(MIN_DELAY_MS, 20.0 * a_ms, 100.0 * self.launch_ms)
        assert d <= MAX_DELAY_MS, (f"stream_order harness: the row takes {a_ms:.3f} ms and an empty launch {self.launch_ms:.4f} ms: the delay would be {d:.1f} ms, past "
                                   f"the {MAX_DELAY_MS} ms cap -- the row's shape is too large for this harness")
        return d

    # -- one row
    def upload(self, ops: dict) -> dict:
        return {n: t.to(self.device) for n, t in ops.items()}

    def reference(self, R, case: StreamCase) -> Ref:
        """Step 1, on the default stream with ``R`` (a default renderer); the second call is timed: (a)."""
        ops = self.upload({**case.early, **case.late})
        torch.cuda.synchronize()
        outs = tuple(o.clone() for o in case.call(R, ops))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        again = case.call(R, ops)
        e1.record()
        torch.cuda.synchronize()
        assert len(again) == len(outs) and all(same_bits(a, b) for a, b in zip(again, outs)), "stream_order harness: the row's call is not repeatable in ordinary placement"
        return Ref(outs, float(e0.elapsed_time(e1)))

    def warm(self, R, case: StreamCase, stream):
        """One call in complete placement on ``stream``.  The context re-lays its scratch out when the geometry changes and builds tables at a geometry's first use,
        both behind a device synchronisation: a call that has to do so waits for the delay on the host, and then tells nothing."""
        ops = self.upload({**case.early, **case.late})
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            case.call(R, ops)
        torch.cuda.synchronize()

    def run(self, R, case: StreamCase, ref: Ref, current, consumer=None, order=None, warm=None) -> dict:
        """Steps 2 - 6.  ``current``: the stream that is current for the producer and the call; ``order(R)``: called after the wrapper (placement B's
        ``ordered_after``); ``consumer``: the stream that clones the outputs (default ``current``); ``warm``: the stream of a warm-up call (``warm()``) in front.
        Returns {"mismatch": [output indices], "delay_ms", "a_ms", "b_ms"}."""
        if warm is not None:
            self.warm(R, case, warm)
        early = self.upload(case.early)
        late = {n: poisoned_like(t, self.device) for n, t in case.late.items()}
        pinned = {n: t.pin_memory() for n, t in case.late.items()}
        delay = self.delay_for(ref.a_ms)
        copied = torch.cuda.Event()
        torch.cuda.synchronize()
        with torch.cuda.stream(current):
            self.sleep(delay)
            for n, t in late.items():
                t.copy_(pinned[n], non_blocking=True)
            copied.record()
            outs = tuple(case.call(R, {**early, **late}))
            still_busy = not copied.query()
            if order is not None:
                order(R)
        with torch.cuda.stream(consumer if consumer is not None else current):
            clones = [o.clone() for o in outs]
        torch.cuda.synchronize()
        assert still_busy or case.host_sync, (f"stream_order harness: the {delay:.1f} ms delay had run out when the wrapper returned: the run cannot tell an ordered call "
                                              "from an unordered one")
        assert len(clones) == len(ref.outs), "stream_order harness: the call returned another number of outputs than its reference"
        return {"mismatch": [i for i, (a, b) in enumerate(zip(clones, ref.outs)) if not same_bits(a, b)], "delay_ms": delay, "a_ms": ref.a_ms, "b_ms": self.launch_ms}

    def known_bad(self, other=None) -> StreamCase:
        """The stand-in every placement must catch: a torch-only op issued on another stream (``other``; default a stream of the harness) that waits for nothing."""
        def call(R, o):
            bad = other if other is not None else self.bad_stream
            out = torch.empty_like(o["x"])
            with torch.cuda.stream(bad):
                torch.mul(o["x"], 2, out=out)
            out.record_stream(bad)
            torch.cuda.current_stream().wait_stream(bad)   # the consumer sees the finished product of an operand read too early
            return (out,)
        return StreamCase({"x": A.rnd((64, 64), 5)}, {}, call, ("x",))

    def sees_race(self, producer, other) -> bool:
        """Does an unordered op on ``other`` show behind a late producer on ``producer``?  Two streams the runtime has put on one hardware queue run in enqueue
        order whatever the program says (HIP opens four per process by default): such a pair hides every ordering fault, and the tests do not use it."""
        case = self.known_bad(other)
        if self._bad_ref is None:
            self._bad_ref = self.reference(None, case)
        return bool(self.run(None, case, self._bad_ref, current=producer)["mismatch"])


# ---------------------------------------------------------------------------------------------------------------- the table
ROWS = []   # (id, build(R) -> StreamCase, names of the functions the row goes through)


def row(rid, covers):
    def deco(fn):
        ROWS.append((rid, fn, tuple(covers)))
        return fn
    return deco


def from_arena(aid, covers, early=()):
    """A row of tests/test_hip_arena.py as a stream row: its input buffers are the operands (``early`` names the ones that are not payload), its ``wrapper`` the call."""
    build = dict(A.ROWS)[aid]

    def make(R):
        c = build(R._L)
        ins = {b.name: b.data for b in c.bufs if b.role == "input"}
        assert set(early) <= set(ins), (aid, early)
        bits16 = {n for n, a in ins.items() if a.dtype == np.int16}

        def call(R, o):
            return tuple(c.wrapper(R, {n: (o[n].view(torch.int16) if n in bits16 else o[n]) for n in ins}).values())
        late = {n: a for n, a in ins.items() if n not in early}
        return StreamCase(late, {n: ins[n] for n in early}, call, tuple(late))
    ROWS.append((aid, make, tuple(covers)))


for _m in ("bf16x3", "fp16x2"):
    from_arena(f"gemm-{_m}-257x48x255-b1", ("linear_x3", "gemm_x3_pack"))
    from_arena(f"attn-{_m}-T65", ("attention_x3",))
    from_arena(f"conv-epi-{_m}", ("conv3x3_epi", "_conv3x3_pack"))
    from_arena(f"depthpro-head-{_m}", ("depthpro_head", "depthpro_head_pack"))
from_arena("gemm-bf16x3-257x48x255-gelu", ("linear_x3", "gemm_x3_pack"))
from_arena("attn-4-T65", ("attention_f32",))
from_arena("attn-8-T65", ("attention_f32",))
for _k in ("k3s1", "k3s2", "t4s2"):
    from_arena(f"conv-ifn-{_k}", ("conv_ifn", "conv_ifn_pack"))
from_arena("dpt-head-conv-f32", ("dpt_head_conv", "dpt_head_conv_pack"))
from_arena("neck-poly", ("neck_poly_conv", "neck_poly_pack"))
from_arena("head-upconv-gather", ("head_upconv_gather",))
from_arena("head-conv-gather", ("dpt_head_conv", "head_conv_gather_pack"))
from_arena("groupnorm-c64-p7", ("groupnorm",))
from_arena("layernorm-f32-384-r5", ("add_layernorm",), early=("gamma", "beta"))    # norm.weight / norm.bias: long-lived module parameters
from_arena("layernorm-bf16-384-r5", ("add_layernorm",), early=("gamma", "beta"))
from_arena("upsample-f32", ("upsample_bilinear",))
from_arena("upsample-bf16", ("upsample_bilinear",))
from_arena("bias-act", ("bias_act",))
from_arena("upsample-bias", ("upsample_bilinear_bias",))
from_arena("head-tail", ("dpt_head_tail",))
from_arena("head-tail-act", ("dpt_head_tail",))
from_arena("depth-to-space", ("depth_to_space_bias",))
from_arena("patchify", ("patchify",))
from_arena("im2col-c3", ("im2col",))
from_arena("maxpool", ("maxpool3x3_s2",))
from_arena("depthpro-preprocess", ("depthpro_preprocess",))
from_arena("depthpro-post", ("depthpro_post",))
from_arena("depthpro-patches", ("depthpro_patches",))
from_arena("depthpro-merge", ("depthpro_merge",))
from_arena("zoedepth-preprocess-37x53", ("zoedepth_preprocess",), early=("table",))
from_arena("zoedepth-post", ("zoedepth_post",))
from_arena("zoedepth-attractor", ("zoedepth_attractor",))
from_arena("zoedepth-bins", ("zoedepth_bins",), early=("table",))
from_arena("depth-preprocess-f32", ("depth_preprocess",))
from_arena("depth-preprocess-bf16", ("depth_preprocess",))
from_arena("depth-preprocess-pil", ("depth_preprocess_pil",))
from_arena("resize-pil-bicubic", ("resize_pil_bicubic_u8",))
from_arena("depth-handoff", ("depth_handoff",))
from_arena("tile-gather", ("tile_gather_cubic_u8",), early=("origins",))
from_arena("tile-blend", ("tile_blend",), early=("pred_off", "tile_tab", "w_pool"))
from_arena("depth-normalize-pclip", ("depth_normalize_pclip",))


def conv_row(fam, Cin, Cout, B, H, W):
    def build(R):
        def call(R, o):
            return (getattr(R, f"conv3x3_{fam}")(A.nchw(o["X"]), getattr(R, f"conv3x3_{fam}_pack")(o["W"]), Cout),)
        return StreamCase({"X": A.ints((B, H, W, Cin)), "W": A.wints((Cout, Cin, 3, 3))}, {}, call, ("X", "W"))
    return build


for _fam, _s in (("x3", (48, 32, 2, 13, 47)), ("s1_x2", (48, 32, 2, 13, 47)), ("x2", (48, 32, 2, 13, 47)), ("s2_x3", (48, 128, 2, 25, 93)), ("s2_x2", (48, 128, 2, 25, 93))):
    ROWS.append((f"conv-{_fam}", conv_row(_fam, *_s), ("_conv3x3", "_conv3x3_pack")))


def pack_row(shapes, fn):
    """A ``*_pack`` wrapper on late float weights: the outputs are the image (and the bias copy where the wrapper returns one)."""
    def build(R):
        ws = {f"w{i}": A.wints(s) for i, s in enumerate(shapes)}

        def call(R, o):
            got = fn(R, *[o[n] for n in ws])
            return tuple(t for t in (got if isinstance(got, tuple) else (got,)) if torch.is_tensor(t))
        return StreamCase(ws, {}, call, tuple(ws))
    return build


for _rid, _cov, _shapes, _fn in (
        ("pack-gemm-bf16x3", "gemm_x3_pack", [(255, 48)], lambda R, w: R.gemm_x3_pack(w, "bf16x3")),
        ("pack-gemm-fp16x2", "gemm_x3_pack", [(255, 48)], lambda R, w: R.gemm_x3_pack(w, "fp16x2")),
        ("pack-conv-x2", "_conv3x3_pack", [(64, 48, 3, 3)], lambda R, w: R.conv3x3_x2_pack(w)),
        ("pack-conv-x3", "_conv3x3_pack", [(256, 48, 3, 3)], lambda R, w: R.conv3x3_x3_pack(w)),
        ("pack-conv-s2_x3", "_conv3x3_pack", [(256, 48, 3, 3)], lambda R, w: R.conv3x3_s2_x3_pack(w)),
        ("pack-conv-s1_x2", "_conv3x3_pack", [(256, 48, 3, 3)], lambda R, w: R.conv3x3_s1_x2_pack(w)),
        ("pack-conv-s2_x2", "_conv3x3_pack", [(256, 48, 3, 3)], lambda R, w: R.conv3x3_s2_x2_pack(w)),
        ("pack-conv-ifn-k3s1", "conv_ifn_pack", [(96, 48, 3, 3)], lambda R, w: R.conv_ifn_pack(0, w)),
        ("pack-conv-ifn-k3s2", "conv_ifn_pack", [(64, 16, 3, 3)], lambda R, w: R.conv_ifn_pack(1, w)),
        ("pack-conv-ifn-t4s2", "conv_ifn_pack", [(48, 32, 4, 4)], lambda R, w: R.conv_ifn_pack(2, w)),
        ("pack-depthpro-head-bf16x3", "depthpro_head_pack", [(16, 32, 48)], lambda R, w: R.depthpro_head_pack(w, "bf16x3")),
        ("pack-depthpro-head-fp16x2", "depthpro_head_pack", [(16, 32, 48)], lambda R, w: R.depthpro_head_pack(w, "fp16x2")),
        ("pack-dpt-head-conv", "dpt_head_conv_pack", [(32, 64, 3, 3)], lambda R, w: R.dpt_head_conv_pack(w)),
        ("pack-head-conv-gather", "head_conv_gather_pack", [(288, 32), (288,)], lambda R, w, b: R.head_conv_gather_pack(w, b)),
        ("pack-neck-poly", "neck_poly_pack", [(36, 64, 48), (36, 64)], lambda R, w, b: R.neck_poly_pack(w, b, 4))):
    ROWS.append((_rid, pack_row(_shapes, _fn), (_cov,)))


# ---- uint8 glue, the up-scale stage, the diagnostics
def u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def simple(rid, covers, late, fn, early=None, host_sync=False):
    """A row whose call is ``fn(R, ops) -> tensor or tuple``; ``late`` / ``early``: dicts, or callables that build them."""
    def build(R):
        la = late() if callable(late) else late
        ea = (early() if callable(early) else early) or {}

        def call(R, o):
            got = fn(R, o)
            return tuple(got) if isinstance(got, (tuple, list)) else (got,)
        return StreamCase(la, ea, call, tuple(la), host_sync)
    ROWS.append((rid, build, tuple(covers)))


simple("resize-cubic-u8", ("resize_cubic_u8",), {"src": u8((37, 53, 3), 1)}, lambda R, o: R.resize_cubic_u8(o["src"], 23, 31))
simple("resize-cubic-u8-gray", ("resize_cubic_u8",), {"src": u8((37, 53), 2)}, lambda R, o: R.resize_cubic_u8(o["src"], 50, 71))
simple("resize-linear-u8", ("resize_linear_u8",), {"src": u8((37, 53, 3), 3)}, lambda R, o: R.resize_linear_u8(o["src"], 50, 71))
simple("resize-area-u8", ("resize_area_u8",), {"src": u8((37, 53, 3), 4)}, lambda R, o: R.resize_area_u8(o["src"], 18, 26))
simple("nv12-to-bgr", ("nv12_to_bgr",), {"nv12": u8((27, 34), 5)}, lambda R, o: R.nv12_to_bgr(o["nv12"]))
simple("bgr-to-nv12", ("bgr_to_nv12",), {"bgr": u8((18, 34, 3), 6)}, lambda R, o: R.bgr_to_nv12(o["bgr"]))
simple("add-weighted-u8", ("add_weighted_u8",), {"a": u8((19, 23, 3), 7), "b": u8((19, 23, 3), 8)}, lambda R, o: R.add_weighted_u8(o["a"], 0.7, o["b"], 0.3, 1.0))
simple("esr-preprocess", ("esr_preprocess",), {"frame": u8((19, 23, 3), 9)}, lambda R, o: R.esr_preprocess(o["frame"], 2, 3, 12, 16, torch.float16))
simple("esr-postprocess", ("esr_postprocess",), {"pred": A.rnd((1, 3, 12, 17), 10, 0.5) + 0.5}, lambda R, o: R.esr_postprocess(o["pred"]))
simple("format-3d-output", ("format_3d_output",), {"l": u8((27, 48, 3), 11), "r": u8((27, 48, 3), 12)}, lambda R, o: R.format_3d_output(o["l"], o["r"], "Full-SBS"))
simple("heal-missing-pixels", ("heal_missing_pixels",),
       {"w": np.abs(A.rnd((3, 19, 23), 13, 0.3)), "o": np.abs(A.rnd((3, 19, 23), 14, 0.3)), "e": (A.rnd((1, 19, 23), 15) > 0.5).astype(np.float32)},
       lambda R, o: R.heal_missing_pixels(o["w"], o["o"], o["e"], 0.5))
simple("torch-math", ("torch_math",), {"x": np.abs(A.rnd((1031,), 16)) + 0.01},
       lambda R, o: (R.torch_math("pow", o["x"], 0.85), R.torch_math("sigmoid", o["x"]), R.torch_math("sqrt", o["x"])))
simple("torch-math-aten", ("torch_math_aten",), {"x": np.abs(A.rnd((1031,), 17)) + 0.01},
       lambda R, o: (R.torch_math_aten("pow", o["x"], 0.85, 8), R.torch_math_aten("sigmoid", o["x"], 0.0, 8)))
simple("quantiles", ("quantiles",), {"plane": A.rnd((54, 96), 18)}, lambda R, o: torch.tensor(R.quantiles(o["plane"], [0.02, 0.98]), dtype=torch.float64), host_sync=True)
simple("subject-depth", ("subject_depth",), {"plane": np.abs(A.rnd((54, 96), 19, 0.3))}, lambda R, o: torch.tensor([R.subject_depth(o["plane"])], dtype=torch.float64),
       host_sync=True)


def _bars_frame(seed):
    f = u8((54, 96, 3), seed)
    f[:6] = 0
    f[-6:] = 0
    return f


simple("detect-black-bars", ("detect_black_bars",), {"frame": _bars_frame(20)}, lambda R, o: torch.tensor(R.detect_black_bars(o["frame"]), dtype=torch.int64), host_sync=True)


def _f16_nhwc(shape, seed, scale=1.0):
    return torch.from_numpy(A.rnd(shape, seed, scale)).to(torch.float16)


def _esr_weights():
    from visiondepth3d_amd.upscale import conv_weight_fragments, dense_weight_fragments, head_weight_matrix
    g = torch.Generator().manual_seed(21)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return dict(w_c64=conv_weight_fragments(r(64, 64, 3, 3) * 0.05), b64=r(64) * 0.1, s64=r(64).abs() * 0.25, w_head=head_weight_matrix(r(64, 3, 3, 3) * 0.2),
                w_dense=dense_weight_fragments(r(32, 64, 3, 3) * 0.05), b32=r(32) * 0.1)


ESR_HW = (9, 33)
simple("conv3x3-c64", ("conv3x3_c64",), lambda: {"x": _f16_nhwc((1, *ESR_HW, 64), 22)}, lambda R, o: R.conv3x3_c64(A.nchw(o["x"]), o["w_c64"], o["b64"], o["s64"]), _esr_weights)
simple("conv3x3-head", ("conv3x3_head",), lambda: {"x": _f16_nhwc((1, *ESR_HW, 3), 23)}, lambda R, o: R.conv3x3_head(A.nchw(o["x"]), o["w_head"], o["b64"], o["s64"]), _esr_weights)
simple("esr-tail", ("esr_tail",), lambda: {"t": _f16_nhwc((1, *ESR_HW, 64), 24), "x": _f16_nhwc((1, *ESR_HW, 3), 25)}, lambda R, o: R.esr_tail(A.nchw(o["t"]), A.nchw(o["x"]), 2))


def _dense(R, o):
    out = A.nchw(torch.empty((1, *ESR_HW, 32), dtype=torch.float16, device=o["x"].device))
    return R.conv3x3_dense(A.nchw(o["x"]), 64, o["w_dense"], o["b32"], 32, out, 0, slope=0.2, r1=A.nchw(o["r1"]), alpha=0.5)


simple("conv3x3-dense", ("conv3x3_dense",), lambda: {"x": _f16_nhwc((1, *ESR_HW, 64), 26), "r1": _f16_nhwc((1, *ESR_HW, 32), 27)}, _dense, _esr_weights)
simple("nhwc-f16-to-planar3", ("nhwc_f16_to_planar3",), lambda: {"t": _f16_nhwc((1, *ESR_HW, 32), 28)}, lambda R, o: R.nhwc_f16_to_planar3(A.nchw(o["t"])))


# ---- letterbox
def _lb_frames(seed):
    f = u8((2, 36, 64, 3), seed)
    f[:, :4] = 0
    f[:, -4:] = 0
    return f


simple("letterbox-stats", ("letterbox_stats",), {"frames": _lb_frames(30)}, lambda R, o: tuple(R.letterbox_stats(o["frames"]).values()))


def _lb_track(R, o):
    R.letterbox_state_reset()   # a fresh tracker per run: the reference and the late run start from one state
    return R.letterbox_track(o["frames"], 36)


simple("letterbox-track", ("letterbox_track", "letterbox_state_reset"), {"frames": _lb_frames(31)}, _lb_track)
simple("canny-u8", ("canny_u8",), {"gray": u8((2, 36, 64), 32)}, lambda R, o: R.canny_u8(o["gray"], want_counts=True))
simple("canny-hysteresis-u8", ("canny_hysteresis_u8",), {}, lambda R, o: R.canny_hysteresis_u8(o["classes"], want_counts=True),
       {"classes": np.random.default_rng(33).integers(0, 3, (2, 36, 64)).astype(np.uint8)})   # a class map, not samples: early
simple("depth-letterbox-fill", ("depth_letterbox_fill",), {"depth": u8((2, 36, 64), 34)}, lambda R, o: R.depth_letterbox_fill(o["depth"], o["bars"]),
       {"bars": np.array([[4, 4], [3, 5]], np.int32)})


# ---- previews and the interpolation glue
def _pv():
    from visiondepth3d_amd import preview_utils
    return preview_utils


_LUT = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], 1).astype(np.uint8)
simple("preview-image", ("preview_image",), {"l": u8((27, 48, 3), 40), "r": u8((27, 48, 3), 41)}, lambda R, o: _pv().preview_image(R, "Passive Interlaced", o["l"], o["r"]))
simple("preview-heatmap", ("preview_heatmap",), {"shift": A.rnd((1, 27, 48), 42, 3.0)}, lambda R, o: _pv().preview_heatmap(R, "Shift Heatmap", o["shift"], _LUT),
       host_sync=True)   # the wrapper uploads its colour table from pageable memory: a copy the host waits for, on the producer's stream
simple("preview-arrows", ("preview_arrows",), {"l": u8((45, 64, 3), 43)}, lambda R, o: _pv().preview_arrows(R, o["l"], o["shift"]),
       {"shift": A.rnd((1, 45, 64), 44, 1.5)})   # the shift map places the arrows: early


def _run_rife(R, o):
    from visiondepth3d_amd.upscale import run_rife
    return tuple(run_rife(R, lambda x: x[:, :3] * 0.5 + x[:, 3:] * 0.5, o["f1"], o["f2"], 3))


simple("run-rife", ("run_rife",), {"f1": u8((33, 65, 3), 45), "f2": u8((33, 65, 3), 46)}, _run_rife)


def _rife_ops():
    g = RG.family(33, 65)
    t, state = RG.update_inputs(33, 65, 2)
    return dict(x6=g["x6"], st=RG.make_state(g["flow"], g["mask"]), t=t, state=state)


def _rife_late(*names):
    return lambda: {n: _rife_ops()[n] for n in names}


_rife_early = _rife_late


simple("rife-warp-pack", ("rife_warp_pack",), _rife_late("x6"),
       lambda R, o: R.rife_warp_pack(o["x6"], o["st"], 2, torch.empty((RG.BATCH, 32, 48, 16), device=o["x6"].device)), _rife_early("st"))   # the flow state places the samples: early
simple("rife-update", ("rife_update",), _rife_late("t"), lambda R, o: R.rife_update(o["t"], o["state"].clone(), 2, False, 33, 65), _rife_early("state"))
simple("rife-blend", ("rife_blend",), _rife_late("x6"), lambda R, o: R.rife_blend(o["x6"], o["st"], torch.empty((RG.BATCH, 3, 33, 65), device=o["x6"].device)), _rife_early("st"))


# ---- the stateful rows: a fresh state per run, so the reference and the late run start alike.  The depth drives the warp's addresses: early.
SH, SW = 216, 384   # __graft_entry__.smoke()'s frame
RENDER_KW = dict(output_format="Half-SBS", output_height=SH, fg_shift=10.0, mg_shift=-2.5, bg_shift=-5.0, sharpness_factor=0.15, dof_strength=2.0, feather_strength=10.0,
                 blur_ksize=9, use_subject_tracking=True, use_floating_window=True)


def render_params():
    from visiondepth3d_amd.params import render_kwargs_to_params
    return render_kwargs_to_params(SW, SH, **RENDER_KW)


def synth_pair(i):
    from visiondepth3d_amd import synth
    return synth.synth_frame(i, SH, SW)


def _pixel_shift(R, o):
    from visiondepth3d_amd._abi import ShiftParams
    R.reset_state()
    return R.pixel_shift(o["frame"], o["depth"], 96, 54, ShiftParams.defaults(10, -2.5, -5), want_shift=True)


simple("pixel-shift", ("pixel_shift",), {"frame": np.abs(A.rnd((3, 54, 96), 50, 0.3)).clip(0, 1)}, _pixel_shift, {"depth": np.random.default_rng(51).random((1, 54, 96), dtype=np.float32)})


def render_row(i):
    def build(R):
        p = render_params()
        f, d = synth_pair(i)

        def call(R, o):
            R.reset_state()
            R.new_clip()
            return (R.render_frame(o["frame"], o["depth"], p),)
        return StreamCase({"frame": f}, {"depth": d}, call, ("frame",), host_sync=True)   # vd3d_render_frame reads the frame's scalars back
    return build


ROWS.append(("render-frame", render_row(1), ("render_frame",)))


def finish_row(seed):
    def build(R):
        p = render_params()
        rng = np.random.default_rng(seed)
        left, right = (rng.integers(0, 256, (p.warp_h, p.warp_w, 3), dtype=np.uint8) for _ in range(2))
        dn = rng.random((p.eye_h, p.eye_w), dtype=np.float32)
        return StreamCase({"left": left, "right": right}, {"dn": dn}, lambda R, o: (R.finish_frame(o["left"], o["right"], o["dn"], p, 0.4),), ("left", "right"))
    return build


ROWS.append(("finish-frame", finish_row(52), ("finish_frame",)))

CASES = {rid: build for rid, build, _ in ROWS}

# functions that call ``_enter`` and have no row, each with its reason; the list may not grow
EXCLUDED = {
    "shard2_p0": "sharded step protocol: driven by sharded.ChunkSharder on streams of its own, tests/test_hip_sharded*.py and the step-path parity tests",
    "shard2_set_crops": "sharded step protocol: its operand is the int32 crop table, early by the safety rule",
    "shard2_p1": "sharded step protocol (as shard2_p0)",
    "shard2_p1_batch": "sharded step protocol (as shard2_p0)",
    "shard2_p3": "sharded step protocol: no payload operand, writes the int64 reduction record",
    "shard2_p3_batch": "sharded step protocol (as shard2_p3)",
    "shard2_r1": "sharded step protocol: replays the gathered reduction records",
    "shard2_r2": "sharded step protocol: its operand is the int64 record table, early by the safety rule",
    "shard_pixels": "pixel-overlap entry point: runs on the context's own pixel streams, ordered by join_pixels / wait_pixels; tests/test_hip_sharded*.py",
    "tdf_plane_export": "chunk-boundary hand-off of the sharded clip: reads filter state, no payload operand",
    "tdf_plane_import": "chunk-boundary hand-off of the sharded clip: writes the filter state the next frame's warp reads",
    "letterbox_state_export": "no operand; synchronises the host before it returns",
    "letterbox_state_import": "tracker state: early by the safety rule, so nothing of it can be late",
}


# ---------------------------------------------------------------------------------------------------------------- the host checks
SOURCES = ("visiondepth3d_amd/render_3d.py", "visiondepth3d_amd/upscale.py", "visiondepth3d_amd/preview_utils.py")

# pointer arguments that need not be among ``_enter``'s, by (function, name), each with its reason
STATIC_EXCEPTIONS = {
    ("add_layernorm", "norm.weight"): "long-lived module parameter: finished long before the forward, never freed during it",
    ("add_layernorm", "norm.bias"): "long-lived module parameter (as norm.weight)",
    ("letterbox_state_export", "g"): "allocated behind _enter(), and the function synchronises before it returns",
}
NO_ENTER_NEEDED = {"view": "the copy-out helper of debug_planes (tests only), which synchronises before and after"}


def _functions(src: str):
    tree = ast.parse(src)
    for node in ast.walk(tree):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            yield node


def _own_nodes(fn):
    """The nodes of ``fn`` without those of nested ``def``s (lambdas stay: they are part of the statement that holds them)."""
    stack = list(ast.iter_child_nodes(fn))
    while stack:
        n = stack.pop()
        yield n
        if not isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)):
            stack.extend(ast.iter_child_nodes(n))


def _is_enter(call):
    return isinstance(call, ast.Call) and isinstance(call.func, ast.Attribute) and call.func.attr == "_enter"


def _name_of(e):
    """``x`` -> "x"; ``x[i]`` / ``x["k"]`` -> "x"; ``a.b`` -> "a.b"; anything else -> None."""
    if isinstance(e, ast.Name):
        return e.id
    if isinstance(e, ast.Subscript):
        return _name_of(e.value)
    if isinstance(e, ast.Attribute):
        b = _name_of(e.value)
        return None if b is None else f"{b}.{e.attr}"
    return None


def enter_callers(root=ROOT) -> dict:
    """{function name: file} of every function of SOURCES that calls ``_enter`` (``Renderer._enter`` itself aside)."""
    out = {}
    for rel in SOURCES:
        with open(os.path.join(root, rel)) as f:
            src = f.read()
        for fn in _functions(src):
            if fn.name != "_enter" and any(_is_enter(n) for n in _own_nodes(fn)):
                out[fn.name] = rel
    return out


def completeness_problems(root=ROOT) -> list:
    covered = {c for _, _, cov in ROWS for c in cov}
    callers = enter_callers(root)
    problems = [f"{rel}: {name} calls _enter and has neither a row in tests/stream_order.py ROWS nor a reason in EXCLUDED" for name, rel in sorted(callers.items())
                if name not in covered and name not in EXCLUDED]
    problems += [f"EXCLUDED names {name}, which also has a row" for name in sorted(EXCLUDED) if name in covered]
    problems += [f"{name} is named by ROWS / EXCLUDED and does not call _enter (renamed or removed?)" for name in sorted((covered | set(EXCLUDED)) - set(callers))]
    return problems


def _pointer_passes(fn):
    """(line, name) of every device pointer ``fn`` hands to the library: ``_ptr(x)``, ``x.data_ptr()``, and calls of a local ``p = lambda t: _ptr(t) ...``."""
    nodes = list(_own_nodes(fn))
    lam_params, ptr_lambdas, loop_vars = set(), set(), {}
    for n in nodes:
        if isinstance(n, ast.Lambda):
            lam_params |= {a.arg for a in n.args.args}
        if isinstance(n, ast.Assign) and isinstance(n.value, ast.Lambda) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
            if any(isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == "_ptr" for c in ast.walk(n.value)):
                ptr_lambdas.add(n.targets[0].id)
        if isinstance(n, ast.comprehension) and isinstance(n.target, ast.Name):
            loop_vars[n.target.id] = _name_of(n.iter)
    out = []
    for n in nodes:
        if not isinstance(n, ast.Call):
            continue
        arg = None
        if isinstance(n.func, ast.Name) and (n.func.id == "_ptr" or n.func.id in ptr_lambdas) and len(n.args) == 1:
            arg = n.args[0]
        elif isinstance(n.func, ast.Attribute) and n.func.attr == "data_ptr":
            arg = n.func.value
        if arg is None:
            continue
        name = _name_of(arg)
        if name in lam_params and not isinstance(arg, ast.Subscript):
            continue   # the lambda's own parameter: its call sites are collected instead
        name = loop_vars.get(name, name)
        out.append((n.lineno, name if name is not None else ast.unparse(arg)))
    return out


def _enter_names(fn):
    """(line of the first ``_enter``, the names it is given): plain names, ``*name`` (and the names of the expression ``name`` was assigned), names inside a starred
    expression."""
    nodes = list(_own_nodes(fn))
    assigned = {}
    for n in nodes:
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
            assigned.setdefault(n.targets[0].id, set()).update(_name_of(x) for x in ast.walk(n.value) if isinstance(x, (ast.Name, ast.Attribute)))
    line, names = None, set()
    for n in nodes:
        if not _is_enter(n):
            continue
        line = n.lineno if line is None else min(line, n.lineno)
        for a in n.args:
            if isinstance(a, ast.Starred):
                for x in ast.walk(a.value):
                    nm = _name_of(x) if isinstance(x, (ast.Name, ast.Attribute)) else None
                    if nm:
                        names.add(nm)
                        names |= {v for v in assigned.get(nm, ()) if v}
            else:
                nm = _name_of(a)
                if nm:
                    names.add(nm)
    return line, names


def static_problems(root=ROOT, sources=SOURCES) -> list:
    """For every function that hands a device pointer to the library: ``_enter`` is called before the first one, and every pointer's tensor is among its arguments."""
    problems = []
    for rel in sources:
        with open(os.path.join(root, rel)) as f:
            src = f.read()
        for fn in _functions(src):
            passes = _pointer_passes(fn)
            if not passes or fn.name == "_ptr":
                continue
            line, names = _enter_names(fn)
            if line is None:
                if fn.name not in NO_ENTER_NEEDED:
                    problems.append(f"{rel}:{fn.lineno}: {fn.name} passes device pointers to the library and never calls _enter")
                continue
            first = min(ln for ln, _ in passes)
            if line > first:
                problems.append(f"{rel}:{first}: {fn.name} takes a device pointer before its first _enter (line {line})")
            for ln, name in sorted(set(passes)):
                if name not in names and (fn.name, name) not in STATIC_EXCEPTIONS:
                    problems.append(f"{rel}:{ln}: {fn.name} passes '{name}' to the library and leaves it out of _enter({', '.join(sorted(names))})")
    return problems


def stub_renderer():
    """What a builder may ask of the renderer on the host: the library's size queries."""
    from visiondepth3d_amd import _lib
    return types.SimpleNamespace(_L=_lib.lib())
