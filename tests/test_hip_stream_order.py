"""GPU tests (-m gpu): every public wrapper behind a late producer on a side stream (tests/stream_order.py states the harness, its safety rule and the table).

Placement A: a default ``Renderer(0)`` built on the default stream, rows run in turn inside ``torch.cuda.stream(S1)``, ``S2`` and on the default stream again --
producer, call and consumer on that one stream, so only ``_enter``'s re-target orders the library's launches.  Placement B: ``Renderer(0, private_stream=True)``
with ``auto_order``: producer = the current stream, consumer = the current stream behind ``R.ordered_after()``, and once more a third stream behind
``R.ordered_after(stream=S3)``.  Every placement first runs the known-bad stand-in, which the harness must report.  Then: the caching allocator does not hand
out a block a queued kernel still owns, the hand-over event of ``vd3d_ctx_set_stream`` keeps two streams' calls on one context in order, and two contexts on two
streams compute what they compute serially."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_order as SO   # noqa: E402

IDS = [r for r, _, _ in SO.ROWS]


class Env:
    """The renderers, the streams and the references of the module.  The streams are chosen so that the harness can see what it is looking for: for every
    (producer, stream a mis-ordered launch would run on) pair the tests use, the known-bad stand-in -- ``torch.mul`` on that other stream, waiting for nothing -- is
    run once and must come back wrong.  A pair the runtime has put on one hardware queue is never wrong; then the next stream of PyTorch's pool is tried."""
    TRIES = 12

    def __init__(self):
        from visiondepth3d_amd.render_3d import Renderer
        assert torch.cuda.is_available()
        torch.cuda.set_device(0)
        self.D = torch.cuda.default_stream()
        assert torch.cuda.current_stream() == self.D
        self.R = Renderer(0)                                # built while the default stream is current
        self.h = h = SO.Harness(0)
        self.stand_in_log = []

        def sees(producer, other, what):
            ok = h.sees_race(producer, other)
            self.stand_in_log.append(f"STREAM stand-in {what}: {'caught' if ok else 'missed (one hardware queue): pair not used'}")
            print(self.stand_in_log[-1])
            return ok
        blind = "stream_order harness (not the library): no stream of PyTorch's pool shows torch.mul on an unordered stream behind a late producer on "
        # placement A: rows run on S1, S2, the default stream in turn; a wrapper that forgot _enter launches on the stream bound before: D, S1, S2
        self.S1 = next((s for s in (torch.cuda.Stream() for _ in range(self.TRIES)) if sees(s, self.D, "A producer S1 / unordered default stream")), None)
        assert self.S1 is not None, blind + "a side stream: the delay is not doing its job"
        self.S2 = next((s for s in (torch.cuda.Stream() for _ in range(self.TRIES))
                        if sees(s, self.S1, "A producer S2 / unordered S1") and sees(self.D, s, "A producer default stream / unordered S2")), None)
        assert self.S2 is not None, blind + "a second side stream: the delay is not doing its job"
        self.S3 = torch.cuda.Stream()
        self.turn = [self.S1, self.S2, self.D]
        self.n = 0
        # placement B: the producer is the current (default) stream, a mis-ordered launch runs on the renderer's own stream
        self.Rb = None
        for _ in range(self.TRIES):
            r = Renderer(0, private_stream=True)            # auto_order is the default
            if sees(self.D, r.stream, "B producer default stream / unordered private stream"):
                self.Rb = r
                break
            r.close()
        assert self.Rb is not None, blind + "the default stream with the renderer's private stream: the delay is not doing its job"
        self.refs, self.cases = {}, {}

    def case(self, rid):
        if rid not in self.cases:
            self.cases[rid] = SO.CASES[rid](self.R)
            SO.check_late_rule(self.cases[rid], rid)
        return self.cases[rid]

    def ref(self, rid):
        """Step 1, once per row: the default renderer on the default stream, shared by every placement and left unchanged."""
        if rid not in self.refs:
            self.refs[rid] = self.h.reference(self.R, self.case(rid))
        return self.refs[rid]

    def next_stream(self):
        """(the stream the context was bound to last, the stream of this row): S1, S2, the default stream, S1, ..."""
        prev, s = self.turn[(self.n - 1) % 3], self.turn[self.n % 3]
        self.n += 1
        return prev, s

    def placements(self):
        return {"A": dict(R=self.R, current=self.S1), "B": dict(R=self.Rb, current=torch.cuda.current_stream(), order=lambda R: R.ordered_after()),
                "B3": dict(R=self.Rb, current=torch.cuda.current_stream(), consumer=self.S3, order=lambda R: R.ordered_after(stream=self.S3))}

    def stand_in(self, placement):
        """The stand-in was caught for every pair of the placement when the streams were chosen (the constructor asserts it); B3 differs from B in its consumer only."""
        assert self.S1 is not None and self.S2 is not None and self.Rb is not None and placement in ("A", "B", "B3")


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    torch.cuda.synchronize()
    e.R.close()
    e.Rb.close()


def _report(record_property, rid, placement, got):
    for k in ("a_ms", "b_ms", "delay_ms"):
        record_property(k, round(got[k], 5))
    print(f"STREAM {rid} placement {placement}: a {got['a_ms'] * 1e3:.1f} us b {got['b_ms'] * 1e3:.1f} us delay {got['delay_ms']:.2f} ms mismatch {got['mismatch']}")


def test_known_bad_stand_in_is_caught_in_every_placement(env):
    """Once more, on the streams the module settled on: every (producer, other stream) pair of placements A and B reports the stand-in as a mismatch."""
    pairs = [("A", env.S1, env.D), ("A", env.S2, env.S1), ("A", env.D, env.S2), ("B", env.D, env.Rb.stream)]
    missed = [(p, i) for i, (p, producer, other) in enumerate(pairs) if not env.h.sees_race(producer, other)]
    assert not missed, f"stream_order harness (not the library): the stand-in was not caught for (placement, pair) {missed}: the delay is not doing its job"


@pytest.mark.parametrize("rid", IDS)
def test_placement_a_default_renderer_on_side_streams(env, record_property, rid):
    env.stand_in("A")
    case, ref = env.case(rid), env.ref(rid)
    prev, s = env.next_stream()   # the warm-up leaves the context on the stream before: the late call's _enter re-targets it, in both directions over the rows
    got = env.h.run(env.R, case, ref, current=s, warm=prev)
    _report(record_property, rid, "A", got)
    assert not got["mismatch"], f"{rid}: outputs {got['mismatch']} differ from ordinary placement when the operands arrive {got['delay_ms']:.1f} ms late on a side stream"


@pytest.mark.parametrize("rid", IDS)
def test_placement_b_private_stream_renderer(env, record_property, rid):
    env.stand_in("B")
    case, ref = env.case(rid), env.ref(rid)
    got = env.h.run(env.Rb, case, ref, current=torch.cuda.current_stream(), order=lambda R: R.ordered_after(), warm=torch.cuda.current_stream())
    _report(record_property, rid, "B", got)
    assert not got["mismatch"], f"{rid}: outputs {got['mismatch']} differ from ordinary placement on a private-stream renderer behind a {got['delay_ms']:.1f} ms late producer"


@pytest.mark.parametrize("rid", IDS)
def test_placement_b_consumer_on_a_third_stream(env, record_property, rid):
    env.stand_in("B3")
    case, ref = env.case(rid), env.ref(rid)
    got = env.h.run(env.Rb, case, ref, current=torch.cuda.current_stream(), consumer=env.S3, order=lambda R: R.ordered_after(stream=env.S3), warm=torch.cuda.current_stream())
    _report(record_property, rid, "B3", got)
    assert not got["mismatch"], f"{rid}: outputs {got['mismatch']} differ from ordinary placement for a consumer on a third stream behind ordered_after(stream=...)"


# ---------------------------------------------------------------------------------------------------------------- allocator lifetime
def _row_call(rid):
    def prepare(env, R):
        case = env.case(rid)
        ops = env.h.upload({**case.early, **case.late})
        return lambda: case.call(R, ops)[0]
    return prepare


def _linear_x3(env, R):
    x, w = torch.from_numpy(SO.A.ints((257, 48))).cuda(), torch.from_numpy(SO.A.wints((255, 48))).cuda()
    img = R.gemm_x3_pack(w)   # packed before the probe: the call under it allocates its output and nothing else
    return lambda: R.linear_x3(x, img, 255)


def _conv_x3(env, R):
    x, w = SO.A.nchw(torch.from_numpy(SO.A.ints((2, 13, 47, 48))).cuda()), torch.from_numpy(SO.A.wints((32, 48, 3, 3))).cuda()
    img = R.conv3x3_x3_pack(w)
    return lambda: R.conv3x3_x3(x, img, 32)


# calls that allocate their output and nothing else, so the freed block has no free neighbour of the call's own to merge with
ALLOC = {"linear_x3": _linear_x3, "conv3x3_x3": _conv_x3, "attention_f32": _row_call("attn-4-T65"), "depth_handoff": _row_call("depth-handoff"),
         "resize_cubic_u8": _row_call("resize-cubic-u8"), "preview_image": _row_call("preview-image"), "esr_postprocess": _row_call("esr-postprocess"),
         "upsample_bilinear": _row_call("upsample-f32")}


def _alloc_probe(env, R, name):
    """The issue's sequence: delay on the current stream, call, note the output's block, drop it, allocate the same size at once.  Returns (p, the new pointer)."""
    call = ALLOC[name](env, R)
    call()   # warm-up: the context's scratch has this geometry now (Harness.warm)
    torch.cuda.synchronize()
    env.h.sleep(SO.MIN_DELAY_MS)
    out = call()
    p, n, dt = out.data_ptr(), out.numel(), out.dtype
    del out
    t = torch.empty(n, dtype=dt, device="cuda")
    q = t.data_ptr()
    torch.cuda.synchronize()
    return p, q


@pytest.mark.parametrize("name", sorted(ALLOC))
def test_allocator_does_not_recycle_an_output_a_queued_kernel_owns(env, name):
    p, q = _alloc_probe(env, env.R, name)
    assert q == p, (f"allocator probe (not the library): with a default renderer on one stream the freed output of {name} at {p:#x} was not handed out again ({q:#x}): "
                    "the probe is blind")
    p, q = _alloc_probe(env, env.Rb, name)
    assert q != p, f"{name}: the output's block {p:#x} was handed out again while the private stream's kernel was still queued behind the delay (record_stream missing)"


def _non_contiguous(t):
    """The same values in memory the wrapper has to copy: every second element of a buffer twice as wide."""
    wide = torch.empty(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    v = wide[..., ::2]
    v.copy_(t)
    return v


COPY_ROWS = {   # rows whose wrapper makes a device copy of an argument that is non-contiguous or of another dtype: (row, operand, how)
    "depth-normalize-pclip": ("planes", lambda t: t.double()),                 # planes.to(float32)
    "heal-missing-pixels": ("w", _non_contiguous),                              # .contiguous()
    "resize-cubic-u8": ("src", lambda t: t.permute(1, 0, 2).contiguous().permute(1, 0, 2)),   # column-major rows: .contiguous()
    "depth-handoff": ("pred", lambda t: t.double()),
    "pixel-shift": ("frame", lambda t: t.half()),
}


def _copy_probe(env, R, rid, monkeypatch):
    """Track the tensors ``Tensor.to`` / ``Tensor.contiguous`` allocate during the call; return (their pointers, the pointers handed out right after it)."""
    name, how = COPY_ROWS[rid]
    case = env.case(rid)
    ops = env.h.upload({**case.early, **case.late})
    ops[name] = how(ops[name])
    case.call(R, ops)   # warm-up (Harness.warm)
    torch.cuda.synchronize()
    made = []
    real_to, real_contig = torch.Tensor.to, torch.Tensor.contiguous

    def track(real):
        def shim(self, *a, **k):
            r = real(self, *a, **k)
            if r.is_cuda and r.numel() and r.data_ptr() != self.data_ptr():
                made.append((r.data_ptr(), r.numel() * r.element_size()))
            return r
        return shim
    env.h.sleep(SO.MIN_DELAY_MS)
    monkeypatch.setattr(torch.Tensor, "to", track(real_to))
    monkeypatch.setattr(torch.Tensor, "contiguous", track(real_contig))
    try:
        outs = case.call(R, ops)
    finally:
        monkeypatch.setattr(torch.Tensor, "to", real_to)
        monkeypatch.setattr(torch.Tensor, "contiguous", real_contig)
    assert made, f"copy probe (not the library): {rid} made no device copy of '{name}'"
    after = [torch.empty(nb, dtype=torch.uint8, device="cuda") for _, nb in made]   # the wrapper's temporaries are dead by now
    again = {t.data_ptr() for t in after}
    torch.cuda.synchronize()
    del outs
    return {p for p, _ in made}, again


@pytest.mark.parametrize("rid", sorted(COPY_ROWS))
def test_allocator_does_not_recycle_a_wrapper_temporary(env, monkeypatch, rid):
    made, again = _copy_probe(env, env.R, rid, monkeypatch)
    assert made & again, f"copy probe (not the library): with a default renderer none of the temporaries of {rid} was handed out again: the probe is blind"
    made, again = _copy_probe(env, env.Rb, rid, monkeypatch)
    assert not (made & again), f"{rid}: a temporary the wrapper copied an argument into was handed out again while the private stream's kernel was still queued"


# ---------------------------------------------------------------------------------------------------------------- hand-over of context scratch and state
def _second(rid):
    """The row ``rid`` with other operands (the next synthetic frame / another seed)."""
    if rid == "render-frame":
        return SO.render_row(2)
    if rid == "finish-frame":
        return SO.finish_row(53)
    build = SO.CASES[rid]

    def other(R):
        c = build(R)
        c.late = {n: t.flip(-1).contiguous() for n, t in c.late.items()}
        return c
    return other


HANDOVER = ["render-frame", "finish-frame", "preview-heatmap", "letterbox-stats", "depth-preprocess-pil"]


@pytest.mark.parametrize("rid", HANDOVER)
def test_two_streams_share_one_context_in_call_order(env, rid):
    """A default renderer: call 1 on S1 behind the delay, call 2 on S2 at once with other operands -- the event ``vd3d_ctx_set_stream`` records is all that keeps
    S2's launches behind S1's on the context's scratch.  Both equal their ordinary-placement results."""
    h, R = env.h, env.R
    c1, c2 = env.case(rid), _second(rid)(R)
    r1, r2 = env.ref(rid), h.reference(R, c2)
    e1, e2 = h.upload(c1.early), h.upload({**c2.early, **c2.late})
    late = {n: SO.poisoned_like(t, h.device) for n, t in c1.late.items()}
    pinned = {n: t.pin_memory() for n, t in c1.late.items()}
    delay = h.delay_for(max(r1.a_ms, r2.a_ms))
    h.warm(R, c1, env.S2)   # the context is on S2 now: call 1 hands it to S1, call 2 back to S2
    with torch.cuda.stream(env.S1):
        h.sleep(delay)
        for n, t in late.items():
            t.copy_(pinned[n], non_blocking=True)
        o1 = c1.call(R, {**e1, **late})
    with torch.cuda.stream(env.S2):
        o2 = c2.call(R, e2)
        k2 = [o.clone() for o in o2]
    with torch.cuda.stream(env.S1):
        k1 = [o.clone() for o in o1]
    torch.cuda.synchronize()
    bad1 = [i for i, (a, b) in enumerate(zip(k1, r1.outs)) if not SO.same_bits(a, b)]
    bad2 = [i for i, (a, b) in enumerate(zip(k2, r2.outs)) if not SO.same_bits(a, b)]
    print(f"STREAM hand-over {rid}: delay {delay:.2f} ms, first call mismatch {bad1}, second call mismatch {bad2}")
    assert not bad1 and not bad2, f"{rid}: S1's call differs in outputs {bad1}, S2's in {bad2}, with S2's call enqueued while S1's waited {delay:.1f} ms for its operands"


def test_tracker_state_crosses_streams_in_call_order(env):
    """The letterbox tracker's state lives in the context: a reset and the frames A on S1 behind the delay, then at once on S2 the statistics of the frames B
    chained to the tracker's previous frame (``mad_sum[0]`` = |B[0] - A[-1]|).  A call that is not held behind S1's compares with the frame an earlier call left."""
    h, R = env.h, env.R
    A_ = env.case("letterbox-track").late["frames"]
    B_ = A_.flip(-1).contiguous()
    dA, dB = A_.cuda(), B_.cuda()
    stats = lambda: tuple(t.clone() for t in R.letterbox_stats(dB, chain=True).values())   # noqa: E731
    torch.cuda.synchronize()
    R.letterbox_state_reset()
    want0 = R.letterbox_track(dA, 36).clone()
    want1 = stats()
    R.letterbox_track(dB, 36)   # leaves B[-1] as the previous frame: what a call that runs too early is chained to
    stale = stats()
    torch.cuda.synchronize()
    assert not all(SO.same_bits(a, b) for a, b in zip(stale, want1)), "stream_order harness (not the library): the chained statistics do not depend on the tracker's frame"
    late, pinned = SO.poisoned_like(A_, h.device), A_.pin_memory()
    h.warm(R, env.case("letterbox-stats"), env.S2)
    with torch.cuda.stream(env.S1):
        h.sleep(SO.MIN_DELAY_MS)
        late.copy_(pinned, non_blocking=True)
        R.letterbox_state_reset()
        g0 = R.letterbox_track(late, 36)
    with torch.cuda.stream(env.S2):
        got1 = stats()
    with torch.cuda.stream(env.S1):
        got0 = g0.clone()
    torch.cuda.synchronize()
    assert SO.same_bits(got0, want0), (got0.tolist(), want0.tolist())
    bad = [i for i, (a, b) in enumerate(zip(got1, want1)) if not SO.same_bits(a, b)]
    assert not bad, f"S2's chained statistics differ in outputs {bad} (dict order of letterbox_stats): they were not held behind S1's tracker update"


def test_render_state_crosses_streams_in_call_order(env):
    """The temporal state of the render loop lives in the context: a new clip and frame 1 on S1 behind the delay, frame 2 on S2 at once, without a reset.  Frame 2
    is rendered on what frame 1 left, as in the serial loop."""
    h, R = env.h, env.R
    p = SO.render_params()
    (f1, d1), (f2, d2) = SO.synth_pair(1), SO.synth_pair(2)
    T = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    F1, D1, F2, D2 = T(f1), T(d1), T(f2), T(d2)
    torch.cuda.synchronize()
    R.reset_state(); R.new_clip()
    want = [R.render_frame(F1, D1, p).clone(), R.render_frame(F2, D2, p).clone()]
    torch.cuda.synchronize()
    late, pinned = SO.poisoned_like(torch.from_numpy(f1), h.device), torch.from_numpy(f1).pin_memory()
    delay = h.delay_for(env.ref("render-frame").a_ms)   # before the clip starts: the row's reference renders a frame of its own
    R.reset_state(); R.new_clip()
    torch.cuda.synchronize()
    with torch.cuda.stream(env.S1):
        h.sleep(delay)
        late.copy_(pinned, non_blocking=True)
        g1 = R.render_frame(late, D1, p)
    with torch.cuda.stream(env.S2):
        g2 = R.render_frame(F2, D2, p)
        k2 = g2.clone()
    with torch.cuda.stream(env.S1):
        k1 = g1.clone()
    torch.cuda.synchronize()
    assert SO.same_bits(k1, want[0]) and SO.same_bits(k2, want[1]), (SO.same_bits(k1, want[0]), SO.same_bits(k2, want[1]))


# ---------------------------------------------------------------------------------------------------------------- two contexts at once
PAIR_A, PAIR_B = ["gemm-bf16x3-257x48x255-b1", "attn-4-T65"], ["conv3x3-dense", "conv-x3"]


@pytest.mark.parametrize("same_rows", [False, True], ids=["own-rows", "same-rows"])
def test_two_contexts_on_two_streams(env, same_rows):
    """Two default renderers on two side streams: four interleaved rounds of two rows each with no synchronisation between them.  ``same-rows``: both renderers run
    all four rows, so both pass through the library's per-device static state (LDS opt-in records, row-table cache, per-geometry tables)."""
    from visiondepth3d_amd.render_3d import Renderer
    Ra, Rb = Renderer(0), Renderer(0)
    try:
        rows_a, rows_b = (PAIR_A + PAIR_B, PAIR_B + PAIR_A) if same_rows else (PAIR_A, PAIR_B)
        ops = {rid: env.h.upload({**env.case(rid).early, **env.case(rid).late}) for rid in PAIR_A + PAIR_B}
        refs = {rid: env.ref(rid) for rid in PAIR_A + PAIR_B}
        torch.cuda.synchronize()
        got = []
        for rnd in range(4):
            for ra, rb in zip(rows_a, rows_b):
                with torch.cuda.stream(env.S1):
                    got.append((ra, rnd, "a", [o.clone() for o in env.case(ra).call(Ra, ops[ra])]))
                with torch.cuda.stream(env.S2):
                    got.append((rb, rnd, "b", [o.clone() for o in env.case(rb).call(Rb, ops[rb])]))
        torch.cuda.synchronize()
        bad = [(rid, rnd, who) for rid, rnd, who, outs in got if not all(SO.same_bits(a, b) for a, b in zip(outs, refs[rid].outs))]
        assert not bad, f"(row, round, renderer) that differ from the serial run: {bad}"
    finally:
        torch.cuda.synchronize()
        Ra.close()
        Rb.close()


def test_depth_pipe_refuses_a_private_stream_renderer_on_the_gpu(env):
    from visiondepth3d_amd.depth import DepthPipe
    with pytest.raises(ValueError, match="SAME stream as the network"):
        DepthPipe("depth-anything-v2-small", device="cuda", renderer=env.Rb)
