"""Launch-trace characterisation of DepthPipe's DPT neck / head rewrite (depth.py): per mode, the ORDERED list of Renderer methods one forward calls and the whole
conv_routes dict, against tests/golden/depth_route_trace.json.  The golden was recorded from the tree before the rewrite was taken apart into route objects, so the
test pins "the sequence of launches per forward stays what it was" for every mode the rewrite serves; the cases behind the comment in CASES were recorded from the
tree before the rewrites moved out of DepthPipe into depth_routes.py / depth_pro.py, and cover DPT in fp16x2, the self-contained DPT-Hybrid and metric head and DepthPro's
encoder / decoder routes (whose decoder_routes and encoders_resize are pinned too).  The trace holds method names only: no timings, no addresses,
nothing a ROCm release changes.  Each case builds its own pipe and runs two forwards: the first packs / composes what is cached per parameter version, the second
must not.

Recording (off by default, local to this file): VD3D_ROUTE_TRACE_RECORD=<path of a JSON file> makes every case write its entry there instead of comparing."""
import inspect
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_route_trace.json")
RECORD = os.environ.get("VD3D_ROUTE_TRACE_RECORD")
SWITCHES = ("VD3D_NECK_GLUE", "VD3D_HEAD_FUSED", "VD3D_HEAD_CONV2_GATHER", "VD3D_HEAD_UPCONV", "VD3D_NECK_POLY")
DA = "depth-anything-v2-small"
SMALL_DPT = "small-dpt-processor"   # the 128 x 128 image processor of tests/test_hip_self_contained_dpt.py
MINI_PRO = "mini-depth-pro"         # depth_pro_cases.mini_config() / mini_processor(): these cases also pin decoder_routes and encoders_resize

# id -> (model, seed, frame size, environment, DepthPipe keywords); "neck-alone" calls pipe.model.neck(hs, 5, 7) instead of a forward
CASES = {
    "da-f32": (DA, 0, (270, 480), {}, {}),
    **{f"da-f32-{s}=0": (DA, 0, (270, 480), {s: "0"}, {}) for s in SWITCHES},   # (set before construction: VD3D_NECK_GLUE is read there)
    "da-f32-VD3D_HEAD_CONV2_GATHER=1": (DA, 0, (270, 480), {"VD3D_HEAD_CONV2_GATHER": "1"}, {}),
    "da-f32-neck-alone": (DA, 0, (270, 480), {}, {}),
    "da-bf16": (DA, 0, (270, 480), {}, dict(dtype="bfloat16")),
    "da-bf16x3": (DA, 0, (270, 480), {}, dict(gemm="bf16x3")),
    "da-bf16x3-conv": (DA, 0, (270, 480), {}, dict(gemm="bf16x3", conv="bf16x3")),
    "da-fp16x2": (DA, 0, (270, 480), {}, dict(gemm="fp16x2")),
    "da-fp16x2-conv": (DA, 0, (270, 480), {}, dict(gemm="fp16x2", conv="fp16x2")),
    "da-self-contained-bf16x3": (DA, 0, (270, 480), {}, dict(gemm="bf16x3", conv="bf16x3", self_contained=True)),
    "da-self-contained-fp16x2": (DA, 0, (270, 480), {}, dict(gemm="fp16x2", conv="fp16x2", self_contained=True)),
    "dpt-large-bf16x3": ("dpt-large", 5, (252, 476), {}, dict(gemm="bf16x3", processor=SMALL_DPT)),
    "dpt-large-self-contained-bf16x3": ("dpt-large", 5, (252, 476), {}, dict(gemm="bf16x3", conv="bf16x3", self_contained=True, processor=SMALL_DPT)),
    "dpt-hybrid-bf16x3": ("dpt-hybrid-midas", 7, (252, 476), {}, dict(gemm="bf16x3")),
    # what the move of the rewrites into depth_routes.py / depth_pro.py touches and the matrix above does not reach
    "dpt-large-fp16x2": ("dpt-large", 5, (252, 476), {}, dict(gemm="fp16x2", processor=SMALL_DPT)),
    "dpt-large-self-contained-fp16x2": ("dpt-large", 5, (252, 476), {}, dict(gemm="fp16x2", conv="fp16x2", self_contained=True, processor=SMALL_DPT)),
    "dpt-hybrid-self-contained-bf16x3": ("dpt-hybrid-midas", 7, (252, 476), {}, dict(gemm="bf16x3", conv="bf16x3", self_contained=True)),
    "da-metric-self-contained-bf16x3": ("depth-anything-v2-metric-indoor-large", 0, (270, 480), {}, dict(gemm="bf16x3", conv="bf16x3", self_contained=True)),
    "depth-pro-mini": (MINI_PRO, 4, (135, 241), {}, {}),
    **{f"depth-pro-mini-encoders-{m}": (MINI_PRO, 4, (135, 241), {}, dict(encoders=m)) for m in ("bf16x3", "fp16x2")},
    **{f"depth-pro-mini-encoders-decoder-{m}": (MINI_PRO, 4, (135, 241), {}, dict(encoders=m, decoder=m)) for m in ("bf16x3", "fp16x2")},
}


@pytest.fixture(scope="module")
def R():
    from visiondepth3d_amd.render_3d import Renderer
    assert torch.cuda.is_available()
    r = Renderer(0)
    yield r
    r.close()


def _trace_renderer(R, monkeypatch):
    """Every public method of the Renderer INSTANCE appends its name to the returned list, then runs."""
    log = []
    for name, _ in inspect.getmembers(type(R), callable):
        if name.startswith("_") or not callable(getattr(R, name)):
            continue

        def traced(*a, _name=name, _real=getattr(R, name), **k):
            log.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(R, name, traced)
    return log


@pytest.mark.parametrize("case", list(CASES))
def test_forward_calls_the_recorded_renderer_methods_and_routes(R, monkeypatch, case):
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.depth import PROCESSORS, DepthPipe
    model, seed, (fh, fw), env, kw = CASES[case]
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s, v in env.items():
        monkeypatch.setenv(s, v)
    kw = dict(kw)
    if kw.get("processor") == SMALL_DPT:
        kw["processor"] = dict(PROCESSORS["dpt"], size=(128, 128))
    if model == MINI_PRO:
        import depth_pro_cases
        kw.update(model=depth_pro_cases.build(depth_pro_cases.mini_config(), seed), processor=depth_pro_cases.mini_processor())
    dtype = getattr(torch, kw.pop("dtype", "float32"))
    pipe = DepthPipe(model, device="cuda", dtype=dtype, seed=seed, renderer=R, **kw)
    log = _trace_renderer(R, monkeypatch)
    got = {}
    with torch.no_grad():
        for which in ("first", "second"):
            del log[:]
            if case.endswith("neck-alone"):   # no head behind the neck: the un-armed path
                g = torch.Generator(device="cuda").manual_seed(1)
                hs = [torch.randn(1, 1 + 5 * 7, pipe.model.neck.reassemble_stage.layers[0].projection.in_channels, device="cuda", generator=g) for _ in range(4)]
                pipe.model.neck(hs, 5, 7)
            else:
                frames = torch.from_numpy(np.stack([synth.synth_frame(i, fh, fw)[0] for i in range(2)])).cuda()
                pred = pipe.infer_bgr_u8(frames, raw=True)
                assert pred.shape[0] == 2 and bool(torch.isfinite(pred).all())
            got[which] = list(log)
    torch.cuda.synchronize()
    got["conv_routes"] = {k: list(v) for k, v in sorted(pipe.conv_routes.items())}
    if model == MINI_PRO:
        got["decoder_routes"], got["encoders_resize"] = dict(sorted(pipe.decoder_routes.items())), dict(sorted(pipe.encoders_resize.items()))
    if RECORD:
        data = {}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                data = json.load(f)
        data[case] = got
        with open(RECORD, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(data[k])}" for k in sorted(data)) + "\n}\n")
        return
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    assert got["conv_routes"] == want["conv_routes"]
    assert got["first"] == want["first"]
    assert got["second"] == want["second"]
    if model == MINI_PRO:
        assert got["decoder_routes"] == want["decoder_routes"]
        assert got["encoders_resize"] == want["encoders_resize"]
