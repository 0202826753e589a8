"""The measurements of profiles/r22_dpt_hybrid.md, on one MI355X: ``forward`` (16-frame forwards of the five configurations, alternating), ``kernels`` (the BiT
prefix per launch under self_contained=True, the library prefix beside it, each new kernel beside a device copy of the same bytes), ``cold`` (process start to the
end of the first forward, a fresh process per configuration; ``cold1 CFG`` is that child).  Writes hybrid_*.json into the directory VD3D_PROBE_OUT names (default: vd3d_probe under the temporary directory)."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

T0 = time.time()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("VD3D_PROBE_OUT") or os.path.join(tempfile.gettempdir(), "vd3d_probe")
os.makedirs(OUT, exist_ok=True)
NAME, SEED, B = "dpt-hybrid-midas", 7, 16
CFGS = {"f32": dict(), "bf16x3": dict(gemm="bf16x3", conv="bf16x3"), "fp16x2": dict(gemm="fp16x2", conv="fp16x2"),
        "bf16x3_sc": dict(gemm="bf16x3", conv="bf16x3", self_contained=True), "fp16x2_sc": dict(gemm="fp16x2", conv="fp16x2", self_contained=True)}


def setup(n):
    import numpy as np
    import torch
    from visiondepth3d_amd import synth
    from visiondepth3d_amd.render_3d import Renderer
    R = Renderer(0)
    frames = torch.from_numpy(np.stack([synth.synth_frame(i, 252, 476)[0] for i in range(n)])).cuda()
    return torch, R, frames


def pipe(R, cfg):
    import torch
    from visiondepth3d_amd.depth import DepthPipe
    return DepthPipe(NAME, device="cuda", dtype=torch.float32, seed=SEED, renderer=R, **CFGS[cfg])


def med(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), n=len(v))


def forward():
    torch, R, frames = setup(B)
    pipes = {c: pipe(R, c) for c in CFGS}
    x = R.depth_preprocess(frames, 384, 384, (0.5,) * 3, (0.5,) * 3)
    res = {c: [] for c in CFGS}
    with torch.no_grad():
        for c, p in pipes.items():
            for _ in range(3):
                p.model(pixel_values=x)
        torch.cuda.synchronize()
        for _ in range(7):   # alternating rounds
            for c, p in pipes.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(3):
                    p.model(pixel_values=x)
                torch.cuda.synchronize()
                res[c].append((time.perf_counter() - t) / 3 * 1e3)
    out = {c: med(v) for c, v in res.items()}
    print(json.dumps(out, indent=1))
    json.dump(out, open(os.path.join(OUT, "hybrid_forward.json"), "w"), indent=1)


def kernels():
    torch, R, frames = setup(B)
    p = pipe(R, "bf16x3_sc")
    plib = pipe(R, "bf16x3")
    x = R.depth_preprocess(frames, 384, 384, (0.5,) * 3, (0.5,) * 3)
    emb = p.model.dpt.embeddings
    bb_lib = plib.model.dpt.embeddings.backbone
    log, on = {}, [False]

    def wrap(name, key_fn):
        orig = getattr(R, name)

        def timed(*a, **kw):
            if not on[0]:
                return orig(*a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = orig(*a, **kw)
            e1.record()
            log.setdefault((name,) + key_fn(*a, **kw), []).append((e0, e1, y.numel() * 4))
            return y
        setattr(R, name, timed)
    wrap("im2col", lambda x, k, s, pad, out=None: (tuple(x.shape), k, s))
    wrap("groupnorm", lambda x, g, w, b, eps, residual=None, relu=False, out=None: (tuple(x.shape), "res" if residual is not None else "", "relu" if relu else ""))
    wrap("maxpool3x3_s2", lambda x, pad, pv=0.0: (tuple(x.shape),))
    wrap("linear_x3", lambda x, img, N, bias=None, gelu=False, mode="bf16x3": (tuple(x.shape), N))
    wrap("conv3x3_x3", lambda x, img, Cout: (tuple(x.shape), Cout))
    import visiondepth3d_amd.depth as D
    prefix = D._BitPrefix(p, emb.backbone, D.bit_prefix_plan(emb.backbone, {id(m): n for n, m in p.model.named_modules()}), {id(m): n for n, m in p.model.named_modules()})
    with torch.no_grad():
        for _ in range(3):
            prefix(x)
            bb_lib(x)
        torch.cuda.synchronize()
        tot, lib = [], []
        for _ in range(7):
            torch.cuda.synchronize(); t = time.perf_counter(); prefix(x); torch.cuda.synchronize(); tot.append((time.perf_counter() - t) * 1e3)
            torch.cuda.synchronize(); t = time.perf_counter(); bb_lib(x); torch.cuda.synchronize(); lib.append((time.perf_counter() - t) * 1e3)
        on[0] = True
        for _ in range(5):
            prefix(x)
        torch.cuda.synchronize()
        on[0] = False
    rows = []
    for key, evs in log.items():
        ms = [a.elapsed_time(b) for a, b, _ in evs]
        calls = len(evs) // 5
        rows.append(dict(op=key[0], shape=str(key[1:]), calls_per_forward=calls, median_ms_per_call=statistics.median(ms), ms_per_forward=statistics.median(ms) * calls,
                         out_bytes=evs[0][2]))
    # new kernels beside a device copy that moves the same bytes (in + out of the algorithm)
    def timeit(fn, n=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(5):
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / n)
        return statistics.median(ts)
    cmp_rows = []

    def beside(what, fn, nbytes):
        a = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda")
        b = torch.empty_like(a)
        t_k, t_c = timeit(fn), timeit(lambda: b.copy_(a))
        cmp_rows.append(dict(kernel=what, algorithm_bytes=nbytes, kernel_ms=t_k, kernel_GBps=nbytes / t_k / 1e6, copy_ms=t_c, copy_GBps=nbytes / t_c / 1e6, kernel_over_copy=t_k / t_c))
    g = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*s):
        return torch.randn(*s, device="cuda", generator=g)
    xs = x.permute(0, 2, 3, 1).contiguous()
    beside("im2col 7x7 s2 16x384x384x3 -> 160", lambda: R.im2col(xs, 7, 2, (2, 3, 2, 3)), xs.numel() * 4 + B * 192 * 192 * 160 * 4)
    for (h, c) in ((96, 128), (48, 256)):
        t = rnd(B, h, h, c)
        beside(f"im2col 3x3 s2 16x{h}x{h}x{c}", lambda t=t: R.im2col(t, 3, 2, (0, 1, 0, 1)), t.numel() * 4 + B * (h // 2) ** 2 * 9 * c * 4)
    for (h, c) in ((96, 256), (48, 512)):
        t = rnd(B, h, h, c)
        beside(f"im2col 1x1 s2 16x{h}x{h}x{c}", lambda t=t: R.im2col(t, 1, 2, (0, 0, 0, 0)), t.numel() * 4 + B * (h // 2) ** 2 * c * 4)
    t = rnd(B, 192, 192, 64)
    beside("maxpool 16x192x192x64", lambda: R.maxpool3x3_s2(t, (0, 1, 0, 1)), t.numel() * 4 + t.numel())
    for (h, c) in ((192, 64), (96, 64), (96, 256), (48, 128), (48, 512), (24, 256), (24, 1024)):
        t, w, bb = rnd(B, h, h, c), rnd(c), rnd(c)
        beside(f"groupnorm+relu 16x{h}x{h}x{c}", lambda t=t, w=w, bb=bb: R.groupnorm(t, 32, w, bb, 1e-5, relu=True), t.numel() * 8)
        if c >= 256:
            r = rnd(B, h, h, c)
            beside(f"groupnorm+res+relu 16x{h}x{h}x{c}", lambda t=t, w=w, bb=bb, r=r: R.groupnorm(t, 32, w, bb, 1e-5, residual=r, relu=True), t.numel() * 12)
    out = dict(prefix_self_contained=med(tot), prefix_library=med(lib), per_op=sorted(rows, key=lambda r: -r["ms_per_forward"]), beside_copy=cmp_rows)
    json.dump(out, open(os.path.join(OUT, "hybrid_kernels.json"), "w"), indent=1)
    print(json.dumps(dict(prefix_self_contained=out["prefix_self_contained"], prefix_library=out["prefix_library"]), indent=1))
    by = {}
    for r in rows:
        by[r["op"]] = by.get(r["op"], 0.0) + r["ms_per_forward"]
    print(json.dumps(by, indent=1))
    for r in cmp_rows:
        print(r["kernel"], round(r["kernel_ms"], 4), "ms", round(r["kernel_GBps"]), "GB/s; copy", round(r["copy_ms"], 4), "ms", round(r["copy_GBps"]), "GB/s")


def cold1(cfg):
    torch, R, frames = setup(B)
    p = pipe(R, cfg)
    p.infer_bgr_u8(frames, raw=True)
    torch.cuda.synchronize()
    print("COLD1", cfg, time.time() - T0)


def cold():
    out = {}
    for cfg in CFGS:
        ts = []
        for _ in range(2):
            t = time.time()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "cold1", cfg], timeout=240, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:])
                sys.exit(r.returncode if r.returncode > 0 else 1)
            ts.append(time.time() - t)
        out[cfg] = dict(seconds=ts)
        print(cfg, ts)
    json.dump(out, open(os.path.join(OUT, "hybrid_cold.json"), "w"), indent=1)


if __name__ == "__main__":
    {"forward": forward, "kernels": kernels, "cold": cold}.get(sys.argv[1], lambda: cold1(sys.argv[2]))()
