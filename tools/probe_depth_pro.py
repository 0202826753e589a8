"""Measurements behind profiles/r25_depth_pro.md: DepthPro's two kernels alone (time, bytes moved, fraction of the stream-copy yardstick measured in the same
process) and the 1536 x 1536 forward of DepthPipe("depth-pro") at one frame and four, beside the stock path (processor and post-process as ATen operators around the
same module) in the same process, runs alternating.  Medians of ROUNDS rounds, the spread as min .. max.  Prints one JSON line per measurement.

    python tools/probe_depth_pro.py kernels
    python tools/probe_depth_pro.py forward [--frames 1 4]

and behind profiles/r28_depth_pro_encoders.md (DepthPipe(encoders=...)): the pyramid and merge kernels alone at the published shapes beside the stream copy of the
same bytes and the ATen operations they replace; the 1536 x 1536 forward with encoders=None / "bf16x3" / "fp16x2" (one synthetic model, copied per pipe), its three
own parts timed apart, and the two hand-over layouts of the merge in front of the library neck; the time from process start to the end of the first forward.

    python tools/probe_depth_pro.py pyramid [--frames 1 4]
    python tools/probe_depth_pro.py encoders [--frames 1 4]
    python tools/probe_depth_pro.py first --mode bf16x3

and behind profiles/r29_depth_pro_decoder.md (DepthPipe(encoders=..., decoder=...)): vd3d_conv3x3_epi beside the pair of launches it replaces, per argument set
the decoder uses, at 256 -> 256 channels; vd3d_depthpro_head beside the four launches it replaces, with the peak device memory of both forms; the 1536 x 1536
forward with encoders=m alone and with decoder=m on top, the decoder apart on the pipe's own features; the cold start with the keyword.

    python tools/probe_depth_pro.py epi [--frames 1 4]
    python tools/probe_depth_pro.py head [--frames 1 4]
    python tools/probe_depth_pro.py decoder [--frames 1 4]
    python tools/probe_depth_pro.py first --mode bf16x3 --decoder
"""
import argparse
import json
import os
import statistics
import sys
import time

T0 = time.time()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ROUNDS = 7


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def rounds(fns, iters, warm=3):
    """Alternating rounds over the callables -> {name: (median ms, min, max)}."""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            got[k].append(timed(f, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def kernels():
    from visiondepth3d_amd import _lib
    from visiondepth3d_amd.render_3d import Renderer, _ptr
    R = Renderer(0)
    n = 256 << 20
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    copy = rounds({"copy": lambda: _lib.check(R._L.vd3d_stream_copy(R._ctx, _ptr(src), _ptr(dst), n))}, 20)["copy"]
    bw = 2 * n / (copy[0] * 1e-3)
    print(json.dumps(dict(what="stream_copy_256MiB", ms=copy, bytes_per_s=bw)))
    fr = torch.randint(0, 256, (1, 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    fr8 = torch.randint(0, 256, (8, 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    fr_small = torch.randint(0, 256, (1, 540, 960, 3), dtype=torch.uint8, device="cuda")
    fr_4k = torch.randint(0, 256, (1, 2160, 3840, 3), dtype=torch.uint8, device="cuda")
    pred, fov = torch.rand(1, 1536, 1536, device="cuda") * 10 + 0.5, torch.tensor([55.0], device="cuda")
    half = (0.5, 0.5, 0.5)
    cases = {
        "preprocess_1080p_to_1536": (lambda: R.depthpro_preprocess(fr, 1536, half, half), fr.numel() + 3 * 1536 * 1536 * 4),
        "preprocess_540p_to_1536": (lambda: R.depthpro_preprocess(fr_small, 1536, half, half), fr_small.numel() + 3 * 1536 * 1536 * 4),
        "preprocess_4k_to_1536": (lambda: R.depthpro_preprocess(fr_4k, 1536, half, half), fr_4k.numel() + 3 * 1536 * 1536 * 4),
        "preprocess_8x1080p_to_1536": (lambda: R.depthpro_preprocess(fr8, 1536, half, half), fr8.numel() + 8 * 3 * 1536 * 1536 * 4),   # (past the launch floor)
        "post_1536_to_1080p_fov": (lambda: R.depthpro_post(pred, fov, 1080, 1920), pred.numel() * 4 + 1080 * 1920 * 4),
        "post_1536_raw_fov": (lambda: R.depthpro_post(pred, fov, 1536, 1536), pred.numel() * 8),
    }
    for name, (fn, nbytes) in cases.items():
        ms = rounds({name: fn}, 50)[name]
        print(json.dumps(dict(what=name, ms=ms, bytes=nbytes, bytes_per_s=nbytes / (ms[0] * 1e-3), of_stream_copy=nbytes / (ms[0] * 1e-3) / bw)))
    R.close()


def forward(frames):
    from visiondepth3d_amd import depth_pro
    from visiondepth3d_amd.depth import DepthPipe
    from visiondepth3d_amd.render_3d import Renderer
    R = Renderer(0)
    t = time.time()
    pipe = DepthPipe("depth-pro", renderer=R)
    built = time.time()
    fr = torch.randint(0, 256, (max(frames), 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    pipe.infer_bgr_u8(fr[:1])
    torch.cuda.synchronize()
    print(json.dumps(dict(what="start_to_first_forward", import_s=t - T0, construct_s=built - t, first_forward_s=time.time() - built, total_s=time.time() - T0,
                          params=pipe.n_params)))
    half = (0.5, 0.5, 0.5)

    @torch.no_grad()
    def stock(f):
        out = pipe.model(pixel_values=depth_pro.preprocess_statement(f, (1536, 1536), half, half))
        return depth_pro.post_statement(out.predicted_depth, out.field_of_view, f.shape[1], f.shape[2])

    @torch.no_grad()
    def net(x):
        return pipe.model(pixel_values=x).predicted_depth
    for B in frames:
        f = fr[:B]
        x = R.depthpro_preprocess(f, 1536, half, half)
        r = rounds({"pipe": lambda: pipe.infer_bgr_u8(f), "stock": lambda: stock(f), "network_alone": lambda: net(x)}, 2, warm=1)
        print(json.dumps(dict(what=f"forward_1536_f32_B{B}", ms=r)))
    R.close()


def pyramid(frames):
    """The two encoder-side kernels alone at the published shapes (S = 1536, p = 384, a 24 x 24 grid of 1024 channels)."""
    import torch.nn.functional as F
    from transformers.models.depth_pro.modeling_depth_pro import reconstruct_feature_maps, split_to_patches
    from visiondepth3d_amd import _lib
    from visiondepth3d_amd.render_3d import Renderer, _ptr
    R = Renderer(0)
    n = 512 << 20
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")

    def copy_of(nbytes):   # the stream copy of nbytes / 2 in, nbytes / 2 out
        return lambda: _lib.check(R._L.vd3d_stream_copy(R._ctx, _ptr(src), _ptr(dst), nbytes // 2))

    def aten_patches(x):
        imgs = [split_to_patches(F.interpolate(x, scale_factor=r, mode="bilinear", align_corners=False), 384, o) for r, o in ((0.25, 0.0), (0.5, 0.5), (1, 0.25))]
        return torch.cat(imgs[::-1], dim=0)
    for B in frames:
        x = torch.randn(B, 3, 1536, 1536, device="cuda")
        nbytes = x.numel() * 4 + 35 * B * 3 * 384 * 384 * 4
        r = rounds({"kernel": lambda: R.depthpro_patches(x, 384, [288, 192, 384]), "stream_copy": copy_of(nbytes), "aten": lambda: aten_patches(x)}, 20)
        print(json.dumps(dict(what=f"patches_1536_p384_B{B}", ms=r, bytes=nbytes, bytes_per_s=nbytes / (r["kernel"][0] * 1e-3), of_stream_copy=r["stream_copy"][0] / r["kernel"][0])))
        for name, nseq, pad, out in (("level_full", 25, 3, 96), ("level_half", 9, 6, 48), ("level_quarter", 1, 12, 24), ("hook", 35, 3, 96)):
            rows = torch.randn(nseq * B, 577, 1024, device="cuda")
            nbytes = 2 * B * out * out * 1024 * 4
            r = rounds({"kernel": lambda: R.depthpro_merge(rows, B, 24, pad, out, out), "stream_copy": copy_of(nbytes),
                        "aten": lambda: reconstruct_feature_maps(rows, B, pad, (out, out))}, 20)
            print(json.dumps(dict(what=f"merge_{name}_B{B}", ms=r, bytes=nbytes, bytes_per_s=nbytes / (r["kernel"][0] * 1e-3), of_stream_copy=r["stream_copy"][0] / r["kernel"][0])))
    R.close()


def _full_model():
    from transformers import DepthProForDepthEstimation
    from visiondepth3d_amd import depth_pro
    from visiondepth3d_amd.depth import synthetic_weights_
    m = DepthProForDepthEstimation(depth_pro.config()).eval()
    synthetic_weights_(m, 0)
    return m


def encoders(frames):
    import copy
    from visiondepth3d_amd.depth import DepthPipe, patch_embedding_rows
    from visiondepth3d_amd.render_3d import Renderer
    from visiondepth3d_amd.vit_blocks import dinov2_operands, encoder_blocks
    R = Renderer(0)
    model = _full_model()
    pipes = {str(mode): DepthPipe("depth-pro", renderer=R, model=copy.deepcopy(model), encoders=mode) for mode in (None, "bf16x3", "fp16x2")}
    del model
    fr = torch.randint(0, 256, (max(frames), 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    half = (0.5, 0.5, 0.5)
    for B in frames:
        f = fr[:B]
        r = rounds({k: (lambda p=p: p.infer_bgr_u8(f)) for k, p in pipes.items()}, 2, warm=1)
        print(json.dumps(dict(what=f"forward_1536_encoders_B{B}", ms=r, resize={k: p.encoders_resize for k, p in pipes.items()})))
    # the three own parts apart (random activations of the published shapes; the blocks on freshly packed copies of the same weights)
    for mode in ("bf16x3", "fp16x2"):
        pipe = pipes[mode]
        net = pipe.model
        vits = [net.depth_pro.encoder.patch_encoder.model, net.depth_pro.encoder.image_encoder.model, net.fov_model.fov_encoder.model]
        embeds = [patch_embedding_rows(R, v.embeddings.patch_embeddings.projection, mode) for v in vits]
        blocks = [encoder_blocks(R, [dinov2_operands(lay) for lay in v.encoder.layer], mode, keyword="encoders") for v in vits]
        for B in frames:
            x = R.depthpro_preprocess(fr[:B], 1536, half, half)

            @torch.no_grad()
            def embed():
                patches = R.depthpro_patches(x, 384, [288, 192, 384])
                for v, rows, inp in zip(vits, embeds, (patches, patches[-B:], patches[-B:])):
                    tok = rows(inp)
                    torch.cat((v.embeddings.cls_token.expand(tok.shape[0], -1, -1), tok), dim=1) + v.embeddings.position_embeddings
            seqs = [torch.randn(n, 577, 1024, device="cuda") * 0.5 for n in (35 * B, B, B)]

            @torch.no_grad()
            def run_blocks():
                for v, bl, t in zip(vits, blocks, seqs):
                    for b in bl:
                        t = b(t)
                    R.add_layernorm(t, None, v.layernorm)

            def merges():
                t = seqs[0]
                R.depthpro_merge(t[:25 * B], B, 24, 3, 96, 96), R.depthpro_merge(t[25 * B:34 * B], B, 24, 6, 48, 48), R.depthpro_merge(t[34 * B:], B, 24, 12, 24, 24)
                R.depthpro_merge(t, B, 24, 3, 96, 96), R.depthpro_merge(t, B, 24, 3, 96, 96), R.depthpro_merge(seqs[1], B, 24, 0, 24, 24)
            r = rounds({"pyramid_and_embeddings": embed, "encoder_blocks": run_blocks, "merges": merges}, 2, warm=1)
            print(json.dumps(dict(what=f"parts_{mode}_B{B}", ms=r)))
        del blocks, embeds
    # the two hand-over layouts of the merge in front of the library neck, fusion stage and head: the [B, C, oh, ow] view of the NHWC storage, or a contiguous copy
    pipe = pipes["bf16x3"]
    for B in frames:
        got = {}
        h = pipe.model.depth_pro.neck.register_forward_pre_hook(lambda mod, args: got.__setitem__("f", [t.clone(memory_format=torch.preserve_format) for t in args[0]]))
        pipe.infer_bgr_u8(fr[:B])
        h.remove()
        feats = got["f"]
        assert all(t.is_contiguous(memory_format=torch.channels_last) for t in feats)

        @torch.no_grad()
        def decoder(fs):
            return pipe.model.head(pipe.model.fusion_stage(pipe.model.depth_pro.neck(fs))[-1])
        r = rounds({"view": lambda: decoder(list(feats)), "contiguous_copy": lambda: decoder([t.contiguous() for t in feats])}, 2, warm=1)
        print(json.dumps(dict(what=f"handover_layout_B{B}", ms=r)))
    R.close()


def epi(frames):
    """vd3d_conv3x3_epi against bias-free convolution + vd3d_nhwc_bias_act_f32 on the same buffers: 256 -> 256 channels on the fusion stage's maps."""
    from visiondepth3d_amd.render_3d import Renderer
    CL = torch.channels_last
    R = Renderer(0)
    w = torch.randn(256, 256, 3, 3, device="cuda") * 0.02
    bias = torch.randn(256, device="cuda")
    sets = {"relu_in+bias+relu": dict(relu_in=True, relu=True), "bias+r1": dict(r1=True), "bias+r1+r2": dict(r1=True, r2=True), "bias": dict()}
    for mode in ("bf16x3", "fp16x2"):
        img = R.conv3x3_tile_pack(w, mode, 1)
        for side in (96, 384, 768):
            for B in frames:
                x, r1, r2 = (torch.randn(B, 256, side, side, device="cuda").contiguous(memory_format=CL) for _ in range(3))
                for name, s in sets.items():
                    kw = dict(bias=bias, r1=r1 if s.get("r1") else None, r2=r2 if s.get("r2") else None, relu=bool(s.get("relu")))

                    def fused():
                        return R.conv3x3_epi(x, img, 256, mode, relu_in=bool(s.get("relu_in")), **kw)

                    def pair():
                        return R.bias_act(R.conv3x3_tile(torch.relu(x) if s.get("relu_in") else x, img, 256, mode, 1), **kw)

                    def bare():
                        return R.conv3x3_tile(x, img, 256, mode, 1)
                    assert torch.equal(fused(), pair())
                    r = rounds({"fused": fused, "pair": pair, "bare_convolution": bare}, 3 if side == 768 else 10, warm=1)
                    print(json.dumps(dict(what=f"epi_{mode}_{side}_B{B}_{name}", ms=r, fused_over_pair=r["fused"][0] / r["pair"][0])))
                del x, r1, r2
    R.close()


def head(frames):
    """vd3d_depthpro_head against the four launches it replaces (GEMM, depth-to-space, bias-free tile convolution, vd3d_dpt_head_tail_f32): 768 x 768 -> 1536 x 1536,
    128 channels, with the peak device memory of both forms above the operands."""
    from visiondepth3d_amd import depth_pro
    from visiondepth3d_amd.depth import conv_transpose_gemm_weight, neck_poly_compose
    from visiondepth3d_amd.render_3d import Renderer
    R = Renderer(0)
    C = 128
    wt, bt = torch.randn(C, C, 2, 2, device="cuda") / C ** 0.5, torch.randn(C, device="cuda")
    w3, b2 = torch.randn(32, C, 3, 3, device="cuda") / (3.0 * C ** 0.5), torch.randn(32, device="cuda")
    w1, b3 = torch.randn(32, device="cuda") / 32 ** 0.5, 0.25
    T = depth_pro.head_poly_table(bt, w3, b2)
    for mode in ("bf16x3", "fp16x2"):
        poly = R.depthpro_head_pack(neck_poly_compose(wt, None, w3, 2)[0], mode)
        gimg, cimg = R.gemm_x3_pack(conv_transpose_gemm_weight(wt), mode), R.conv3x3_tile_pack(w3, mode, 1)
        for B in frames:
            x = torch.randn(B, C, 768, 768, device="cuda").contiguous(memory_format=torch.channels_last)

            def fused():
                return R.depthpro_head(x, poly, T, w1, b3, mode)

            def four():
                y = R.linear_x3(x.permute(0, 2, 3, 1), gimg, 4 * C, None, mode=mode)
                fine = R.depth_to_space_bias(y.view(-1, 4 * C), B, 768, 768, 2, bt)
                return R.dpt_head_tail(R.conv3x3_tile(fine, cimg, 32, mode, 1), b2, w1, b3, 1.0)
            peak = {}
            for k, f in (("fused", fused), ("four_launches", four)):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                out = f()
                torch.cuda.synchronize()
                peak[k] = torch.cuda.max_memory_allocated() - base
                del out
            d = (fused() - four()).abs().max().item()
            r = rounds({"fused": fused, "four_launches": four}, 3, warm=1)
            print(json.dumps(dict(what=f"head_{mode}_768_C{C}_B{B}", ms=r, fused_over_four=r["fused"][0] / r["four_launches"][0], peak_bytes=peak, max_abs_difference=d)))
            del x
    R.close()


def decoder(frames):
    """The 1536 x 1536 forward with encoders=m alone (the parent's pipe) and with decoder=m on top, one synthetic model copied per pipe; and the decoder apart
    -- neck, fusion stage and head on the features the pipe's own encoders hand over -- in the stock and the routed form."""
    import copy
    from visiondepth3d_amd.depth import DepthPipe
    from visiondepth3d_amd.render_3d import Renderer
    R = Renderer(0)
    model = _full_model()
    pipes = {}
    for mode in ("bf16x3", "fp16x2"):
        pipes[f"encoders={mode}"] = DepthPipe("depth-pro", renderer=R, model=copy.deepcopy(model), encoders=mode)
        pipes[f"encoders={mode},decoder={mode}"] = DepthPipe("depth-pro", renderer=R, model=copy.deepcopy(model), encoders=mode, decoder=mode)
    del model
    fr = torch.randint(0, 256, (max(frames), 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    for B in frames:
        f = fr[:B]
        r = rounds({k: (lambda p=p: p.infer_bgr_u8(f)) for k, p in pipes.items()}, 2, warm=1)
        print(json.dumps(dict(what=f"forward_1536_decoder_B{B}", ms=r)))
    routed = pipes["encoders=bf16x3,decoder=bf16x3"]
    print(json.dumps(dict(what="decoder_routes_full_size", routes=routed.decoder_routes)))
    for B in frames:
        got = {}
        src = pipes["encoders=bf16x3"]
        h = src.model.depth_pro.neck.register_forward_pre_hook(lambda mod, args: got.__setitem__("f", [t.clone(memory_format=torch.preserve_format) for t in args[0]]))
        src.infer_bgr_u8(fr[:B])
        h.remove()
        feats = got["f"]

        def apart(p):
            @torch.no_grad()
            def run():
                return p.model.head(p.model.fusion_stage(p.model.depth_pro.neck(list(feats)))[-1])
            return run
        r = rounds({k: apart(p) for k, p in pipes.items()}, 2, warm=1)
        print(json.dumps(dict(what=f"decoder_apart_B{B}", ms=r)))
    R.close()


def first(mode, with_decoder=False):
    from visiondepth3d_amd.depth import DepthPipe
    from visiondepth3d_amd.render_3d import Renderer
    R = Renderer(0)
    t = time.time()
    pipe = DepthPipe("depth-pro", renderer=R, encoders=None if mode == "none" else mode, decoder=mode if with_decoder else None)
    built = time.time()
    fr = torch.randint(0, 256, (1, 1080, 1920, 3), dtype=torch.uint8, device="cuda")
    pipe.infer_bgr_u8(fr)
    torch.cuda.synchronize()
    print(json.dumps(dict(what="start_to_first_forward", encoders=pipe.encoders, decoder=pipe.decoder, import_s=t - T0, construct_s=built - t, first_forward_s=time.time() - built,
                          total_s=time.time() - T0)))
    R.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "forward", "pyramid", "encoders", "first", "epi", "head", "decoder"])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--mode", choices=["none", "bf16x3", "fp16x2"], default="none")
    ap.add_argument("--decoder", action="store_true")
    a = ap.parse_args()
    {"kernels": kernels, "forward": lambda: forward(a.frames), "pyramid": lambda: pyramid(a.frames), "encoders": lambda: encoders(a.frames),
     "first": lambda: first(a.mode, a.decoder), "epi": lambda: epi(a.frames), "head": lambda: head(a.frames), "decoder": lambda: decoder(a.frames)}[a.what]()
