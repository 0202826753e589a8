"""DepthPipe(decoder=...) without a GPU: every refusal of the keyword, by message, raised at construction before the module is moved to a device
(``renderer=object()``, ``device="cuda"``: any use of the renderer, and any move to the absent GPU, would raise something else than the refusal); ``decoder=None``
builds exactly the pipe there was before the keyword; and the two compositions the routes rest on -- a fusion layer's ``deconv`` + ``projection`` as one
transposed convolution, and ``depth_pro.head_poly_statement`` with its border-class table -- against the float64 module chains, exactly, on integer operands."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
F = torch.nn.functional

import depth_pro_cases as cases   # noqa: E402
from visiondepth3d_amd import depth_pro   # noqa: E402
from visiondepth3d_amd.depth import DepthPipe   # noqa: E402

ON = dict(device="cuda", renderer=object(), tuned_gemm=False)
MODES = ["bf16x3", "fp16x2"]


def _mini(**over):
    return cases.build(cases.mini_config(**over))


def _refused(exc, match, model, processor=None, **kw):
    with pytest.raises(exc, match=match):
        DepthPipe("mini", model=model, processor=cases.mini_processor() if processor is None else processor, **dict(ON, **kw))
    if model is not None:
        assert {p.device.type for p in model.parameters()} == {"cpu"}   # refused before the module was moved to a device


@pytest.mark.parametrize("mode", MODES)
def test_arguments_are_refused_by_name(mode):
    m = _mini()
    _refused(ValueError, rf"decoder='{mode}' needs encoders='bf16x3' \| 'fp16x2'", m, decoder=mode)
    _refused(ValueError, r"decoder must be None, 'bf16x3' or 'fp16x2'", m, encoders=mode, decoder="f32")
    # gemm= / conv= / self_contained=True keep refusing DepthPro with their present messages
    _refused(NotImplementedError, rf"gemm='{mode}': 'mini' \(DepthProForDepthEstimation\).*not built", m, encoders=mode, decoder=mode, gemm=mode)
    _refused(NotImplementedError, r"self_contained=True: 'mini' \(DepthProForDepthEstimation\).*not built", m, encoders=mode, decoder=mode, gemm=mode, conv=mode,
             self_contained=True)
    _refused(ValueError, r"self_contained=True needs ", m, encoders=mode, decoder=mode, self_contained=True)


def test_another_model_is_refused_by_name():
    from transformers import DepthAnythingForDepthEstimation
    from visiondepth3d_amd.depth import build_config
    da = DepthAnythingForDepthEstimation(build_config("depth-anything-v2-small")).eval()
    with pytest.raises(NotImplementedError, match=r"decoder='bf16x3': 'da' \(DepthAnythingForDepthEstimation\) -- the keyword routes the neck, the fusion stage, the head "
                                                  r"and the field-of-view convolutions of DepthProForDepthEstimation"):
        depth_pro.decoder_scope(da, "da", "bf16x3", 518)
    # through the constructor the encoders' refusal, which the decoder needs first, names the model
    with pytest.raises(NotImplementedError, match=r"encoders='bf16x3': 'depth-anything-v2-small' \(DepthAnythingForDepthEstimation\)"):
        DepthPipe("depth-anything-v2-small", encoders="bf16x3", decoder="bf16x3", **ON)


@pytest.mark.parametrize("mode", MODES)
def test_graphs_the_routes_do_not_take_are_refused_by_name(mode):
    _refused(NotImplementedError, rf"decoder='{mode}': 'mini' \(DepthProForDepthEstimation\): use_batch_norm_in_fusion_residual=True.*not built",
             _mini(use_batch_norm_in_fusion_residual=True), encoders=mode, decoder=mode)
    _refused(NotImplementedError, r"fusion_hidden_size=32 -- .*64, 128 and 256 are built", _mini(fusion_hidden_size=32, intermediate_feature_dims=[32, 32]),
             encoders=mode, decoder=mode)
    _refused(NotImplementedError, r"fusion_hidden_size=96 -- ", _mini(fusion_hidden_size=96), encoders=mode, decoder=mode)
    m = _mini()
    m.head.layers[2] = torch.nn.Conv2d(32, 16, 3, padding=1)
    m.head.layers[4] = torch.nn.Conv2d(16, 1, 1)
    _refused(NotImplementedError, r"head.layers.2 writes 16 channels -- vd3d_depthpro_head and vd3d_dpt_head_tail_f32 .* are built for 32", m, encoders=mode, decoder=mode)
    # 320 / 4 = 80 is no power of two times the 4 x 4 token grid: the field-of-view features are 5 x 5 and the head would resize them
    _refused(NotImplementedError, r"at a 320 x 320 input the field-of-view head resizes its 5 x 5 features to 4 x 4 \(F.interpolate\) -- only the identity is built",
             _mini(), processor=dict(cases.mini_processor(), size=(320, 320)), encoders=mode, decoder=mode)
    m = _mini()
    m.fusion_stage.final.projection = torch.nn.Conv2d(64, 64, 3, padding=1)
    _refused(NotImplementedError, r"fusion_stage.final.projection is not a 1 x 1 convolution with C_in a multiple of 16 -- not built", m, encoders=mode, decoder=mode)


def test_a_model_without_the_field_of_view_branch_is_accepted():
    m = _mini(use_fov_model=False)
    covered = depth_pro.decoder_scope(m, "mini", "fp16x2", 256)
    assert not any(n.startswith("fov_model") for n, _ in covered) and any(n == "head.layers.4" for n, _ in covered)
    full = depth_pro.decoder_scope(_mini(), "mini", "fp16x2", 256)
    assert {"fov_model.conv", "fov_model.head.layers.0", "fov_model.head.layers.2", "fov_model.head.layers.4"} <= {n for n, _ in full}
    # every Conv2d / ConvTranspose2d of the decoder is covered, and nothing else
    m2 = _mini()
    dec = {n for n, mod in m2.named_modules() if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Linear))
           and n.startswith(("depth_pro.neck.", "fusion_stage.", "head.", "fov_model.conv", "fov_model.head."))}
    assert {n for n, _ in depth_pro.decoder_scope(m2, "mini", "bf16x3", 256)} == dec


def test_decoder_none_builds_the_pipe_as_it_was():
    m = _mini()
    pipe = DepthPipe("mini", model=m, processor=cases.mini_processor(), device="cpu")
    assert pipe.decoder is None and pipe.decoder_routes == {} and pipe.encoders is None and pipe.gemm == "f32" and pipe.arch == "depth_pro"
    for mod in (pipe.model.depth_pro.neck, pipe.model.fusion_stage, pipe.model.head, pipe.model.fov_model):
        assert "forward" not in vars(mod)   # the stock graph: no forward replaced
    x = cases.processor_in_torch(cases.frames(1, 40, 56, 3), 256)
    with torch.no_grad():
        a, b = pipe.model(pixel_values=x), _mini()(pixel_values=x)
    assert torch.equal(a.predicted_depth, b.predicted_depth) and torch.equal(a.field_of_view, b.field_of_view)


def test_switch_table():
    assert depth_pro.DECODER_SWITCHES == ("VD3D_DEPTHPRO_RES_EPI", "VD3D_DEPTHPRO_HEAD_POLY")
    assert set(depth_pro.DECODER_EPI_ROUTED) <= set(depth_pro.DECODER_EPI_BUILT) and set(depth_pro.DECODER_HEAD_POLY_ROUTED) <= set(depth_pro.DECODER_HEAD_POLY_BUILT)
    assert {s for _, s in depth_pro.DECODER_EPI_BUILT} == set(depth_pro.DECODER_EPI_SETS)
    with pytest.raises(KeyError):
        depth_pro.decoder_switch("VD3D_HEAD_FUSED")


def test_switches_read_the_environment_per_call(monkeypatch):
    for name in depth_pro.DECODER_SWITCHES:
        monkeypatch.delenv(name, raising=False)
        assert depth_pro.decoder_switch(name) is None
        monkeypatch.setenv(name, "0")
        assert depth_pro.decoder_switch(name) is False
        monkeypatch.setenv(name, "1")
        assert depth_pro.decoder_switch(name) is True
        monkeypatch.setenv(name, "yes")
        assert depth_pro.decoder_switch(name) is None


# ---- the compositions, exactly, on integer operands: ternary weights of density 0.25, inputs in [-2, 2], a 9 x 33 map, 32 and 128 channels
def _ternary(shape, g, density=0.25):
    r = torch.rand(shape, generator=g)
    return ((r < density / 2).double() - (r > 1 - density / 2).double())


@pytest.mark.parametrize("C", [32, 128])
def test_deconv_and_projection_compose_exactly(C):
    g = torch.Generator().manual_seed(C)
    wd, wp, bp = _ternary((C, C, 2, 2), g), _ternary((C, C, 1, 1), g), _ternary((C,), g)
    x = torch.randint(-2, 3, (2, C, 9, 33), generator=g).double()
    ref = F.conv2d(F.conv_transpose2d(x, wd, None, stride=2), wp, bp)
    assert float(F.conv2d(F.conv_transpose2d(x.abs(), wd.abs(), None, stride=2), wp.abs(), bp.abs()).max()) < 2 ** 24
    W = depth_pro.deconv_projection_compose(wd.float(), wp.float())
    assert W.dtype == torch.float32 and tuple(W.shape) == (C, C, 2, 2)
    assert torch.equal(F.conv_transpose2d(x, W.double(), bp, stride=2), ref)
    # random operands: float64 composition against the float64 chain
    wd, wp, x = torch.randn(C, C, 2, 2, dtype=torch.float64, generator=g) / C ** 0.5, torch.randn(C, C, dtype=torch.float64, generator=g) / C ** 0.5, x + 0.25
    W = depth_pro.deconv_projection_compose(wd, wp, torch.float64)
    err = (F.conv_transpose2d(x, W, None, stride=2) - F.conv2d(F.conv_transpose2d(x, wd, None, stride=2), wp.view(C, C, 1, 1))).abs().max()
    assert float(err) < 1e-12, float(err)
    with pytest.raises(ValueError, match="deconv_projection"):
        depth_pro.deconv_projection_compose(wd, torch.zeros(C, C + 16))


@pytest.mark.parametrize("hw", [(9, 33), (1, 1)])
@pytest.mark.parametrize("C", [32, 128])
def test_head_poly_statement_equals_the_module_chain_on_integers(C, hw):
    g = torch.Generator().manual_seed(1000 + C)
    ct, c3, c1 = torch.nn.ConvTranspose2d(C, C, 2, 2).double(), torch.nn.Conv2d(C, 32, 3, padding=1).double(), torch.nn.Conv2d(32, 1, 1).double()
    with torch.no_grad():
        for p, shape in ((ct.weight, (C, C, 2, 2)), (ct.bias, (C,)), (c3.weight, (32, C, 3, 3)), (c3.bias, (32,)), (c1.weight, (1, 32, 1, 1))):
            p.copy_(_ternary(shape, g))
        c1.bias.fill_(1.0)
        x = torch.randint(-2, 3, (3, C, *hw), generator=g).double()
        mid = c3(ct(x))
        ref = torch.relu(c1(torch.relu(mid)))[:, 0]
        # the absolute-sum bound: the sum of the magnitudes of every term of every output, far below 2^24 -- every partial sum is an exactly represented integer
        # in float32 too, whatever the order (the same case runs on the GPU in tests/test_hip_depth_pro_head_poly.py)
        mag = F.conv2d(F.conv2d(F.conv_transpose2d(x.abs(), ct.weight.abs(), ct.bias.abs(), stride=2), c3.weight.abs(), c3.bias.abs(), padding=1), c1.weight.abs(), c1.bias.abs())
        bound = float(mag.max())
        print("HEAD_POLY_ABS_SUM_BOUND", dict(C=C, hw=hw, bound=bound))
        assert bound < 2 ** 24, bound
        if hw != (1, 1):
            assert 0.2 < float((mid < 0).double().mean()) < 0.8 and float((ref == 0).double().mean()) > 0.01 and float(ref.max()) > 8   # both ReLUs engage
        for operands in (torch.float64, torch.float32):   # the blocks and the table are small integers: float32 holds them exactly
            got = depth_pro.head_poly_statement(x, ct.weight, ct.bias, c3.weight, c3.bias, c1.weight, 1.0, operands=operands)
            assert got.dtype == torch.float64 and torch.equal(got, ref)
        # the table: interior = b2 + every tap's W3 @ bt; the first row / column loses the taps above / left of the map, the last the ones below / right
        T = depth_pro.head_poly_table(ct.bias, c3.weight, c3.bias, torch.float64)
        s = torch.einsum("ocyx,c->oyx", c3.weight, ct.bias)
        assert torch.equal(T[1, 1], c3.bias + s.sum((1, 2))) and torch.equal(T[0, 1], c3.bias + s[:, 1:].sum((1, 2))) and torch.equal(T[2, 0], c3.bias + s[:, :2, 1:].sum((1, 2)))
        # ... which is what the convolution of a constant fine map gives at those pixels
        const = c3(ct.bias.view(1, C, 1, 1).expand(1, C, 6, 6))[0]
        assert torch.equal(const[:, 0, 0], T[0, 0]) and torch.equal(const[:, 3, 5], T[1, 2]) and torch.equal(const[:, 5, 2], T[2, 1])
