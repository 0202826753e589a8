"""Host tests (no GPU) of tests/outlier_weights.py: the stock DA-V2-Small graph in float64 on the CPU must show, under these weights, the statistics that make
tests/test_hip_depth_f64.py meaningful.  Every condition is one the reference alone satisfies -- no kernel of the library runs here."""
import math

import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

import outlier_weights as ow   # noqa: E402

LOG2E = math.log2(math.e)


@pytest.fixture(scope="module", params=[0, 1, 2])
def probed(request):
    """One float64 forward per seed with hooks: per nn.Linear (max |x|, median |x|, the smallest row maximum) of its input, per layer the widest per-query
    spread of the attention logits in exp2 units; plus the float64 and float32 predictions."""
    seed = request.param
    lin, qk, cfg = {}, {}, {}

    def pre(name):
        def hook(_mod, inp):
            x = inp[0].abs().reshape(-1, inp[0].shape[-1])
            lin[name] = (float(x.max()), float(x.median()), float(x.max(dim=1).values.min()))
        return hook

    def keep(name):
        def hook(_mod, _inp, out):
            qk[name] = out
        return hook

    def instrument(model):
        for n, m in model.named_modules():
            if isinstance(m, torch.nn.Linear):
                m.register_forward_pre_hook(pre(n))
                if n.endswith(".query") or n.endswith(".key"):
                    m.register_forward_hook(keep(n))
        att = model.backbone.encoder.layer[0].attention.attention
        cfg.update(nh=att.num_attention_heads, hd=att.attention_head_size, scaling=att.scaling, layers=len(model.backbone.encoder.layer))
    p64, p32 = ow.reference_predictions(seed, instrument)
    nh, hd = cfg["nh"], cfg["hd"]
    spans = []
    for li in range(cfg["layers"]):
        q, k = (qk[f"backbone.encoder.layer.{li}.attention.attention.{p}"] for p in ("query", "key"))
        B, T, _ = q.shape
        logits = (q.view(B, T, nh, hd).transpose(1, 2) @ k.view(B, T, nh, hd).permute(0, 2, 3, 1)) * (cfg["scaling"] * LOG2E)
        spans.append(float((logits.max(-1).values - logits.min(-1).values).max()))
    return dict(seed=seed, lin=lin, spans=spans, p64=p64, p32=p32)


def test_input_is_406_tokens(probed):
    assert tuple(probed["p64"].shape) == (2, 210, 378) and (210 // 14) * (378 // 14) + 1 == 406


def test_some_linear_sees_massive_activations(probed):
    """max |x| >= 50 with max / median >= 100 (the synthetic weights: 5.4)."""
    best = max(probed["lin"].values(), key=lambda s: s[0] / s[1] if s[0] >= 50 else 0.0)
    print("massive:", best)
    assert best[0] >= 50.0 and best[0] / best[1] >= 100.0, best


def test_some_linear_sees_a_row_that_is_small_everywhere(probed):
    small = min(s[2] for s in probed["lin"].values())
    print("smallest row maximum:", small)
    assert small < 2.0 ** -4, small


def test_some_attention_is_nearly_one_hot(probed):
    """The logits of one query span >= 40 in exp2 units: every probability but a few is below 2^-40 of the largest."""
    print("logit spans per layer:", [round(s, 1) for s in probed["spans"]])
    assert max(probed["spans"]) >= 40.0, probed["spans"]


def test_prediction_is_off_the_relu_floor(probed):
    p64 = probed["p64"]
    floor = float((p64 == 0).double().mean())
    print("range", float(p64.max() - p64.min()), "at the floor", floor)
    assert bool(torch.isfinite(p64).all()) and float(p64.max() - p64.min()) > 0.0
    assert floor <= 0.25, floor


def test_float32_error_is_measurable_and_small(probed):
    """The float32 CPU graph against float64: finite and between 1e-6 and 1e-2 of the range, so that a ratio against it means something."""
    E, rms = ow.errors_of_range(probed["p32"], probed["p64"])
    print("float32 CPU vs float64: E", E, "RMS", rms)
    assert bool(torch.isfinite(probed["p32"]).all())
    assert 1e-6 <= E <= 1e-2, E
    assert 0.0 < rms <= E


def test_recipe_is_deterministic_and_seeded():
    a, b, c = ow.stock_model(0, torch.float32), ow.stock_model(0, torch.float32), ow.stock_model(1, torch.float32)
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert any(not torch.equal(sa[k], sc[k]) for k in sa)
