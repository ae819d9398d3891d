"""Training on packed mixed-length batches on the MI355X (run with -m gpu): EncoderLayer with slide_lens,
LongNetViT.forward_packed under autograd and ClassificationHead.forward_packed.

References and limits are the training path's own (tests/test_gpu_train.py, tests/test_gpu_rows_train.py):
  layer   y, dx and every parameter gradient against test_train_host.layer_model run per slide on the CPU in fp32,
          the parameter gradients summed over the slides: e <= 2 e_model, e_model the format model's deviation
          computed the same way (check_gradients, with its k_proj.bias rule);
  model   forward_packed against the same slides through forward() one at a time with gradients accumulated (the
          path that exists without packing): outputs per slide pass test_gpu_model.close_enough, every parameter
          gradient is within the sum of the two arms' bounds, 4 e_model, e_model from test_train_host.train_model
          in the format against fp32 on the CPU;
  a pack of one slide is its forward() bit for bit, dropout and drop-path included.
"""
from functools import partial

import numpy as np
import pytest
import torch

import oracle as orc
import test_gpu_train as gt
import test_train_host as host
from test_dilated_bwd_host import SCHED_B
from test_gpu_model import close_enough

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
LAYER_LENS = [257, 1500, 1, 130]
MODEL_TILES = [300, 1100, 1]
CFG2 = dict(host.CFG, depth=2)


# ----------------------------------------------------------------------------------------------
# one EncoderLayer over a packed stream
# ----------------------------------------------------------------------------------------------
def _layer_inputs():
    T = sum(LAYER_LENS)
    g = torch.Generator().manual_seed(4100 + T)
    return torch.randn(1, T, 768, generator=g), torch.randn(1, T, 768, generator=g).to(torch.float16).float()


def _layer_reference(dt):
    """layer_model per slide (fp32 for dt = None, the format model otherwise): y and dx concatenated, the parameter
    gradients summed over the slides."""
    x, gy = _layer_inputs()
    W = {k: t for k, t in host.leaf_weights().items() if k.startswith(gt.LAYER_PRE + ".")}
    ys, dxs, t0 = [], [], 0
    for L in LAYER_LENS:
        xx = x[:, t0:t0 + L].clone().requires_grad_(True)
        y = host.layer_model(xx, W, gt.LAYER_PRE, SCHED_B[0], SCHED_B[1], 16, dt)
        y.backward(gy[:, t0:t0 + L])
        ys.append(y.detach())
        dxs.append(xx.grad)
        t0 += L
    res = {"y": torch.cat(ys, 1).double().numpy(), "dx": torch.cat(dxs, 1).double().numpy()}
    for k, t in W.items():
        res[k[len(gt.LAYER_PRE) + 1:]] = t.grad.double().numpy()
    return res


@pytest.fixture(scope="module")
def layer_refs():
    return {fmt: _layer_reference(dt) for fmt, dt in (("fp32", None),) + tuple(DTYPES.items())}


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_encoder_layer_packed_gradients(fmt, layer_refs):
    layer = gt._layer()
    x, gy = _layer_inputs()
    xd = x.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
        y = layer(xd, slide_lens=LAYER_LENS)[0]
    assert y.dtype == torch.float32 and y.grad_fn is not None and y.shape == x.shape
    y.backward(gy.to(DEV))
    got = {"dx": xd.grad.double().cpu().numpy()}
    for k, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype, k
        got[k] = p.grad.double().cpu().numpy()
    ref, model = layer_refs["fp32"], layer_refs[fmt]
    ey = np.abs(y.detach().double().cpu().numpy() - ref["y"]).max() / np.abs(ref["y"]).max()
    em = np.abs(model["y"] - ref["y"]).max() / np.abs(ref["y"]).max()
    print("%s packed %s: e(y) %.3e  e_model(y) %.3e" % (fmt, LAYER_LENS, ey, em))
    assert ey <= 2 * em
    gt.check_gradients("%s packed" % fmt, got, ref, model)


def test_drop_path_is_per_slide(monkeypatch):
    """The factors forced to [0, 1 / keep] for two slides: the first slide's rows of the layer's output are its
    input rows, the second slide's are not."""
    from gigapath import runtime
    layer = gt._layer()
    layer.drop_path_prob = 0.5
    calls = []

    def forced(S, p, dev):
        calls.append((S, p))
        return torch.tensor([0.0, 1.0 / (1.0 - p)], dtype=torch.float32, device=dev)

    monkeypatch.setattr(runtime, "drop_path_slide_factors", forced)
    for fused in (True, False):
        monkeypatch.setattr(runtime, "TRAIN_ROWS_FUSED", fused)
        x = torch.randn(1, 12, 768, generator=torch.Generator().manual_seed(3)).to(DEV).requires_grad_(True)
        y = layer(x, slide_lens=[5, 7])[0]
        assert torch.equal(y[:, :5].detach(), x[:, :5].detach()), fused
        assert not torch.equal(y[:, 5:].detach(), x[:, 5:].detach())
        y.square().sum().backward()
        assert bool(torch.isfinite(x.grad).all())
    assert calls == [(2, 0.5)] * 4                       # after the attention and after the FFN, in both arms


# ----------------------------------------------------------------------------------------------
# the whole model
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def depth2():
    """A two-layer 768-wide encoder config for the tests (the registered archs start at 8 layers)."""
    from gigapath.torchscale.model import LongNetConfig
    LongNetConfig.CONFIGS["LongNet_2_layers_768_dim"] = LongNetConfig._cfg(2, 768)
    yield
    LongNetConfig.CONFIGS.pop("LongNet_2_layers_768_dim", None)


def _model2(**kw):
    from gigapath import slide_encoder
    m = slide_encoder.LongNetViT(in_chans=1536, embed_dim=768, depth=2, mlp_ratio=4,
                                 norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), **kw)
    W = orc.make_weights(CFG2, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return m.to(DEV)


def _slides(sizes, seed=40):
    out = []
    for i, n in enumerate(sizes):
        x, c = orc.synthetic_slide(n, seed_x=seed + i, seed_c=seed + 50 + i)
        out.append((torch.from_numpy(x[0]).to(DEV), torch.from_numpy(c[0]).to(DEV)))
    return out


def _grads(model):
    return {k: p.grad.detach().double().cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}


def _model_reference(dt):
    """train_model per slide on the CPU, the weighted loss summed over the slides -> parameter gradients."""
    W = host.leaf_weights(CFG2)
    loss = 0
    for i, n in enumerate(MODEL_TILES):
        x, c = orc.synthetic_slide(n, seed_x=40 + i, seed_c=90 + i)
        loss = loss + host.weighted_loss(host.train_model(W, torch.from_numpy(x), c, CFG2, dt))
    loss.backward()
    return {k: t.grad.double().numpy() for k, t in W.items() if t.grad is not None}


@pytest.fixture(scope="module")
def model_refs():
    return {fmt: _model_reference(dt) for fmt, dt in (("fp32", None),) + tuple(DTYPES.items())}


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_forward_packed_against_the_per_slide_path(fmt, depth2, model_refs):
    model = _model2(dropout=0.0, drop_path_rate=0.0).enable_training().train()
    slides = _slides(MODEL_TILES)
    with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
        packed = model.forward_packed(slides, all_layer_embed=True)
    assert len(packed) == 3 and all(len(o) == 3 for o in packed)
    assert all(t.shape == (1, 768) and t.grad_fn is not None and t.dtype == torch.float32 for o in packed for t in o)
    sum(host.weighted_loss(o) for o in packed).backward()
    gp = _grads(model)
    for p in model.parameters():
        p.grad = None
    seq = []
    for x, c in slides:
        with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
            outs = model(x[None], c[None], all_layer_embed=True)
        host.weighted_loss(outs).backward()
        seq.append([o.detach() for o in outs])
    gs = _grads(model)
    for i in range(3):
        for k in range(3):
            rel, cos, ok = close_enough(packed[i][k].detach().cpu().numpy(), seq[i][k].cpu().numpy())
            print("%s slide %d readout %d: rel %.3e cos %.6f" % (fmt, i, k, rel, cos))
            assert ok, (i, k, rel, cos)
    ref, mod = model_refs["fp32"], model_refs[fmt]
    assert set(gp) == set(gs) and len(gp) > 30
    worst = 0.0
    for k in sorted(gp):
        d = np.abs(gp[k] - gs[k]).max()
        lim = 4 * (np.abs(mod[k]).max() if k.endswith("k_proj.bias") else np.abs(mod[k] - ref[k]).max())
        print("%s %-48s |packed - sequential| %.3e  limit %.3e  ratio %.3f" % (fmt, k, d, lim, d / lim if lim else 0))
        worst = max(worst, d / lim if lim else (0.0 if d == 0 else float("inf")))
        assert d <= lim, (k, d, lim)
    print("%s worst |packed - sequential| / (4 e_model): %.3f" % (fmt, worst))


def _step(model, run, seed):
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(seed)
    outs = run()
    sum(o.square().sum() for o in outs).backward()
    return [o.detach().clone() for o in outs], {k: p.grad.clone() for k, p in model.named_parameters()
                                                 if p.grad is not None}


def test_one_slide_pack_is_the_forward_bit_for_bit(depth2):
    """dropout 0.1, drop-path 0.1, the same seed: shapes, draws and seeds coincide."""
    model = _model2(dropout=0.1, drop_path_rate=0.1).enable_training().train()
    (x, c), = _slides([300])
    o_p, g_p = _step(model, lambda: model.forward_packed([(x, c)], all_layer_embed=True)[0], 5)
    o_f, g_f = _step(model, lambda: model(x[None], c[None], all_layer_embed=True), 5)
    o_2, _ = _step(model, lambda: model.forward_packed([(x, c)], all_layer_embed=True)[0], 6)
    assert len(o_p) == len(o_f) == 3
    for a, b in zip(o_p, o_f):
        assert torch.equal(a, b)
    assert set(g_p) == set(g_f) and len(g_p) > 30
    for k in g_p:
        assert torch.equal(g_p[k], g_f[k]), k
    assert not all(torch.equal(a, b) for a, b in zip(o_p, o_2))        # another seed, another mask


def test_global_pool_readouts(depth2):
    model = _model2(dropout=0.0, drop_path_rate=0.0, global_pool=True).enable_training().train()
    slides = _slides([300, 40])
    for ale in (True, False):
        packed = model.forward_packed(slides, all_layer_embed=ale)
        for i, (x, c) in enumerate(slides):
            want = model(x[None], c[None], all_layer_embed=ale)
            assert len(packed[i]) == len(want) == (3 if ale else 1)
            for a, b in zip(packed[i], want):
                assert a.grad_fn is not None and a.shape == b.shape
                rel, cos, ok = close_enough(a.detach().cpu().numpy(), b.detach().cpu().numpy())
                assert ok, (ale, i, rel, cos)
        for p in model.parameters():
            p.grad = None
        sum(t.square().sum() for o in packed for t in o).backward()
        g = _grads(model)
        assert len(g) > 30 and all(np.isfinite(v).all() for v in g.values())
        assert np.abs(g["patch_embed.proj.weight"]).max() > 0


def test_inference_branch_is_untouched(depth2, monkeypatch):
    """Under no_grad, or in .eval() with nothing requiring grad, forward_packed is the inference engine: the bits of a
    model that never opted in, twice."""
    from gigapath import slide_encoder
    slides = _slides([300, 40, 1])
    plain = _model2(dropout=0.0, drop_path_rate=0.0).eval()
    with torch.no_grad():
        base = [torch.stack(o) for o in plain.forward_packed(slides, all_layer_embed=True)]
    model = _model2(dropout=0.0, drop_path_rate=0.0).enable_training()

    def boom(*a, **k):
        raise AssertionError("the grad path was taken")

    monkeypatch.setattr(slide_encoder.LongNetViT, "_forward_packed_grad", boom)
    model.train()
    with torch.no_grad():
        a = [torch.stack(o) for o in model.forward_packed(slides, all_layer_embed=True)]
        b = [torch.stack(o) for o in model.forward_packed(slides, all_layer_embed=True)]
    model.eval()
    c = [torch.stack(o) for o in model.forward_packed(slides, all_layer_embed=True)]
    for other in (a, b, c):
        for x, y in zip(base, other):
            assert y.grad_fn is None and torch.equal(x, y)


def test_other_head_dims_fall_back_and_still_train():
    """head_dim 96 (the 1536-wide archs): slide by slide through forward(), differentiable."""
    from gigapath import slide_encoder
    torch.manual_seed(0)
    m = slide_encoder.LongNetViT(in_chans=1536, embed_dim=1536, depth=3, mlp_ratio=4, dropout=0.0, drop_path_rate=0.0,
                                 norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)).to(DEV).enable_training().train()
    assert m.encoder.layers[0].self_attn.head_dim == 96
    slides = _slides([40, 9])
    outs = m.forward_packed(slides)
    assert len(outs) == 2 and all(len(o) == 1 and o[0].shape == (1, 1536) and o[0].grad_fn is not None for o in outs)
    sum(o[0].square().sum() for o in outs).backward()
    g = _grads(m)
    assert len(g) > 30 and all(np.isfinite(v).all() for v in g.values())
    want = m(slides[1][0][None], slides[1][1][None])[0]
    assert torch.equal(outs[1][0].detach(), want.detach())


def test_classification_head_forward_packed():
    from gigapath import classification_head
    torch.manual_seed(0)
    kw = dict(input_dim=1536, latent_dim=768, feat_layer="5-11", n_classes=2, model_arch="gigapath_slide_enc12l768d",
              pretrained="", dropout=0.0, drop_path_rate=0.0)
    head = classification_head.get_model(trainable=True, **kw).to(DEV).train()
    slides = _slides([40, 9, 1])
    logits = head.forward_packed(slides)
    assert logits.shape == (3, 2) and logits.grad_fn is not None
    torch.nn.functional.cross_entropy(logits, torch.tensor([1, 0, 1], device=DEV)).backward()
    g = _grads(head)
    enc = [k for k in g if k.startswith("slide_encoder.")]
    assert len(enc) > 100 and all(np.isfinite(g[k]).all() for k in g)
    assert np.abs(g["slide_encoder.encoder.layers.3.self_attn.q_proj.weight"]).max() > 0
    # a frozen encoder: the inference forward_packed under no_grad, only the classifier trains
    frozen = classification_head.get_model(freeze=True, **kw).to(DEV).train()
    logits = frozen.forward_packed(slides)
    assert logits.shape == (3, 2) and not frozen.slide_encoder.training
    logits.sum().backward()
    assert set(_grads(frozen)) == {"classifier.0.weight", "classifier.0.bias"}
