"""The trainable slide encoder, CPU side (no GPU): gp_gelu_layernorm_bwd rejects bad arguments on the host, the
closed form of the GELU + LayerNorm backward is checked against fp64 autograd, the opt-in surface behaves as
documented, and train_model -- a torch restatement of the training path with a pluggable rounding -- is pinned
to the oracle's forward and to the reference's own gradients (tests/golden/train_grads_N1300.npz).

train_model / layer_model with dt = None are the fp32 references the GPU tests (tests/test_gpu_train.py) compare
against; with a 16-bit dt they are the format model: every tensor the GPU path holds in 16 bits is rounded (GEMM
operands and outputs with the weight casts, LN outputs, the attention seam's attn_rounding_model, merged, the
GELU output -- straight-through, as the fused kernel keeps dg in fp32 -- and the FFN-LN output).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as orc
from conftest import load_golden
from test_attn_bwd_host import FAKE, attn_fp32, attn_rounding_model
from test_dilated_bwd_host import LN2, LOG2E, dilated_core

CFG = orc.arch_config("gigapath_slide_enc12l768d")
FP32_RESTATEMENT = 2e-5
COLS = (3072, 4096, 6144)
LOSS_SEED = 13


# ----------------------------------------------------------------------------------------------
# GELU + LayerNorm: the fp64 reference, the reference's lines in the format (e_model), the closed form
# ----------------------------------------------------------------------------------------------
def gelu_ln_inputs(rows, cols, dt, seed=0):
    """h, dy in dt; ln_w, ln_b fp32 (seeded)."""
    g = torch.Generator().manual_seed(1000 * seed + rows + cols)
    h = (1.5 * torch.randn(rows, cols, generator=g)).to(dt)
    dy = torch.randn(rows, cols, generator=g).to(dt)
    w = 1.0 + 0.2 * torch.randn(cols, generator=g)
    b = 0.1 * torch.randn(cols, generator=g)
    return h, dy, w, b


def gelu_ln_ref64(h, dy, w, b, eps):
    """fp64 autograd of y = LN(round(gelu(h))) w + b on the 16-bit h and dy, the rounding straight-through.
    Returns y, dh, dw, db as fp64."""
    h64 = h.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    g = F.gelu(h64)
    g = g + (g.detach().float().to(h.dtype).double() - g.detach())
    y = F.layer_norm(g, (h.shape[1],), w64, b64, eps)
    y.backward(dy.double())
    return y.detach(), h64.grad, w64.grad, b64.grad


def gelu_ln_format_model(h, dy, w, b, eps):
    """The reference's own lines (feedforward_network.py:135-138) by torch in the format: gelu(x.float())
    .type_as(x), then the LayerNorm in fp32 as autocast runs it.  Its backward rounds dg, then dh."""
    hh = h.clone().requires_grad_(True)
    w32, b32 = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    x = F.gelu(hh.float()).type_as(hh)
    y = F.layer_norm(x.float(), (h.shape[1],), w32, b32, eps)
    y.backward(dy.float())
    return y.detach(), hh.grad, w32.grad, b32.grad


def gelu_ln_closed_form(h, dy, w, b, eps):
    """gp_gelu_layernorm_bwd's arithmetic in torch: fp32 throughout, dh rounded once."""
    dt = h.dtype
    C = h.shape[1]
    x = h.float()
    g = F.gelu(x).to(dt).float()
    mean = g.mean(1, keepdim=True)
    rstd = torch.rsqrt(((g - mean) ** 2).mean(1, keepdim=True) + eps)
    xhat = (g - mean) * rstd
    d = dy.float()
    dxhat = d * w
    dg = rstd * (dxhat - dxhat.sum(1, keepdim=True) / C - xhat * ((dxhat * xhat).sum(1, keepdim=True) / C))
    gp = 0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327
    return (xhat * w + b).to(dt), (dg * gp).to(dt), (d * xhat).sum(0), d.sum(0)


def rel_err(got, ref):
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max())


# ----------------------------------------------------------------------------------------------
# the training path restated: one layer, then the whole model
# ----------------------------------------------------------------------------------------------
def _rnd(t, dt):
    """Round to dt, stay fp32; autograd rounds the gradient the same way on its way back."""
    return t.to(dt).float() if dt is not None else t


def _rnd_st(t, dt):
    """Round the value only (straight-through)."""
    return t + (t.detach().to(dt).float() - t.detach()) if dt is not None else t


def _ln(x, W, pre, eps):
    return F.layer_norm(x, (x.shape[-1],), W[pre + ".weight"], W[pre + ".bias"], eps)


def _lin(x, W, pre, dt, scale=1.0):
    return _rnd(F.linear(x, _rnd(W[pre + ".weight"] * scale, dt), _rnd(W[pre + ".bias"] * scale, dt)), dt)


def seam_of(dt):
    return attn_fp32 if dt is None else attn_rounding_model(dt)


def layer_model(x, W, pre, segs, ratios, H, dt=None, eps=1e-5):
    """EncoderLayer's differentiable path on the fp32 residual stream x [B, L, E] (oracle.encoder_layer's
    structure; the attention core is test_dilated_bwd_host.dilated_core)."""
    B, L, E = x.shape
    D = E // H
    fold = dt is not None and D in (48, 64)
    qs = (D ** -0.5) * LOG2E if fold else 1.0
    a = _rnd(_ln(x, W, pre + ".self_attn_layer_norm", eps), dt)
    q, k, v = (_lin(a, W, pre + ".self_attn." + n, dt, s).view(B, L, H, D)
               for n, s in (("q_proj", qs), ("k_proj", 1.0), ("v_proj", 1.0)))
    merged = _rnd(dilated_core(q, k, v, segs, ratios, seam_of(dt), LN2 if fold else None), dt)
    a = _lin(_rnd(_ln(merged, W, pre + ".self_attn.inner_attn_ln", eps), dt), W, pre + ".self_attn.out_proj", dt)
    x = x + a
    f = _rnd(_ln(x, W, pre + ".final_layer_norm", eps), dt)
    h = _lin(f, W, pre + ".ffn.fc1", dt)
    g = _rnd_st(F.gelu(h), dt)
    y = _rnd(_ln(g, W, pre + ".ffn.ffn_layernorm", eps), dt)
    return x + _lin(y, W, pre + ".ffn.fc2", dt)


def train_model(W, x, coords, cfg, dt=None, layers=None):
    """LongNetViT's differentiable forward with all_layer_embed: x [B, N, C] tensor (may require grad), coords
    numpy -> the 1 + depth readouts [B, E] (CLS row through self.norm)."""
    B, N, _ = x.shape
    E, H, G = cfg["embed_dim"], cfg["heads"], cfg["slide_ngrids"]
    h = _lin(_rnd(x, dt), W, "patch_embed.proj", dt)
    pos = orc.coords_to_pos(coords, G, cfg["tile_size"])
    h = h + torch.from_numpy(orc.pos_embed_rows(pos, orc.sincos_axis_table(E, G), G)).to(h.dtype)
    h = torch.cat([W["cls_token"].view(1, 1, E).expand(B, 1, E), h], dim=1)
    states = [h]
    for li in range(cfg["depth"] if layers is None else layers):
        h = layer_model(h, W, "encoder.layers.%d" % li, cfg["segment_length"], cfg["dilated_ratio"], H, dt,
                        cfg["ln_eps"])
        states.append(h)
    return [_ln(t[:, 0], W, "norm", cfg["norm_eps"]) for t in states]


def loss_weights(n_out, E):
    """The seeded, fp16-stored weighting of the readouts that defines the golden's scalar loss."""
    return np.random.Generator(np.random.PCG64(LOSS_SEED)).standard_normal((n_out, E)).astype(np.float16)


def weighted_loss(outs):
    w = torch.from_numpy(loss_weights(len(outs), outs[0].shape[-1]).astype(np.float32))
    return sum(((o if o.dtype == torch.float64 else o.float()).cpu() * w[i]).sum() for i, o in enumerate(outs))


def leaf_weights(cfg=CFG, seed=0):
    return {k: torch.from_numpy(v).requires_grad_(True) for k, v in orc.make_weights(cfg, seed=seed).items()}


# ----------------------------------------------------------------------------------------------
# host checks of the C ABI
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from test_abi_and_api import _lib_path
    _lib_path()
    from gigapath import _hip
    return _hip.load_library()


def _call(lib, h=FAKE, dy=FAKE + (1 << 30), ln_w=FAKE, dh=FAKE + (2 << 30), dw=FAKE, db=FAKE, ws=FAKE,
          ws_bytes=1 << 40, rows=8, cols=3072, fmt=0):
    return lib.gp_gelu_layernorm_bwd(h, dy, ln_w, 1e-5, dh, dw, db, ws, ws_bytes, rows, cols, fmt, None)


def test_symbols_are_exported_under_abi_13(lib):
    from gigapath import _hip
    assert lib.gp_abi_version() == 13 == _hip.ABI_VERSION
    for name in ("gp_gelu_layernorm_bwd", "gp_gelu_layernorm_bwd_workspace_bytes"):
        assert name in _hip.SIGNATURES
        assert getattr(lib, name) is not None


def test_argument_errors_are_rejected_on_the_host(lib):
    err = lib.gp_last_error_string
    assert _call(lib, fmt=7) == -1 and b"bad fmt 7" in err()
    assert _call(lib, fmt=2) == -1 and b"bad fmt 2" in err()                      # GP_FMT_F16_VBF16
    assert _call(lib, cols=3000) == -1 and b"cols=3000 unsupported" in err()
    assert _call(lib, cols=768) == -1 and b"cols=768 unsupported" in err()
    assert _call(lib, rows=-1) == -1 and b"bad rows" in err()
    for kw in ({"h": None}, {"dy": None}, {"ln_w": None}, {"dh": None}):
        assert _call(lib, **kw) == -1 and b"null pointer" in err(), kw
    assert _call(lib, dw=None) == -1 and b"both be given or both be null" in err()
    assert _call(lib, db=None) == -1 and b"both be given or both be null" in err()
    assert _call(lib, rows=1 << 31) == -1 and b"too many rows" in err()
    assert _call(lib, dh=FAKE) == -1 and b"dh must not alias h" in err()
    assert _call(lib, dh=FAKE + 4096) == -1 and b"dh must not alias h" in err()    # partial overlap
    assert _call(lib, dh=FAKE + (1 << 30) + 4096) == -1 and b"only as the same buffer" in err()
    need = lib.gp_gelu_layernorm_bwd_workspace_bytes(8, 3072)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == -1 and b"workspace too small" in err()
    assert _call(lib, ws=None) == -1 and b"workspace too small" in err()
    assert _call(lib, h=FAKE + 2) == -1 and b"misaligned" in err()
    assert _call(lib, ws=FAKE + 4) == -1 and b"misaligned workspace" in err()
    assert _call(lib, rows=0, h=None, dy=None, dh=None) == 0                       # nothing to do


def test_workspace_is_monotone_in_rows(lib):
    f = lib.gp_gelu_layernorm_bwd_workspace_bytes
    for cols in COLS:
        rows = [1, 2, 3, 4, 5, 8, 9, 257, 1024, 2048, 4096, 4097, 70001, 1 << 20]
        sizes = [f(r, cols) for r in rows]
        assert sizes[0] >= 2 * cols * 4 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] == sizes[-2]                   # the grid is capped: the partials stop growing
        assert all(s % (2 * cols * 4) == 0 for s in sizes)
        assert f(0, cols) == 0 and f(-1, cols) == 0
    assert f(8, 768) == 0 and f(8, 3000) == 0


# ----------------------------------------------------------------------------------------------
# the closed form
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", [5, 257])
def test_closed_form_matches_fp64_autograd(rows, dt):
    """Section 1's formulas (fp32, one rounding) against fp64 autograd: dh no further from it than the
    reference's own two-rounding lines in the format (e_model), the fp32 sums within 2e-5."""
    h, dy, w, b = gelu_ln_inputs(rows, 3072, dt)
    y64, dh64, dw64, db64 = gelu_ln_ref64(h, dy, w, b, 1e-5)
    _, dhm, _, _ = gelu_ln_format_model(h, dy, w, b, 1e-5)
    y, dh, dw, db = gelu_ln_closed_form(h, dy, w, b, 1e-5)
    e, em = rel_err(dh, dh64), rel_err(dhm, dh64)
    print("rows %d %s: e(dh) %.3e  e_model(dh) %.3e  ratio %.2f  e(dw) %.2e  e(db) %.2e"
          % (rows, dt, e, em, e / em, rel_err(dw, dw64), rel_err(db, db64)))
    assert e <= em
    assert rel_err(dw, dw64) <= FP32_RESTATEMENT and rel_err(db, db64) <= FP32_RESTATEMENT
    assert rel_err(y, y64) <= 2.0 ** (-8 if dt == torch.bfloat16 else -11)      # one rounding of an O(1) row


# ----------------------------------------------------------------------------------------------
# the fp32 model is the oracle's (and the reference's) function
# ----------------------------------------------------------------------------------------------
def test_fp32_model_matches_oracle_forward():
    """train_model(dt=None) against oracle.slide_encoder_forward: the 13 readouts and the loss within 2e-5 of
    max|ref|.  The gradients are pinned to the reference's own autograd below, not to the oracle's: the oracle's
    merge differentiates through the branch weights, which the reference computes under torch.no_grad()
    (dilated_attention.py:119-124), so its parameter gradients are those of another function (cls_token differs
    by 1.4e-2 of max|ref| at N = 300)."""
    N = 300
    x_np, coords = orc.synthetic_slide(N)
    W = {k: torch.from_numpy(v) for k, v in orc.make_weights(CFG, seed=0).items()}
    with torch.no_grad():
        got = torch.stack(train_model(W, torch.from_numpy(np.asarray(x_np, dtype=np.float32)), coords, CFG))
        ref = torch.stack(orc.slide_encoder_forward(W, x_np, coords, CFG, all_layer_embed=True))
    assert float((got - ref).abs().max()) <= FP32_RESTATEMENT * float(ref.abs().max())
    lg, lr = float(weighted_loss(list(got))), float(weighted_loss(list(ref)))
    assert abs(lg - lr) <= FP32_RESTATEMENT * abs(lr)


def apply_fp64_correction(g, corr):
    """The golden's arrays moved from the reference's fp32 run to its fp64 run (float64 arrays)."""
    for k in [k for k in corr if k.startswith("c:")]:
        key = k[2:]
        g[key] = g[key].astype(np.float64) + corr[k].astype(np.float64) * float(corr["s:" + key])
    g["loss"] = corr["loss64"]
    return g


def load_train_golden(fp64=False):
    """train_grads_N1300.npz and its second part (the 2-D weight rows) as one dict: the reference's fp32 run, or,
    with fp64, its fp64 run (train_grads_N1300_f64.npz applied)."""
    g = load_golden("train_grads_N%d.npz" % GOLDEN_N)
    g.update(load_golden("train_grads_N%d_w.npz" % GOLDEN_N))
    return apply_fp64_correction(g, load_golden("train_grads_N%d_f64.npz" % GOLDEN_N)) if fp64 else g


@pytest.fixture(scope="module")
def golden_vs_model():
    return load_train_golden(fp64=True), model_gradients(None, double=True)


@pytest.mark.parametrize("part", ["outputs", "dx", "top", "layers.0.", "layers.5.", "layers.11."])
def test_fp32_model_matches_reference_golden(part, golden_vs_model):
    """train_model(dt=None) against the outputs and gradients of the reference's fp64 run
    (tests/golden/make_golden_train.py): within 2e-5 of max|ref| per stored array.  Both sides are evaluated in
    fp64, so what is compared is the function: in fp32 the reference's own run is 3.6e-5 (layer 5's d q_proj.weight)
    and 2.2e-5 (its d q_proj.bias) of max|ref| from its fp64 run, and the model's fp32 run 2.1e-5, all rounding of
    small differences of large terms.  Measured: every stored array within 3e-7."""
    g, got = golden_vs_model
    if part == "outputs":
        assert np.abs(got["outs"] - g["outs"]).max() <= FP32_RESTATEMENT * np.abs(g["outs"]).max()
        assert abs(got["loss"] - float(g["loss"])) <= FP32_RESTATEMENT * abs(float(g["loss"]))
        return
    keys = [k for k in golden_gradient_keys(g) if not k.endswith("k_proj.bias")]
    if part == "dx":
        keys = ["dx"]
    elif part == "top":
        keys = [k for k in keys if k != "dx" and ".layers." not in k]
    else:
        keys = [k for k in keys if ".%s" % part in k]
    assert keys
    worst = max((np.abs(select_like_golden(got, k, g) - g[k]).max() / np.abs(g[k]).max(), k) for k in keys)
    print(part, "worst %.2e at %s" % worst)
    assert worst[0] <= FP32_RESTATEMENT, worst


GOLDEN_N = 1300
GOLDEN_LAYERS = (0, 5, 11)
ROW_SEED = 17


def golden_rows(name, n_rows):
    """The eight seeded rows of a 2-D weight gradient the golden stores."""
    seed = ROW_SEED + sum(ord(c) for c in name)
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(n_rows, size=8, replace=False))


def golden_selection(W_shapes):
    """name -> None (stored whole) or the row indices stored, for every gradient the golden keeps."""
    sel = {"cls_token": None, "norm.weight": None, "norm.bias": None, "patch_embed.proj.bias": None}
    for li in GOLDEN_LAYERS:
        pre = "encoder.layers.%d." % li
        for k, shp in W_shapes.items():
            if k.startswith(pre):
                sel[k] = None if len(shp) == 1 else golden_rows(k, shp[0])
    return sel


def model_gradients(dt, N=GOLDEN_N, double=False):
    """loss, dx and the parameter gradients of train_model on synthetic_slide(N), as float64 numpy.  double: the
    fp32 model's arithmetic in fp64 (dt must be None)."""
    x_np, coords = orc.synthetic_slide(N)
    W = leaf_weights()
    x = torch.from_numpy(np.asarray(x_np, dtype=np.float32)).requires_grad_(True)
    if double:
        W = {k: t.detach().double().requires_grad_(True) for k, t in W.items()}
        x = x.detach().double().requires_grad_(True)
    outs = train_model(W, x, coords, CFG, dt)
    loss = weighted_loss(outs)
    loss.backward()
    res = {"loss": float(loss.detach()), "dx": x.grad.double().numpy(), "outs": torch.stack(outs).detach().double().numpy()}
    for k, t in W.items():
        if t.grad is not None:                   # encoder.layer_norm is not on the all_layer_embed path
            res[k] = t.grad.double().numpy()
    return res


def golden_gradient_keys(g):
    return [k for k in g if k == "dx" or k.startswith("d:")]


def select_like_golden(got, key, g):
    """The part of a full gradient the golden stores under `key` ('dx', or 'd:<param name>')."""
    if key == "dx":
        return got["dx"][:, ::16]
    name = key[2:]
    val = got[name]
    rows_key = "rows:" + name
    return val[g[rows_key]] if rows_key in g else val


# ----------------------------------------------------------------------------------------------
# the opt-in surface
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from gigapath import slide_encoder
    return slide_encoder.create_model("", "gigapath_slide_enc12l768d", 1536)


def test_enable_training_reaches_every_trainable_module(model):
    from gigapath.torchscale.architecture.encoder import Encoder, EncoderLayer
    from gigapath.torchscale.component.feedforward_network import FeedForwardNetwork
    kinds = (type(model), Encoder, EncoderLayer, FeedForwardNetwork)
    mods = [m for m in model.modules() if isinstance(m, kinds)]
    assert len(mods) == 1 + 1 + 12 + 12 and not any(m.trainable for m in mods)
    assert model.enable_training() is model
    assert all(m.trainable for m in mods)
    assert not hasattr(model.encoder.layers[0].self_attn, "trainable")      # DilatedAttention keeps its own rule
    model.enable_training(False)
    assert not any(m.trainable for m in mods)


def test_opt_in_errors_on_the_cpu(model):
    x, c = torch.zeros(1, 4, 1536), torch.zeros(1, 4, 2)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):                     # no opt-in: today's error
            model(x, c)
        model.enable_training()
        with pytest.raises(RuntimeError, match="ROCm"):                     # opted in: the path needs the GPU
            model(x, c)
        with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):    # no autograd: the inference path
            model(x, c)
    finally:
        model.enable_training(False)
        model.eval()


def test_classification_head_trainable():
    from gigapath import classification_head
    kw = dict(input_dim=1536, latent_dim=768, feat_layer="5-11", n_classes=3,
              model_arch="gigapath_slide_enc12l768d", pretrained="")
    head = classification_head.get_model(trainable=True, **kw)
    assert all(p.requires_grad for p in head.slide_encoder.parameters())
    assert head.slide_encoder.trainable and head.slide_encoder.encoder.layers[3].ffn.trainable
    head.train()
    assert head.slide_encoder.training
    head.eval()
    assert not head.slide_encoder.training
    frozen = classification_head.get_model(trainable=True, freeze=True, **kw)
    assert not any(p.requires_grad for p in frozen.slide_encoder.parameters())
    assert not frozen.slide_encoder.trainable
    frozen.train()
    assert not frozen.slide_encoder.training
    assert sum(p.requires_grad for p in frozen.parameters()) == 2


def test_classification_head_environment_default(monkeypatch):
    from gigapath import classification_head
    kw = dict(input_dim=1536, latent_dim=768, feat_layer="11", model_arch="gigapath_slide_enc12l768d", pretrained="")
    monkeypatch.setenv("GIGAPATH_TRAINABLE", "1")
    assert classification_head.get_model(**kw).encoder_trainable
    assert not classification_head.get_model(freeze=True, **kw).encoder_trainable
    monkeypatch.delenv("GIGAPATH_TRAINABLE")
    assert not classification_head.get_model(**kw).encoder_trainable


def test_pos_rows_helper_is_bit_equal_to_the_oracle():
    from gigapath.pos_embed import axis_table, pos_rows
    G = 1000
    g = load_golden("pos_embed_rows.npz")
    rng = np.random.Generator(np.random.PCG64(5))
    pos = np.concatenate([g["rows"].reshape(-1), np.array([0, 1, G, G * G, -1, -(G * G)], dtype=np.int64),
                          rng.integers(0, G * G + 1, size=500)])
    tab = axis_table(768, G)
    ours = pos_rows(torch.from_numpy(tab), torch.from_numpy(pos).view(2, -1), G).numpy().reshape(-1, 768)
    ref = orc.pos_embed_rows(pos, tab, G)
    assert np.array_equal(ours.view(np.uint32), ref.view(np.uint32))


def test_drop_path_helper():
    from gigapath import runtime
    torch.manual_seed(3)
    x = torch.randn(4, 8, 16)
    assert runtime.drop_path(x, 0.3, False) is x and runtime.drop_path(x, 0.0, True) is x
    seen = set()
    for _ in range(20):
        y = runtime.drop_path(x, 0.3, True)
        for b in range(4):
            zero, kept = bool((y[b] == 0).all()), torch.allclose(y[b], x[b] / 0.7, rtol=1e-6, atol=0)
            assert zero or kept
            seen.add(zero)
    assert seen == {True, False}
