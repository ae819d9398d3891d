"""The training path's row kernels on the MI355X (run with -m gpu): gp_resid_drop_ln_fwd / _bwd against fp64 autograd
with gp_dropout_keep_mask's own bytes as the mask, the exact properties the issue lists, the mask itself, the
autograd wrappers of runtime, and the wiring into EncoderLayer / Encoder / LongNetViT.

Tolerances (tests/test_rows_train_host.py holds the references): e = max|G - ref64| / max|ref64| <= 2 e_model for r,
a, dx, dy, dln_w and dln_b, e_model the deviation of today's torch lines in the format from the same ref64 on the same
inputs.  Layer: fused against unfused within the sum of the two arms' bounds (2 e_model each, e_model the format
model's deviation from the fp32 model, as tests/test_gpu_train.py).  Measured worst ratios: DESIGN §3.11.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_rows_train_host as host

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
EPS = host.EPS
SEED = 0x1234567887654321
WORST = {}


def rows_per_pass(cols):
    """Rows one pass of gp_resid_drop_ln_bwd's grid covers, from the workspace size: the partials are [blocks, 2,
    cols] fp32 and stop growing once the grid is at its cap."""
    from gigapath import _hip
    f = _hip.load_library().gp_resid_drop_ln_bwd_workspace_bytes
    per = 2 * cols * 4
    cap = f(1 << 24, cols) // per
    lo = next(r for r in range(1, 1 << 16) if f(r, cols) // per == cap)     # (cap - 1) * group + 1
    return cap * ((lo - 1) // (cap - 1))


def guarded(rows, cols, dtype):
    g = torch.full((rows + 2, cols), 7.0, dtype=dtype, device=DEV)
    return g, g[1:-1]


def guards_ok(g):
    return bool((g[0] == 7).all()) and bool((g[-1] == 7).all())


def keep_mask(seed, p, rows, cols):
    """gp_dropout_keep_mask's bytes on the CPU (None for p == 0), written between guard rows."""
    from gigapath import _hip
    if p == 0:
        return None
    g, m = guarded(rows, cols, torch.uint8)
    _hip.dropout_keep_mask(seed, p, rows, cols, m)
    torch.cuda.synchronize()
    assert guards_ok(g)
    return m.cpu().clone()


def run_op(shape, inp, p, seed, dt, params=True, alias=False):
    """One forward and one backward call of the shape on device copies, every output between sentinel guard rows
    (dln_w / dln_b between guard elements), guards checked.  Returns the outputs on the CPU keyed as host.OUTPUTS."""
    from gigapath import _hip
    rows, cols = inp["x"].shape
    d = {k: (v.to(DEV) if v is not None else None) for k, v in inp.items()}
    out, guards = {}, []

    def buf(dtype):
        g, v = guarded(rows, cols, dtype)
        guards.append(g)
        return v

    add, ln = shape in ("A", "B"), shape != "B"
    x = d["x16"] if shape == "C16" else d["x"]
    r = buf(torch.float32) if add else None
    a = buf(dt) if ln else None
    _hip.resid_drop_ln_fwd(x, d["y"] if add else None, d["s"] if add else None, p if add else 0.0, seed,
                           d["w"] if ln else None, d["b"] if ln else None, EPS, r, a)
    gw = torch.full((cols + 16,), 7.0, dtype=torch.float32, device=DEV)
    gb = gw.clone()
    dw, db = (gw[8:-8], gb[8:-8]) if (params and ln) else (None, None)
    dy = buf(dt) if add else None
    if shape == "B":
        dr_in, dx = d["dr"], None
    else:
        dx = buf(dt if shape == "C16" else torch.float32)
        dr_in = d["dr"] if shape == "A" else None
        if alias:
            dx.copy_(d["dr"])
            dr_in = dx
    _hip.resid_drop_ln_bwd(d["da"] if ln else None, dr_in, (r if add else x) if ln else None, d["w"] if ln else None,
                           EPS, d["s"] if add else None, p if add else 0.0, seed, dx, dy, dw, db)
    torch.cuda.synchronize()
    assert all(guards_ok(g) for g in guards)
    for t in (gw, gb):
        assert bool((t[:8] == 7).all()) and bool((t[-8:] == 7).all())
    if dw is None:
        assert bool((gw == 7).all()) and bool((gb == 7).all())
    for k, t in (("r", r), ("a", a), ("dx", dx if shape != "B" else d["dr"]), ("dy", dy), ("dw", dw), ("db", db)):
        if t is not None:
            out[k] = t.cpu().clone()
    return out


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check_parity(tag, shape, got, r64, model):
    for k, (e, em) in host.errors(got, r64, model).items():
        ratio = e / em if em > 0 else (0.0 if e == 0 else float("inf"))
        print("%-44s %-2s e %.3e  e_model %.3e  ratio %.3f" % (tag, k, e, em, ratio))
        key = (shape, k)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        assert e <= 2 * em, (tag, k, e, em)


def variants(shape, rows, big):
    """(p, nscale): the add shapes run p in {0, 0.1} with one drop-path factor and, where rows allow, with two or
    more of which one is 0 (a dropped path); the largest shape runs one of each."""
    if shape not in ("A", "B"):
        return [(0.0, 0)]
    many = next((n for n in (2, 3, 5, 257, rows) if n > 1 and rows % n == 0), None)
    if big:
        return [(0.0, 1), (0.1, many)]
    return [(p, n) for p in (0.0, 0.1) for n in (1, many) if n is not None]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("cols", host.COLS)
def test_op_parity(cols, fmt):
    """Shapes (A), (B), (C) fp32 and 16-bit; rows 1, 3, 4, 5, 257 and 3 beyond one pass of the backward's grid."""
    dt = DTYPES[fmt]
    big = rows_per_pass(cols) + 3
    for rows in (1, 3, 4, 5, 257, big):
        for shape in host.SHAPES:
            for p, nscale in variants(shape, rows, rows == big):
                inp = host.rows_inputs(rows, cols, dt, nscale)
                mask = keep_mask(SEED + rows, p, rows, cols)
                got = run_op(shape, inp, p, SEED + rows, dt)
                check_parity("%s cols %d rows %d %s p %.1f s %d" % (fmt, cols, rows, shape, p, nscale), shape, got,
                             host.ref64(shape, inp, mask, p, dt), host.format_model(shape, inp, mask, p, dt))
    print("worst e / e_model so far: %s" % {"%s.%s" % k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_exact_cases(fmt):
    dt = DTYPES[fmt]
    rows, cols = 37, 768
    # p == 0, s == NULL: (A) is (B) followed by (C) on its r, bit for bit
    for c in host.COLS:
        inp = host.rows_inputs(rows, c, dt, 0)
        A, B = run_op("A", inp, 0.0, 0, dt), run_op("B", inp, 0.0, 0, dt)
        C = run_op("C32", dict(inp, x=B["r"]), 0.0, 0, dt)
        assert same_bits(A["r"], B["r"]) and same_bits(A["a"], C["a"]), c
    # with dropout and drop-path: dx over dr_in, a second call and a frozen LayerNorm give the same bits
    inp = host.rows_inputs(rows + 3, cols, dt, 4)
    base = run_op("A", inp, 0.1, SEED, dt)
    for other in (run_op("A", inp, 0.1, SEED, dt, alias=True), run_op("A", inp, 0.1, SEED, dt)):
        assert all(same_bits(base[k], other[k]) for k in host.OUTPUTS), [k for k in host.OUTPUTS]
    frozen = run_op("A", inp, 0.1, SEED, dt, params=False)
    assert "dw" not in frozen and same_bits(frozen["dx"], base["dx"]) and same_bits(frozen["dy"], base["dy"])
    for shape in ("C32", "C16"):
        c, c2, cf = (run_op(shape, inp, 0.0, 0, dt, params=on) for on in (True, True, False))
        assert same_bits(c["dx"], cf["dx"]) and all(same_bits(c[k], c2[k]) for k in c)
    # a row of da at +Inf: every other row of dx / dy stays finite and keeps its bits
    bad = dict(inp, da=inp["da"].clone())
    bad["da"][11] = float("inf")
    gi = run_op("A", bad, 0.1, SEED, dt)
    for k in ("dx", "dy"):
        fin = torch.isfinite(gi[k].float())
        keep = torch.ones(rows + 3, dtype=torch.bool)
        keep[11] = False
        assert bool(fin[keep].all()) and not bool(fin[11].all()), k
        assert same_bits(gi[k][keep], base[k][keep]), k
    assert not bool(torch.isfinite(gi["db"]).any())


def test_mask():
    from gigapath import _hip
    rows, cols, p = 257, 768, 0.1
    m = keep_mask(SEED, p, rows, cols)
    n = m.numel()
    frac = float(m.float().mean())
    sigma = float(np.sqrt(p * (1 - p) / n))
    print("kept fraction %.5f (1 - p = %.5f, sigma %.2e)" % (frac, 1 - p, sigma))
    assert set(m.unique().tolist()) <= {0, 1} and abs(frac - (1 - p)) <= 5 * sigma
    assert torch.equal(m, keep_mask(SEED, p, rows, cols))
    assert not torch.equal(m, keep_mask(SEED + 1, p, rows, cols))
    assert not torch.equal(m, keep_mask(SEED + (1 << 32), p, rows, cols))          # the seed's high word counts
    assert torch.equal(m[:5], keep_mask(SEED, p, 5, cols))                         # index-only dependence
    # the documented mapping, restated in numpy
    assert np.array_equal(m.numpy(), host.philox_keep_mask(SEED, p, rows, cols))
    # p == 0 keeps everything
    g, z = guarded(4, cols, torch.uint8)
    _hip.dropout_keep_mask(SEED, 0.0, 4, cols, z)
    assert bool((z == 1).all()) and guards_ok(g)
    # the kernels apply exactly this mask, forward and backward (y has no zeros, dr none to speak of)
    for fmt, dt in DTYPES.items():
        inp = host.rows_inputs(rows, cols, dt, 0)
        inp["dr"] = inp["dr"] + torch.where(inp["dr"] >= 0, 1.0, -1.0)             # |dr| >= 1: dy = 0 only if dropped
        got = run_op("B", inp, p, SEED, dt)
        assert torch.equal((got["r"] - inp["x"]) != 0, m.bool()), fmt
        assert torch.equal(got["dy"].float() != 0, m.bool()), fmt
        gotA = run_op("A", inp, p, SEED, dt)
        assert torch.equal((gotA["r"] - inp["x"]) != 0, m.bool()), fmt


# ----------------------------------------------------------------------------------------------
# the autograd wrappers
# ----------------------------------------------------------------------------------------------
def _composition(shape, d, mask, p, act, w, b):
    """The GIGAPATH_TRAIN_ROWS_FUSED=0 lines on the device with the kernel's own mask in dropout's place."""
    if shape in ("A", "B"):
        t = d["y"].float()
        if mask is not None:
            t = t * (mask.to(t.device).float() / (1.0 - p))
        if d["s"] is not None:
            t = (t.view(d["s"].numel(), -1) * d["s"].view(-1, 1)).view_as(t)
        r = d["x"] + t
    else:
        r = d["x"]
    a = None if shape == "B" else F.layer_norm(r.float(), (r.shape[-1],), w.float(), b.float(), EPS).to(act)
    return (r if shape in ("A", "B") else None), a


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("param_dtype", [torch.float32, torch.bfloat16], ids=["p32", "p16"])
def test_autograd_wrappers(fmt, param_dtype):
    from gigapath import runtime
    assert runtime.TRAIN_ROWS_FUSED
    dt = DTYPES[fmt]
    rows, cols, p = 36, 768, 0.1
    inp = host.rows_inputs(rows, cols, dt, 4)
    ln = torch.nn.LayerNorm(cols, eps=EPS).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(inp["w"])
        ln.bias.copy_(inp["b"])
    ln = ln.to(param_dtype)
    inp["w"], inp["b"] = ln.weight.detach().float().cpu(), ln.bias.detach().float().cpu()
    torch.manual_seed(77)
    seed = int(torch.empty((), dtype=torch.int64).random_())
    mask = keep_mask(seed, p, rows, cols)
    for shape in host.SHAPES:
        leaf = {k: (v.to(DEV).requires_grad_(k in ("x", "x16", "y")) if v is not None else None)
                for k, v in inp.items()}
        leaf["x"] = leaf["x16"] if shape == "C16" else leaf["x"]
        results = {}
        for arm in ("fused", "torch"):
            for t in list(leaf.values()) + [ln.weight, ln.bias]:
                if t is not None:
                    t.grad = None
            if arm == "torch":
                r, a = _composition(shape, leaf, mask if shape in ("A", "B") else None, p, dt, ln.weight, ln.bias)
            elif shape == "A":
                torch.manual_seed(77)
                r, a = runtime.resid_drop_ln_grad(leaf["x"], leaf["y"], ln, p, leaf["s"], True)
            elif shape == "B":
                torch.manual_seed(77)
                r, a = runtime.resid_drop_grad(leaf["x"], leaf["y"], p, leaf["s"], True), None
            else:
                r, a = None, runtime.layernorm_act_grad(leaf["x"], ln, act=dt)
            heads = [t for t in (r, a) if t is not None]
            assert all(t.grad_fn is not None for t in heads)
            assert a is None or a.dtype == dt
            torch.autograd.backward(heads, [leaf["dr"] if t is r else leaf["da"] for t in heads])
            res = {"dx": leaf["x"].grad}
            if r is not None:
                res["r"], res["dy"] = r.detach(), leaf["y"].grad
            if a is not None:
                assert ln.weight.grad.dtype == param_dtype and ln.bias.grad.dtype == param_dtype
                res["a"], res["dw"], res["db"] = a.detach(), ln.weight.grad, ln.bias.grad
            assert res["dx"].dtype == leaf["x"].dtype
            results[arm] = {k: v.detach().cpu().clone() for k, v in res.items()}
        r64 = host.ref64(shape, inp, mask if shape in ("A", "B") else None, p if shape in ("A", "B") else 0.0, dt)
        for k, (e, em) in host.errors(results["fused"], r64, results["torch"]).items():
            print("%s %s %-3s %-2s e %.3e  e_composition %.3e" % (fmt, param_dtype, shape, k, e, em))
            assert e <= 2 * em, (shape, k, e, em)
    # eval (training = False): no dropout, no seed drawn
    state = torch.random.get_rng_state()
    x, y = inp["x"].to(DEV), inp["y"].to(DEV)
    r = runtime.resid_drop_grad(x, y, p, None, False)
    assert torch.equal(torch.random.get_rng_state(), state) and torch.equal(r, x + y.float())


# ----------------------------------------------------------------------------------------------
# layer, encoder, model
# ----------------------------------------------------------------------------------------------
class count_calls:
    """Counts _hip.resid_drop_ln_fwd calls by shape while active."""

    def __enter__(self):
        from gigapath import _hip
        self.n = {"A": 0, "B": 0, "C32": 0, "C16": 0}
        self.orig = _hip.resid_drop_ln_fwd

        def counted(x, y, s, p, seed, ln_w, ln_b, eps, r, a):
            k = ("A" if ln_w is not None else "B") if y is not None else ("C32" if x.dtype == torch.float32 else "C16")
            self.n[k] += 1
            return self.orig(x, y, s, p, seed, ln_w, ln_b, eps, r, a)

        _hip.resid_drop_ln_fwd = counted
        return self

    def __exit__(self, *exc):
        from gigapath import _hip
        _hip.resid_drop_ln_fwd = self.orig


@pytest.fixture
def unfused_arm():
    """Flips runtime.TRAIN_ROWS_FUSED off on request and always restores it."""
    from gigapath import runtime
    before = runtime.TRAIN_ROWS_FUSED

    def set_fused(on):
        runtime.TRAIN_ROWS_FUSED = on

    yield set_fused
    runtime.TRAIN_ROWS_FUSED = before


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_encoder_layer_fused_against_unfused(fmt, unfused_arm):
    """One EncoderLayer, B = 2, L = 257, dropout 0: y, dx and every parameter gradient of the two arms agree within
    the sum of the two arms' bounds, 2 e_model each."""
    import test_gpu_train as gt
    B, L = 2, 257
    ref, model = gt._layer_reference(B, L, None), gt._layer_reference(B, L, DTYPES[fmt])
    x, gy = gt._layer_inputs(B, L)
    arms = {}
    for fused in (True, False):
        unfused_arm(fused)
        layer = gt._layer()
        xd = x.to(DEV).requires_grad_(True)
        with count_calls() as cc, torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
            y = layer(xd)[0]
        assert cc.n == ({"A": 1, "B": 1, "C32": 1, "C16": 1} if fused else {"A": 0, "B": 0, "C32": 0, "C16": 0})
        y.backward(gy.to(DEV))
        got = {"y": y.detach().double().cpu().numpy(), "dx": xd.grad.double().cpu().numpy()}
        for k, p in layer.named_parameters():
            assert p.grad is not None and p.grad.dtype == p.dtype, k
            got[k] = p.grad.double().cpu().numpy()
        arms[fused] = got
    worst = 0.0
    for k, r in ref.items():
        d = np.abs(arms[True][k] - arms[False][k]).max()
        if k.endswith("k_proj.bias"):                       # true gradient zero: the model's own magnitude
            lim = 4 * np.abs(model[k]).max()
        else:
            lim = 4 * np.abs(model[k] - r).max()
        print("%s %-40s |fused - unfused| %.3e  limit %.3e  ratio %.3f" % (fmt, k, d, lim, d / lim))
        worst = max(worst, d / lim)
        assert d <= lim, (k, d, lim)
    print("%s worst |fused - unfused| / (4 e_model): %.3f" % (fmt, worst))


def test_encoder_hand_off_is_the_layer_chain_bit_for_bit():
    """A two-layer Encoder with return_all_hiddens: layer 0's last add and layer 1's first LayerNorm are one (A) call,
    and the states are the bits of the layers called one by one."""
    from gigapath.torchscale.architecture.config import EncoderConfig
    from gigapath.torchscale.architecture.encoder import Encoder
    from test_dilated_bwd_host import SCHED_B
    args = EncoderConfig(encoder_embed_dim=768, encoder_attention_heads=16, encoder_ffn_embed_dim=3072,
                         encoder_layers=2, segment_length=list(SCHED_B[0]), dilated_ratio=list(SCHED_B[1]),
                         flash_attention=True)
    torch.manual_seed(1)
    enc = Encoder(args).to(DEV).train()
    for m in enc.modules():
        if hasattr(type(m), "trainable"):
            m.trainable = True
    x = torch.randn(2, 130, 768, device=DEV)
    with count_calls() as cc:
        out = enc(None, token_embeddings=x.clone().requires_grad_(True), return_all_hiddens=True)
    assert cc.n == {"A": 3, "B": 1, "C32": 1, "C16": 2}, cc.n
    states = out["encoder_states"]
    h = x
    with count_calls() as cc:
        for i, layer in enumerate(enc.layers):
            h = layer(h.requires_grad_(True))[0].detach()
            assert torch.equal(states[i + 1].detach(), h), i
    assert cc.n == {"A": 2, "B": 2, "C32": 2, "C16": 2}, cc.n
    out["encoder_out"].square().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in enc.parameters())


def test_model_step_with_dropout_and_drop_path():
    """300 tiles, dropout 0.1 / drop-path 0.1 through the fused rows: finite, the same bits under the same
    torch.manual_seed, different under another."""
    import test_gpu_train as gt
    model = gt._model(dropout=0.1, drop_path_rate=0.1).enable_training().train()
    x, coords = gt._slide(300)
    with count_calls() as cc:
        l0, g0 = gt._loss_and_grads(model, x, coords, 5)
    assert cc.n == {"A": 23, "B": 1, "C32": 1, "C16": 12}, cc.n
    l1, g1 = gt._loss_and_grads(model, x, coords, 5)
    l2, _ = gt._loss_and_grads(model, x, coords, 6)
    assert bool(torch.isfinite(l0)) and all(bool(torch.isfinite(g).all()) for g in g0) and len(g0) > 200
    assert torch.equal(l0, l1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert not torch.equal(l0, l2)
