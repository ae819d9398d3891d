"""gp_dilated_attn_bwd and the differentiable DilatedAttention module on the MI355X (run with -m gpu).

Op parity: e(G) = max|G - G_ref| / max|G_ref| for G in {dq, dk, dv}; G_ref is the fp32 CPU autograd of
test_dilated_bwd_host.dilated_core (pinned there to the reference's own golden) with the fp32 attention at the
seam, on the same 16-bit q, k, v and dmerged.  Limit: e_kernel <= 2 e_model, e_model from the same restatement
with test_attn_bwd_host.attn_rounding_model at the seam (the project's rule for gp_seg_attn_bwd).  The model rounds
each branch's gradients to the format before autograd sums them; the kernel sums the branches in fp32 and rounds
once.  Where G_ref is identically zero (L = 1: one key, dS = 0) the kernel
must return exact zeros.
"""
import numpy as np
import pytest
import torch

import test_attn_bwd_host as seam_host
import test_dilated_bwd_host as host
from conftest import load_golden
from test_gpu_model import close_enough

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 16
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SCHEDS = {"A": host.SCHED_A, "B": host.SCHED_B}
SENTINEL = -1024.0
FP32_RESTATEMENT = 2e-5


def _hip():
    from gigapath import _hip as h
    h.load_library()
    return h


def _inputs(seed, B, L, D, dt, qk_scale=1.0, q_scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    q, k, v = (torch.from_numpy(rng.standard_normal((B, L, H, D)).astype(np.float32)) for _ in range(3))
    dm = torch.from_numpy(rng.standard_normal((B, L, H * D)).astype(np.float32))
    return (q * qk_scale * q_scale).to(dt), (k * qk_scale).to(dt), v.to(dt), dm.to(dt)


def _geometry(L, sl, r):
    s = min(sl, L)
    return s, -(-L // s), -(-s // r)


def _kernel(q, k, v, dm, segs, ratios, prescaled=False, nan_fill=False, full=False):
    """Forward + backward through the C ABI.  Returns (dq, dk, dv) [B, L, H, D] on the CPU; with full also the
    sentinel guard rows around dqkv and the forward's LSEs."""
    h = _hip()
    B, L, _, D = q.shape
    E, M = H * D, B * L
    qkv = torch.cat([t.reshape(M, E) for t in (q, k, v)], 1).to(DEV).contiguous()
    outs, lses = [], []
    for sl, r in zip(segs, ratios):
        s, nseg, m = _geometry(L, sl, r)
        outs.append(torch.full((B * nseg * m * H * D,), float("nan") if nan_fill else 0.0, dtype=q.dtype, device=DEV))
        lses.append(torch.full((B * nseg * H * m,), float("nan") if nan_fill else 0.0, dtype=torch.float32,
                               device=DEV))
    h.dilated_attn_fwd(qkv, qkv[:, E:], qkv[:, 2 * E:], 3 * E, B, L, H, D, segs, ratios, outs, lses, 0.0, prescaled)
    buf = torch.full((M + 2, 3 * E), SENTINEL, dtype=q.dtype, device=DEV)
    dqkv = buf[1:-1]
    h.dilated_attn_bwd(qkv, qkv[:, E:], qkv[:, 2 * E:], 3 * E, B, L, H, D, segs, ratios, outs, lses,
                       dm.reshape(M, E).to(DEV).contiguous(), dqkv, dqkv[:, E:], dqkv[:, 2 * E:], 3 * E, 0.0, prescaled)
    torch.cuda.synchronize()
    grads = tuple(dqkv[:, i * E:(i + 1) * E].cpu().view(B, L, H, D) for i in range(3))
    if full:
        return grads, torch.cat([buf[0], buf[-1]]).cpu(), [l.cpu() for l in lses]
    return grads


def _cpu_grads(seam, q, k, v, dm, segs, ratios, scale=None):
    ql, kl, vl = (t.float().requires_grad_(True) for t in (q, k, v))
    host.dilated_core(ql, kl, vl, segs, ratios, seam, scale).backward(dm.float())
    return ql.grad, kl.grad, vl.grad


def _parity(name, q, k, v, dm, segs, ratios, prescaled=False):
    dt = q.dtype
    scale = host.LN2 if prescaled else None          # pre-scaled q': the logit is q'.k ln 2, differentiated w.r.t. q'
    ref = _cpu_grads(seam_host.attn_fp32, q, k, v, dm, segs, ratios, scale)
    model = _cpu_grads(seam_host.attn_rounding_model(dt), q, k, v, dm, segs, ratios, scale)
    got = _kernel(q, k, v, dm, segs, ratios, prescaled)
    bad = []
    for nm, g, m, r in zip(("dq", "dk", "dv"), got, model, ref):
        assert torch.isfinite(g.float()).all(), (name, nm)
        if r.abs().max().item() == 0.0:
            print("dilated_bwd parity %s %s: reference identically zero" % (name, nm))
            assert (g == 0).all(), (name, nm)
            continue
        ek = ((g.float() - r).abs().max() / r.abs().max()).item()
        em = ((m - r).abs().max() / r.abs().max()).item()
        print("dilated_bwd parity %s %s: e_kernel %.3e e_model %.3e ratio %.2f" % (name, nm, ek, em, ek / em))
        if not ek <= 2 * em:
            bad.append((nm, ek, em))
    assert not bad, (name, bad)


SHAPES = [("A", 2, 1), ("A", 2, 5), ("A", 2, 31), ("A", 2, 200), ("B", 2, 257), ("B", 1, 1500)]


@pytest.mark.parametrize("sched,B,L", SHAPES)
@pytest.mark.parametrize("D", [48, 64, 96])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_parity(fmt, D, sched, B, L):
    """Measured on the MI355X: e_kernel / e_model is at most 2.00, reached exactly at L = 1, where dv is
    one more rounding of the model's sum."""
    segs, ratios = SCHEDS[sched]
    q, k, v, dm = _inputs(1000 * D + L, B, L, D, DTYPES[fmt])
    _parity("%s D%d %s B%d L%d" % (fmt, D, sched, B, L), q, k, v, dm, segs, ratios)


@pytest.mark.parametrize("sched,B,L", [("A", 2, 200), ("B", 2, 257)])
@pytest.mark.parametrize("D", [48, 64])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_parity_prescaled(fmt, D, sched, B, L):
    """q_log2_prescaled = 1: q' = q D^-0.5 log2 e as the Q projection would write it; the reference is
    differentiated with respect to q'."""
    segs, ratios = SCHEDS[sched]
    q, k, v, dm = _inputs(2000 * D + L, B, L, D, DTYPES[fmt], q_scale=D ** -0.5 * host.LOG2E)
    _parity("%s prescaled D%d %s L%d" % (fmt, D, sched, L), q, k, v, dm, segs, ratios, prescaled=True)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_parity_sharp_softmax(fmt):
    """q, k scaled x4: sharp, near one-hot P."""
    segs, ratios = SCHEDS["B"]
    q, k, v, dm = _inputs(7, 2, 257, 48, DTYPES[fmt], qk_scale=4.0)
    _parity("%s sharp D48 B L257" % fmt, q, k, v, dm, segs, ratios)


# ----------------------------------------------------------------------------------------------
# exact cases
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_zero_dmerged_gives_zero(fmt):
    q, k, v, dm = _inputs(12, 2, 200, 64, DTYPES[fmt])
    for g in _kernel(q, k, v, torch.zeros_like(dm), *SCHEDS["A"]):
        assert (g == 0).all()


@pytest.mark.parametrize("sched,L,D", [("A", 200, 96), ("B", 1500, 48)])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_two_runs_are_bit_identical(fmt, sched, L, D):
    q, k, v, dm = _inputs(14, 1, L, D, DTYPES[fmt])
    a, b = _kernel(q, k, v, dm, *SCHEDS[sched]), _kernel(q, k, v, dm, *SCHEDS[sched])
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("sched,L", [("A", 200), ("B", 257)])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_guard_rows_survive(fmt, sched, L):
    """A sentinel row before and after the fused dqkv is not written, and every row between them is."""
    q, k, v, dm = _inputs(15, 2, L, 48, DTYPES[fmt])
    grads, guards, _ = _kernel(q, k, v, dm, *SCHEDS[sched], full=True)
    assert (guards.float() == SENTINEL).all()
    for g in grads:
        assert torch.isfinite(g.float()).all() and (g.float() != SENTINEL).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_batches_and_heads_do_not_mix(fmt):
    """dmerged non-zero in one (batch, head)'s columns only: every other (batch, head) slice is exactly 0."""
    q, k, v, dm = _inputs(13, 2, 200, 48, DTYPES[fmt])
    one = torch.zeros_like(dm).view(2, 200, H, 48)
    one[1, :, 5] = dm.view(2, 200, H, 48)[1, :, 5]
    for g in _kernel(q, k, v, one.view(2, 200, H * 48), *SCHEDS["A"]):
        assert (g[1, :, 5] != 0).any()
        g = g.clone()
        g[1, :, 5] = 0
        assert (g == 0).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_segments_do_not_mix(fmt):
    """One branch (64, 1) at L = 200, dmerged non-zero on segment 2's tokens only: zero gradients elsewhere."""
    q, k, v, dm = _inputs(16, 2, 200, 48, DTYPES[fmt])
    one = torch.zeros_like(dm)
    one[:, 128:192] = dm[:, 128:192]
    for g in _kernel(q, k, v, one, [64], [1]):
        assert (g[:, 128:192] != 0).any()
        g = g.clone()
        g[:, 128:192] = 0
        assert (g == 0).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_uncovered_heads_read_zero(fmt):
    """One branch (64, 2): token p is covered for heads h with h // 8 == (p % 64) % 2 only.  dqkv starts full of a
    sentinel: every uncovered (token, head) must read 0, and no element keeps the sentinel."""
    L = 200
    q, k, v, dm = _inputs(17, 2, L, 48, DTYPES[fmt])
    grads = _kernel(q, k, v, dm, [64], [2])
    p = torch.arange(L)
    covered = (torch.arange(H)[None, :] // 8) == ((p % 64) % 2)[:, None]          # [L, H]
    for g in grads:
        g = g.float()
        assert (g != SENTINEL).all()
        assert (g[:, ~covered] == 0).all()
        assert (g[:, covered] != 0).any()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_unwritten_forward_rows_are_not_read(fmt):
    """The branch o / lse buffers hold NaN before the forward (schedule A, L = 200: the forward leaves rows
    unwritten): a backward that read such a row would return a NaN."""
    q, k, v, dm = _inputs(18, 2, 200, 48, DTYPES[fmt])
    for g in _kernel(q, k, v, dm, *SCHEDS["A"], nan_fill=True):
        assert torch.isfinite(g.float()).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_single_token_is_exact(fmt):
    """L = 1: every branch has one key, P = 1, so dv = sum_b round(w_b dmerged) with w_b the merge's weights
    (from the returned LSEs), summed in fp32 and rounded once; dP == delta, so dq == dk == 0."""
    dt = DTYPES[fmt]
    segs, ratios = SCHEDS["A"]
    q, k, v, dm = _inputs(11, 2, 1, 48, dt)
    (dq, dk, dv), _, lses = _kernel(q, k, v, dm, segs, ratios, full=True)
    assert (dq == 0).all() and (dk == 0).all()
    lse = torch.full((len(segs), 2, H), -1e8)
    for b, r in enumerate(ratios):
        hpg = -(-H // r)
        l = lses[b].view(2, H)[:, :hpg]                    # token 0 has phase 0: heads below hpg are covered
        lse[b, :, :hpg] = torch.where(l == 0, torch.full_like(l, -1e8), l)
    w = torch.softmax(lse, 0)                              # [branch, B, H] fp32
    dmh = dm.float().view(2, H, 48)
    want = sum((w[b][..., None] * dmh).to(dt).float() * (w[b][..., None] > 0) for b in range(len(segs))).to(dt)
    assert torch.equal(dv.reshape(2, H, 48).view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_inf_in_dmerged_reaches_every_gradient(fmt):
    q, k, v, dm = _inputs(19, 2, 200, 48, DTYPES[fmt])
    dm[1, 77, 5 * 48 + 3] = float("inf")
    for g in _kernel(q, k, v, dm, *SCHEDS["A"]):
        assert not torch.isfinite(g.float()).all()


# ----------------------------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------------------------
def _module(train=True):
    from gigapath.torchscale.architecture.config import EncoderConfig
    from gigapath.torchscale.component.dilated_attention import DilatedAttention
    import oracle as orc
    g = load_golden("dilated_attention_custom.npz")
    args = EncoderConfig(encoder_embed_dim=768, encoder_attention_heads=16, segment_length=list(g["segs"]),
                         dilated_ratio=list(g["ratios"]), flash_attention=True)
    mod = DilatedAttention(args, 768, 16, self_attention=True, subln=True)
    W = orc.make_weights(seam_host.CFG, seed=0)
    pre = seam_host.PRE + "."
    mod.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in W.items() if k.startswith(pre)})
    mod = mod.to(DEV)
    return (mod.train() if train else mod.eval()), g


@pytest.fixture(scope="module")
def module_ref():
    return seam_host.module_reference()


@pytest.fixture(scope="module")
def module_models():
    return {fmt: host.module_model(dt) for fmt, dt in DTYPES.items()}


def _module_grads(mod, x, gb):
    got = {"dx": x.grad[:, torch.from_numpy(gb["dx_rows"]).to(DEV)]}
    for name in seam_host.GRAD_PARAMS:
        p = mod.get_parameter(name)
        assert p.grad is not None and p.grad.dtype == p.dtype, name
        got["d_" + name] = p.grad
    return {k: t.double().cpu().numpy() for k, t in got.items()}


def _check_module(fmt, y, got, module_ref, model):
    for b in range(y.shape[0]):
        rel, cos, ok = close_enough(y[b], module_ref["y"][b])
        assert ok, (b, rel, cos)
    bad = []
    for name, ref in module_ref.items():
        if name == "y":
            continue
        ref = np.asarray(ref, np.float64)
        rel_k = np.abs(got[name] - ref).max() / np.abs(ref).max()
        rel_m = np.abs(model[name] - ref).max() / np.abs(ref).max()
        cos = (got[name] * ref).sum() / np.sqrt((got[name] ** 2).sum() * (ref ** 2).sum())
        print("dilated_bwd module %s %s: rel_kernel %.3e rel_model %.3e cos %.6f" % (fmt, name, rel_k, rel_m, cos))
        if not (rel_k <= max(2 * rel_m, FP32_RESTATEMENT) and cos >= 0.9995):
            bad.append((name, rel_k, rel_m, cos))
    assert not bad, bad


def test_module_gradients_bf16(module_ref, module_models):
    """Our DilatedAttention in .train() on the golden's x and gy: y against the golden, dx at dx_rows and the six
    listed parameter gradients against the reference's autograd; limit max(2 rel_model, 2e-5), cosine >= 0.9995."""
    mod, g = _module()
    gb = load_golden("dilated_attention_bwd.npz")
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    y = mod(x, x, x)[0]
    assert y.dtype == x.dtype and y.grad_fn is not None
    y.backward(torch.from_numpy(gb["gy"].astype(np.float32)).to(DEV))
    _check_module("bf16", y.detach().cpu().numpy(), _module_grads(mod, x, gb), module_ref, module_models["bf16"])


def test_module_fp16_autocast_with_grad_scaler(module_ref, module_models):
    """Under fp16 autocast with a GradScaler: the unscaled gradients pass the same check, the step moves the
    parameters and leaves the scale; a second step with an Inf in gy is skipped."""
    mod, g = _module()
    gb = load_golden("dilated_attention_bwd.npz")
    gy = torch.from_numpy(gb["gy"].astype(np.float32)).to(DEV)
    opt = torch.optim.SGD(mod.parameters(), lr=1e-2)
    # the fp16 bias gradients are sums over all B L rows of the scaled gy, formed in fp16: a small scale keeps them
    # below 65504 (a GradScaler backs off to such a scale by itself)
    scale0 = 2.0 ** 4
    scaler = torch.amp.GradScaler("cuda", init_scale=scale0, growth_interval=1000)
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    with torch.autocast("cuda", torch.float16):
        y = mod(x, x, x)[0]
    assert y.dtype == torch.float32
    scaler.scale((y * gy).sum()).backward()
    before = [p.detach().clone() for p in mod.parameters()]
    scaler.unscale_(opt)
    x.grad /= scale0
    _check_module("fp16", y.detach().cpu().numpy(), _module_grads(mod, x, gb), module_ref, module_models["fp16"])
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == scale0
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, mod.parameters()))

    opt.zero_grad()
    before = [p.detach().clone() for p in mod.parameters()]
    bad = gy.clone()
    bad[1, 77, 100] = float("inf")
    with torch.autocast("cuda", torch.float16):
        y = mod(x, x, x)[0]
    scaler.scale((y * bad).sum()).backward()
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() < scale0
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, mod.parameters()))


def test_separate_key_and_value_inputs():
    """key is not query: three projections into one [M, 3E] buffer, one gradient per input."""
    mod, g = _module()
    xs = [torch.from_numpy(g["x"]).to(DEV).requires_grad_(True) for _ in range(3)]
    y3 = mod(*xs)[0]
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    y1 = mod(x, x, x)[0]
    # the fused [3E, E] GEMM and three [E, E] GEMMs may tile differently: a few 16-bit roundings apart
    assert ((y3 - y1).abs().max() <= 2.0 ** -6 * y1.abs().max()).item()
    gy = torch.ones_like(y1)
    y3.backward(gy)
    y1.backward(gy)
    total = sum(t.grad for t in xs)
    assert all(t.grad is not None and t.grad.abs().max() > 0 for t in xs)
    assert ((total - x.grad).abs().max() <= 2.0 ** -6 * x.grad.abs().max()).item()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_inference_path_is_unchanged(fmt):
    """Under no_grad, and in .eval() with grad enabled and no input requiring grad, the module takes the
    inference path: nothing is recorded and the bits are those of a no_grad call; .train() under no_grad too."""
    mod, g = _module(train=False)
    x = torch.from_numpy(g["x"]).to(DEV)
    ctx = torch.autocast("cuda", torch.float16, enabled=fmt == "fp16")
    with ctx:
        with torch.no_grad():
            y0 = mod(x, x, x)[0]
        y1 = mod(x, x, x)[0]
        mod.train()
        with torch.no_grad():
            y2 = mod(x, x, x)[0]
        y3 = mod(x, x, x)[0]
    assert y0.grad_fn is None and y1.grad_fn is None and y2.grad_fn is None and y3.grad_fn is not None
    assert torch.equal(y0, y1) and torch.equal(y0, y2)
    rel, cos, ok = close_enough(y3[0].detach().cpu().numpy(), y0[0].cpu().numpy())
    assert ok, (rel, cos)


def test_training_with_dropout_still_raises():
    mod, g = _module()
    mod.dropout = 0.1
    x = torch.from_numpy(g["x"]).to(DEV)
    with pytest.raises(RuntimeError, match="dropout"):
        mod(x, x, x)
