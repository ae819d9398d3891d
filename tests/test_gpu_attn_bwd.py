"""gp_seg_attn_bwd and the autograd flash_attn_func seam on the MI355X (run with -m gpu).

Error measure: e(G) = max|G - G_ref| / max|G_ref| for G in {dq, dk, dv}, G_ref the fp32 CPU autograd of
softmax(c q k^T) v on the same 16-bit-rounded q, k, v and 16-bit dout.  Tolerance: e_kernel(G) <= 2 e_model(G),
e_model from the CPU rounding model of the kernel (test_attn_bwd_host._RoundingModel: O, P, dS and the results
rounded to the format, everything else fp32).  The kernel has the model's rounding points, carries the shipped
forward's own error in o and lse (of the order of the model's rounding of P) and sums in another order: two
independent error sources of equal size add to at most 2x.
"""
import numpy as np
import pytest
import torch

import test_attn_bwd_host as host

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 16
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# one value below, at and above every tile edge in both directions: the issue's lengths plus the kernel's own
# edges (16-row MFMA sub-tiles, 32-row wave chunks, 64-row LDS tiles, 128 rows per workgroup)
FP32_RESTATEMENT = 2e-5
LENGTHS = (31, 63, 64, 65, 127, 128, 129, 257, 517)


def _hip():
    from gigapath import _hip as h
    h.load_library()
    return h


def _inputs(seed, B, L, D, dt, qk_scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    q, k, v, do = (torch.from_numpy(rng.standard_normal((B, L, H, D)).astype(np.float32)) for _ in range(4))
    return (q * qk_scale).to(dt), (k * qk_scale).to(dt), v.to(dt), do.to(dt)


def _kernel(q, k, v, do, guard=False):
    """forward + backward through the C ABI; returns (dq, dk, dv) on the CPU (and the guard rows)."""
    h = _hip()
    B, L, _, D = q.shape
    qd, kd, vd, dod = (t.to(DEV).contiguous() for t in (q, k, v, do))
    o = torch.empty_like(qd)
    lse = torch.empty(B, H, L, dtype=torch.float32, device=DEV)
    h.seg_attn_fwd(qd, kd, vd, o, lse)
    row = H * D
    bufs = [torch.full(((B * L + 2) * row,), -1024.0, dtype=q.dtype, device=DEV) for _ in range(3)]
    outs = [b[row:-row].view(B, L, H, D) for b in bufs]
    h.seg_attn_bwd(qd, kd, vd, o, lse, dod, outs[0], outs[1], outs[2])
    torch.cuda.synchronize()
    grads = tuple(t.cpu() for t in outs)
    if guard:
        return grads, [torch.cat([b[:row], b[-row:]]).cpu() for b in bufs]
    return grads


def _cpu_grads(seam, q, k, v, do):
    ql, kl, vl = (t.float().requires_grad_(True) for t in (q, k, v))
    seam(ql, kl, vl)[0].backward(do.float())
    return ql.grad, kl.grad, vl.grad


def _err(g, ref):
    return ((g.float() - ref).abs().max() / ref.abs().max()).item()


def _parity(name, q, k, v, do):
    dt = q.dtype
    ref = _cpu_grads(host.attn_fp32, q, k, v, do)
    model = _cpu_grads(host.attn_rounding_model(dt), q, k, v, do)
    got = _kernel(q, k, v, do)
    for nm, g, m, r in zip(("dq", "dk", "dv"), got, model, ref):
        assert torch.isfinite(g.float()).all(), (name, nm)
        ek, em = _err(g, r), _err(m, r)
        print("attn_bwd parity %s %s: e_kernel %.3e e_model %.3e ratio %.2f" % (name, nm, ek, em, ek / em))
        assert ek <= 2 * em, (name, nm, ek, em)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("D", [48, 64, 96])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_parity(fmt, D, L):
    q, k, v, do = _inputs(1000 * D + L, 2, L, D, DTYPES[fmt])
    _parity("%s D%d L%d" % (fmt, D, L), q, k, v, do)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_parity_sharp_softmax(fmt):
    """q, k scaled x4: sharp, near one-hot P."""
    q, k, v, do = _inputs(7, 2, 257, 48, DTYPES[fmt], qk_scale=4.0)
    _parity("%s sharp D48 L257" % fmt, q, k, v, do)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_single_key_is_exact(fmt):
    """L = 1: P = 1, so dv == dout bit for bit, and dP == delta, so dq == dk == 0."""
    q, k, v, do = _inputs(11, 2, 1, 48, DTYPES[fmt])
    dq, dk, dv = _kernel(q, k, v, do)
    assert torch.equal(dv.view(torch.int16), do.view(torch.int16))
    assert (dq == 0).all() and (dk == 0).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_zero_dout_gives_zero(fmt):
    q, k, v, do = _inputs(12, 2, 129, 64, DTYPES[fmt])
    for g in _kernel(q, k, v, torch.zeros_like(do)):
        assert (g == 0).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_heads_do_not_mix(fmt):
    """dout non-zero for one (batch, head) only: every other (batch, head) slice of dq, dk, dv is exactly 0."""
    q, k, v, do = _inputs(13, 2, 129, 48, DTYPES[fmt])
    one = torch.zeros_like(do)
    one[1, :, 5] = do[1, :, 5]
    for g in _kernel(q, k, v, one):
        assert (g[1, :, 5] != 0).any()
        g = g.clone()
        g[1, :, 5] = 0
        assert (g == 0).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_is_bitwise_reproducible(fmt):
    q, k, v, do = _inputs(14, 2, 517, 96, DTYPES[fmt])
    a, b = _kernel(q, k, v, do), _kernel(q, k, v, do)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("L", [65, 517])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd_guard_rows_survive(fmt, L):
    """A sentinel row on each side of dq, dk and dv is not written."""
    q, k, v, do = _inputs(15, 2, L, 48, DTYPES[fmt])
    grads, guards = _kernel(q, k, v, do, guard=True)
    for g in guards:
        assert (g.float() == -1024.0).all()
    for g in grads:
        assert torch.isfinite(g.float()).all() and (g.float() != -1024.0).any()


# ----------------------------------------------------------------------------------------------
# the autograd seam
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_seam_backward_fills_grads_in_the_input_dtype(dt):
    from gigapath.torchscale.component.flash_attention import flash_attn_func
    cdt = torch.float16 if dt == torch.float16 else torch.bfloat16
    q, k, v, do = _inputs(21, 2, 65, 48, cdt)
    leaves = [t.to(dt).to(DEV).requires_grad_(True) for t in (q, k, v)]
    out, lse = flash_attn_func(*leaves)
    assert out.dtype == dt and out.grad_fn is not None and not lse.requires_grad
    out.backward(do.to(dt).to(DEV))
    ref = _cpu_grads(host.attn_fp32, q, k, v, do)
    model = _cpu_grads(host.attn_rounding_model(cdt), q, k, v, do)
    for leaf, m, r in zip(leaves, model, ref):
        assert leaf.grad is not None and leaf.grad.dtype == dt and leaf.grad.shape == leaf.shape
        assert _err(leaf.grad.cpu(), r) <= 2 * _err(m, r)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_seam_without_grad_is_todays_path(dt):
    """Under no_grad (and for inputs that do not require grad) out and lse are bit-identical to a direct
    seg_attn_fwd call, and nothing is recorded."""
    from gigapath.torchscale.component.flash_attention import flash_attn_func
    h = _hip()
    q, k, v, _ = _inputs(22, 2, 129, 48, dt)
    qd, kd, vd = (t.to(DEV) for t in (q, k, v))
    o = torch.empty_like(qd)
    lse = torch.empty(2, H, 129, dtype=torch.float32, device=DEV)
    h.seg_attn_fwd(qd, kd, vd, o, lse)
    leaves = [t.clone().requires_grad_(True) for t in (qd, kd, vd)]
    with torch.no_grad():
        o1, l1 = flash_attn_func(*leaves)
    o2, l2 = flash_attn_func(qd, kd, vd)
    o3, l3 = flash_attn_func(*leaves)
    for oo, ll in ((o1, l1), (o2, l2), (o3, l3)):
        assert torch.equal(oo.view(torch.int16), o.view(torch.int16)) and torch.equal(ll, lse)
    assert o1.grad_fn is None and o2.grad_fn is None and o3.grad_fn is not None


def test_seam_fp16_autocast_with_grad_scaler():
    """fp16 autocast with a GradScaler-scaled loss: finite grads at scale 2^16 on unit-variance inputs, and an
    Inf planted in dout reaches dq, dk and dv as non-finite (so the scaler skips the step)."""
    from gigapath.torchscale.component.flash_attention import flash_attn_func
    q, k, v, _ = _inputs(23, 2, 129, 48, torch.float32)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    for plant in (False, True):
        leaves = [t.to(DEV).requires_grad_(True) for t in (q, k, v)]
        with torch.autocast("cuda", torch.float16):
            out, _ = flash_attn_func(*(t.half() for t in leaves))   # a Linear's output under autocast is fp16
            assert out.dtype == torch.float16
            if plant:
                def poison(g):
                    g = g.clone()
                    g[1, 7, 3, 5] = float("inf")
                    return g
                out.register_hook(poison)
            loss = out.float().square().mean()
        scaler.scale(loss).backward()
        for leaf in leaves:
            assert leaf.grad.dtype == torch.float32
            finite = torch.isfinite(leaf.grad).all().item()
            assert finite != plant
            if not plant:
                assert leaf.grad.abs().max().item() > 0


# ----------------------------------------------------------------------------------------------
# module level: the reference's DilatedAttention around the seam
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def module_ref():
    return host.module_reference()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_module_gradients_match_reference(fmt, module_ref):
    """DilatedAttention (restated in test_attn_bwd_host, pinned there to the reference) with flash_attn_func at
    the seam: dx and the listed parameter gradients against the reference's fp32 autograd.  close_enough's two
    figures (max|d| / max|ref| and the cosine); the limit on the first is twice what the same
    restatement gives on the CPU with the rounding model at the seam."""
    from gigapath.torchscale.component.flash_attention import flash_attn_func
    dt = DTYPES[fmt]

    def gpu_seam(q, k, v):
        out, lse = flash_attn_func(q.to(dt), k.to(dt), v.to(dt))
        return out.float(), lse

    def cpu_seam(q, k, v):
        return host.attn_rounding_model(dt)(q, k, v)

    got = host.module_backward(gpu_seam, DEV)
    model = host.module_backward(cpu_seam, "cpu")
    bad = []
    for name, ref in module_ref.items():
        if name == "y":
            continue
        ref = np.asarray(ref, np.float64)
        rel_k = np.abs(got[name] - ref).max() / np.abs(ref).max()
        rel_m = np.abs(model[name] - ref).max() / np.abs(ref).max()
        cos = (got[name] * ref).sum() / np.sqrt((got[name] ** 2).sum() * (ref ** 2).sum())
        print("attn_bwd module %s %s: rel_kernel %.3e rel_model %.3e cos %.6f" % (fmt, name, rel_k, rel_m, cos))
        # FP32_RESTATEMENT: a gradient that does not pass through the seam (out_proj.bias = sum of gy,
        # inner_attn_ln.bias) has rel_model = 0 on the CPU and differs on the GPU by the order of torch's fp32
        # sums only; for those the limit is the bound at which the fp32 restatement itself is pinned to the
        # reference (test_attn_bwd_host, test_oracle_golden.py)
        if not (rel_k <= max(2 * rel_m, FP32_RESTATEMENT) and cos >= 0.9995):
            bad.append((name, rel_k, rel_m, cos))
    assert not bad, bad
