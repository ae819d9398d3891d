"""Attention backward at the flash_attn_func seam, CPU side (no GPU): the ABI 13 entry points reject bad
arguments on the host, and a torch restatement of DilatedAttention.forward with a pluggable seam function
reproduces the reference's y, dx and parameter gradients (tests/golden/dilated_attention_bwd.npz).

The restatement is what tests/test_gpu_attn_bwd.py runs with the MI355X seam; this file pins it -- and the
no-grad branch weights (dilated_attention.py:119-124) in particular -- to the reference.  It also holds the CPU
seams the GPU tests compare against: the fp32 attention and the rounding model of gp_seg_attn_bwd.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as orc
from conftest import load_golden

CFG = orc.arch_config("gigapath_slide_enc12l768d")
PRE = "encoder.layers.0.self_attn"
GRAD_PARAMS = ("q_proj.bias", "k_proj.bias", "v_proj.bias", "out_proj.bias", "inner_attn_ln.weight",
               "inner_attn_ln.bias")
FAKE = 0x1000   # a non-null, 16-byte aligned address that is never dereferenced


# ----------------------------------------------------------------------------------------------
# seams: f(q, k, v) -> (out [B, L, H, D], lse [B, H, L]) on [B, L, H, D] inputs
# ----------------------------------------------------------------------------------------------
def attn_fp32(q, k, v, softmax_scale=None):
    """softmax(c q k^T) v in the inputs' precision, differentiable by autograd."""
    c = q.shape[-1] ** -0.5 if softmax_scale is None else softmax_scale
    s = torch.einsum("blhd,bmhd->bhlm", q, k) * c
    lse = torch.logsumexp(s, -1)
    out = torch.einsum("bhlm,bmhd->blhd", torch.exp(s - lse[..., None]), v)
    return out, lse


def _rnd(t, dt):
    return t.to(dt).float()


class _RoundingModel(torch.autograd.Function):
    """gp_seg_attn_bwd's math in fp32 with its rounding points: q, k, v, o and dout in the 16-bit format,
    P and dS rounded before the products that consume them, results rounded once."""

    @staticmethod
    def forward(ctx, q, k, v, dt, c):
        q, k, v = _rnd(q, dt), _rnd(k, dt), _rnd(v, dt)
        s = torch.einsum("blhd,bmhd->bhlm", q, k) * c
        lse = torch.logsumexp(s, -1)
        out = _rnd(torch.einsum("bhlm,bmhd->blhd", torch.exp(s - lse[..., None]), v), dt)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.dt, ctx.c = dt, c
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse = ctx.saved_tensors
        dt, c = ctx.dt, ctx.c
        do = _rnd(dout, dt)
        delta = (do * out).sum(-1).permute(0, 2, 1)                        # [B, H, L]
        p = torch.exp(torch.einsum("blhd,bmhd->bhlm", q, k) * c - lse[..., None])
        dv = torch.einsum("bhlm,blhd->bmhd", _rnd(p, dt), do)
        dp = torch.einsum("blhd,bmhd->bhlm", do, v)
        ds = _rnd(p * (dp - delta[..., None]), dt)
        dq = c * torch.einsum("bhlm,bmhd->blhd", ds, k)
        dk = c * torch.einsum("bhlm,blhd->bmhd", ds, q)
        return _rnd(dq, dt), _rnd(dk, dt), _rnd(dv, dt), None, None


def attn_rounding_model(dt):
    def seam(q, k, v, softmax_scale=None):
        c = q.shape[-1] ** -0.5 if softmax_scale is None else softmax_scale
        return _RoundingModel.apply(q, k, v, dt, c)
    return seam


# ----------------------------------------------------------------------------------------------
# DilatedAttention.forward (dilated_attention.py:133-217) around a seam, differentiable by autograd
# ----------------------------------------------------------------------------------------------
def dilated_attention_seam(x, W, segs, ratios, H, seam, eps=1e-5):
    """x [B, L, E]; W: name -> tensor (orc.make_weights keys under PRE, on x's device).  The branch weights
    are computed from the LSEs under no_grad, as scattering does; orc.merge_branches differentiates through
    them and is not used."""
    B, L, E = x.shape
    D = E // H
    dev = x.device

    def lin(t, name):
        return F.linear(t, W["%s.%s.weight" % (PRE, name)], W["%s.%s.bias" % (PRE, name)])

    q, k, v = (lin(x, n).view(B, L, H, D) for n in ("q_proj", "k_proj", "v_proj"))
    hcol = torch.arange(H, device=dev)
    dense_o, dense_l = [], []
    for sl, r in zip(segs, ratios):
        tok = torch.from_numpy(orc.gather_index(L, sl, r, H)).to(dev)          # [nseg, H, m], -1 = zero pad
        nseg, _, m = tok.shape
        tok = torch.where(tok < 0, torch.full_like(tok, L), tok)
        hidx = hcol.view(1, H, 1).expand_as(tok)

        def gather(t):                                                         # -> [B * nseg, m, H, D]
            tp = torch.cat([t, t.new_zeros(B, 1, H, D)], dim=1)
            return tp[:, tok, hidx].permute(0, 1, 3, 2, 4).reshape(B * nseg, m, H, D)

        o, lse = seam(gather(q), gather(k), gather(v))
        o = o.view(B, nseg, m, H, D)
        lse = lse.view(B, nseg, H, m)
        n_idx, i_idx = (torch.from_numpy(a).to(dev) for a in orc.scatter_index(L, sl, r, H))   # [L, H]
        cov = n_idx >= 0
        nn_, ii = n_idx.clamp(min=0), i_idx.clamp(min=0)
        hh = hcol.view(1, H).expand(L, H)
        dense_o.append(o[:, nn_, ii, hh] * cov[None, :, :, None].to(o.dtype))  # [B, L, H, D]
        with torch.no_grad():
            ld = lse.float()[:, nn_, hh, ii]
            ld = torch.where(cov[None] & (ld != 0), ld, torch.full_like(ld, -1e8))
        dense_l.append(ld)
    with torch.no_grad():
        mx = torch.stack(dense_l, 0).max(0)[0]
        w = [torch.exp(l - mx) for l in dense_l]
        wsum = torch.stack(w, 0).sum(0)
        w = [t / wsum for t in w]
    out = 0
    for od, wi in zip(dense_o, w):
        out = out + od * wi[..., None].to(od.dtype)
    attn = out.reshape(B, L, E)
    attn = F.layer_norm(attn, (E,), W[PRE + ".inner_attn_ln.weight"], W[PRE + ".inner_attn_ln.bias"], eps)
    return lin(attn, "out_proj")


def module_weights(device="cpu"):
    """The self-attention weights of layer 0 as leaf tensors that collect gradients."""
    return {k: torch.from_numpy(v).to(device).requires_grad_(True)
            for k, v in orc.make_weights(CFG, seed=0).items() if k.startswith(PRE + ".")}


def module_backward(seam, device="cpu"):
    """Runs the restatement on the golden's x and gy; returns y and the gradients the golden lists
    (dx at the golden's dx_rows), as float64 numpy arrays."""
    g = load_golden("dilated_attention_custom.npz")
    gb = load_golden("dilated_attention_bwd.npz")
    W = module_weights(device)
    x = torch.from_numpy(g["x"]).to(device).requires_grad_(True)
    y = dilated_attention_seam(x, W, [int(s) for s in g["segs"]], [int(r) for r in g["ratios"]], 16, seam)
    y.backward(torch.from_numpy(gb["gy"].astype(np.float32)).to(device))
    got = {"y": y.detach(), "dx": x.grad[:, torch.from_numpy(gb["dx_rows"]).to(device)]}
    for name in GRAD_PARAMS:
        got["d_" + name] = W["%s.%s" % (PRE, name)].grad
    return {k: t.double().cpu().numpy() for k, t in got.items()}


def module_reference():
    g = load_golden("dilated_attention_custom.npz")
    gb = load_golden("dilated_attention_bwd.npz")
    ref = {"y": g["y"], "dx": gb["dx"]}
    ref.update({"d_" + n: gb["d_" + n] for n in GRAD_PARAMS})
    return ref


# ----------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from test_abi_and_api import _lib_path
    _lib_path()
    from gigapath import _hip
    return _hip.load_library()


def _bwd(lib, D=48, fmt=0, dq=FAKE, ws=FAKE, ws_bytes=1 << 30, seqlen=100, q=FAKE):
    return lib.gp_seg_attn_bwd(q, FAKE, FAKE, FAKE, FAKE, FAKE, 2, seqlen, 16, D, 0.0, dq, FAKE, FAKE, ws, ws_bytes,
                               fmt, None)


def test_abi_version_is_13(lib):
    from gigapath import _hip
    assert lib.gp_abi_version() == 13 == _hip.ABI_VERSION
    assert "gp_seg_attn_bwd" in _hip.SIGNATURES and "gp_seg_attn_bwd_workspace_bytes" in _hip.SIGNATURES


def test_bwd_argument_errors_are_rejected_on_the_host(lib):
    assert _bwd(lib, D=40) == -1 and b"head dim 40" in lib.gp_last_error_string()
    assert _bwd(lib, fmt=7) == -1 and b"bad fmt 7" in lib.gp_last_error_string()
    assert _bwd(lib, dq=None) == -1 and b"null pointer (dq)" in lib.gp_last_error_string()
    need = lib.gp_seg_attn_bwd_workspace_bytes(2, 100, 16, 48)
    assert need >= 2 * 16 * 100 * 4
    assert _bwd(lib, ws_bytes=need - 1) == -1 and b"workspace too small" in lib.gp_last_error_string()
    assert _bwd(lib, ws=None) == -1 and b"workspace too small" in lib.gp_last_error_string()
    assert _bwd(lib, ws=FAKE + 4) == -1 and b"misaligned workspace" in lib.gp_last_error_string()
    assert _bwd(lib, q=FAKE + 2) == -1 and b"misaligned pointer (q)" in lib.gp_last_error_string()
    assert _bwd(lib, seqlen=0) == -1 and b"bad seqlen" in lib.gp_last_error_string()
    assert _bwd(lib, seqlen=1 << 31) == -1 and b"bad seqlen" in lib.gp_last_error_string()


def test_bwd_workspace_is_monotone(lib):
    shapes = [(1, 1, 1), (1, 1, 16), (1, 31, 16), (2, 31, 16), (2, 517, 16), (3, 8192, 16), (69, 1024, 16),
              (13, 2896, 16), (1, 8751, 16), (64, 8751, 16)]
    shapes.sort(key=lambda s: s[0] * s[1] * s[2])
    sizes = [lib.gp_seg_attn_bwd_workspace_bytes(nb, sl, H, 48) for nb, sl, H in shapes]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s >= nb * sl * H * 4 for s, (nb, sl, H) in zip(sizes, shapes))
    assert sizes[0] > 0 and sizes[-1] > sizes[0]
    assert lib.gp_seg_attn_bwd_workspace_bytes(1, 100, 16, 40) == 0          # bad shape


def test_restatement_matches_reference_gradients():
    """fp32 CPU attention at the seam: y, dx and the parameter gradients within 2e-5 max|ref| of the reference's
    own autograd (the bound test_oracle_golden.py uses for the same module's forward)."""
    got = module_backward(attn_fp32)
    for name, ref in module_reference().items():
        np.testing.assert_allclose(got[name], ref, rtol=0, atol=2e-5 * np.abs(ref).max(), err_msg=name)


def test_restatement_would_catch_a_differentiated_lse():
    """Letting the gradient flow through the branch weights (what orc.merge_branches would do) moves dx past the
    bound above: the golden does pin the no-grad LSE."""
    g = load_golden("dilated_attention_custom.npz")
    W = {k: torch.from_numpy(v) for k, v in orc.make_weights(CFG, seed=0).items()}
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    y = orc.dilated_attention(x, W, PRE, [int(s) for s in g["segs"]], [int(r) for r in g["ratios"]], 16)
    gb = load_golden("dilated_attention_bwd.npz")
    y.backward(torch.from_numpy(gb["gy"].astype(np.float32)))
    d = np.abs(x.grad.numpy()[:, gb["dx_rows"]] - gb["dx"]).max()
    assert d > 2e-5 * np.abs(gb["dx"]).max(), d


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_rounding_model_is_close_to_fp32(dt):
    """The rounding model is the fp32 math plus 16-bit roundings: a few format epsilons from fp32 autograd."""
    rng = np.random.Generator(np.random.PCG64(3))
    q, k, v, do = (torch.from_numpy(rng.standard_normal((1, 65, 2, 48)).astype(np.float32)).to(dt).float()
                   for _ in range(4))
    grads = []
    for seam in (attn_fp32, attn_rounding_model(dt)):
        ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
        seam(ql, kl, vl)[0].backward(do)
        grads.append((ql.grad, kl.grad, vl.grad))
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    for a, b in zip(*grads):
        e = ((a - b).abs().max() / a.abs().max()).item()
        assert 0 < e <= 8 * eps, e
