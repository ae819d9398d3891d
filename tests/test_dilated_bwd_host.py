"""The fused dilated attention backward (gp_dilated_attn_bwd), CPU side (no GPU): the entry points reject bad
arguments on the host, and a torch restatement of the attention core -- DilatedAttention.forward between the
projections and inner_attn_ln (dilated_attention.py:133-211) -- is pinned to the reference's own autograd golden.

dilated_core is the reference the GPU tests (tests/test_gpu_dilated_bwd.py) differentiate; module_model is the CPU
rounding model of the module's differentiable path (the restatement plus that path's 16-bit roundings).
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as orc
from conftest import load_golden
from test_attn_bwd_host import (FAKE, GRAD_PARAMS, PRE, attn_fp32, attn_rounding_model, module_reference,
                                module_weights)

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
SCHED_A = ([32, 60, 90, 120, 1000], [1, 2, 4, 8, 16])      # the golden's: s % r != 0 with nseg > 1
SCHED_B = ([256, 512, 1024, 2048, 4096], [1, 2, 4, 8, 16])


# ----------------------------------------------------------------------------------------------
# the core: q, k, v [B, L, H, D] -> merged [B, L, H*D]
# ----------------------------------------------------------------------------------------------
def dilated_core(q, k, v, segs, ratios, seam, softmax_scale=None):
    """Literal gathers with zero pads, the seam per branch, the scatter and the LSE merge with the weights
    computed under no_grad (dilated_attention.py:119-124): dilated_attention_seam without its projections and
    LayerNorm.  seam(q, k, v, softmax_scale) -> (out [B', m, H, D], lse [B', H, m])."""
    B, L, H, D = q.shape
    dev = q.device
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

        o, lse = seam(gather(q), gather(k), gather(v), softmax_scale)
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
    return out.reshape(B, L, H * D)


def _rnd(t, dt):
    """Round to dt, stay fp32; autograd rounds the gradient the same way on its way back."""
    return t.to(dt).float() if dt is not None else t


def module_via_core(x, W, segs, ratios, H, seam, dt=None, eps=1e-5):
    """lin -> dilated_core -> layer_norm -> lin.  dt = None: the fp32 restatement.  dt = a 16-bit dtype: the
    rounding model of DilatedAttention's differentiable path -- x, the projection weights and biases (the Q scale
    D^-0.5 log2 e folded in fp32 first, so the seam sees log2-domain logits: softmax_scale = ln 2), the projected
    q | k | v, the merged rows, the LayerNorm output and the out-proj output are rounded to dt."""
    B, L, E = x.shape
    D = E // H
    fold = dt is not None and D in (48, 64)
    qs = (D ** -0.5) * LOG2E if fold else 1.0

    def lin(t, name, scale=1.0):
        w, b = W["%s.%s.weight" % (PRE, name)], W["%s.%s.bias" % (PRE, name)]
        return _rnd(F.linear(t, _rnd(w * scale, dt), _rnd(b * scale, dt)), dt)

    xr = _rnd(x, dt)
    q, k, v = lin(xr, "q_proj", qs), lin(xr, "k_proj"), lin(xr, "v_proj")
    merged = dilated_core(q.view(B, L, H, D), k.view(B, L, H, D), v.view(B, L, H, D), segs, ratios, seam,
                          LN2 if fold else None)
    merged = _rnd(merged, dt)
    attn = F.layer_norm(merged, (E,), W[PRE + ".inner_attn_ln.weight"], W[PRE + ".inner_attn_ln.bias"], eps)
    return lin(_rnd(attn, dt), "out_proj")


def module_backward_core(seam, dt=None):
    """module_via_core on the golden's x and gy (CPU): y and the gradients the golden lists, float64 numpy."""
    g = load_golden("dilated_attention_custom.npz")
    gb = load_golden("dilated_attention_bwd.npz")
    W = module_weights("cpu")
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    y = module_via_core(x, W, [int(s) for s in g["segs"]], [int(r) for r in g["ratios"]], 16, seam, dt)
    y.backward(torch.from_numpy(gb["gy"].astype(np.float32)))
    got = {"y": y.detach(), "dx": x.grad[:, torch.from_numpy(gb["dx_rows"])]}
    for name in GRAD_PARAMS:
        got["d_" + name] = W["%s.%s" % (PRE, name)].grad
    return {k: t.double().numpy() for k, t in got.items()}


def module_model(dt):
    """The CPU rounding model of the module's differentiable path in dt (see module_via_core)."""
    return module_backward_core(attn_rounding_model(dt), dt)


# ----------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from test_abi_and_api import _lib_path
    _lib_path()
    from gigapath import _hip
    return _hip.load_library()


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _tab(n, val=FAKE):
    return (ctypes.c_void_p * n)(*([val] * n))


def _call(lib, D=48, fmt=0, q=FAKE, dq=FAKE, dmerged=FAKE, ws=FAKE, ws_bytes=1 << 40, pre=0, segs=SCHED_A[0],
          ratios=SCHED_A[1], nbranch=None, o_in="tab", lse_in="tab", row_stride=None, d_row_stride=None, H=16, L=200):
    n = len(segs) if nbranch is None else nbranch
    o = _tab(8) if o_in == "tab" else o_in
    l = _tab(8) if lse_in == "tab" else lse_in
    rs = 3 * H * D if row_stride is None else row_stride
    ds = 3 * H * D if d_row_stride is None else d_row_stride
    segs, ratios = list(segs) + [1] * 8, list(ratios) + [1] * 8
    return lib.gp_dilated_attn_bwd(q, FAKE, FAKE, rs, 2, L, H, D, _i32(segs), _i32(ratios), n, o, l, dmerged, 0.0, pre,
                                   dq, FAKE, FAKE, ds, ws, ws_bytes, fmt, None)


def test_symbols_are_exported_under_abi_13(lib):
    from gigapath import _hip
    assert lib.gp_abi_version() == 13 == _hip.ABI_VERSION
    for name in ("gp_dilated_attn_bwd", "gp_dilated_attn_bwd_workspace_bytes"):
        assert name in _hip.SIGNATURES
        assert getattr(lib, name) is not None


def test_argument_errors_are_rejected_on_the_host(lib):
    err = lib.gp_last_error_string
    assert _call(lib, D=40) == -1 and b"head dim 40" in err()
    assert _call(lib, fmt=7) == -1 and b"bad fmt 7" in err()
    assert _call(lib, fmt=2) == -1 and b"bad fmt 2" in err()                      # GP_FMT_F16_VBF16
    assert _call(lib, D=96, pre=1) == -1 and b"q_log2_prescaled" in err()
    assert _call(lib, q=None) == -1 and b"null pointer (q)" in err()
    assert _call(lib, dq=None) == -1 and b"null pointer (dq)" in err()
    assert _call(lib, dmerged=None) == -1 and b"null pointer (dmerged)" in err()
    assert _call(lib, q=FAKE + 2) == -1 and b"misaligned pointer (q)" in err()
    assert _call(lib, dq=FAKE + 8) == -1 and b"misaligned pointer (dq)" in err()
    assert _call(lib, o_in=None) == -1 and b"null pointer (o_in)" in err()
    assert _call(lib, lse_in=None) == -1 and b"null pointer (lse_in)" in err()
    assert _call(lib, o_in=_tab(8, None)) == -1 and b"null pointer (o_in / lse_in [0])" in err()
    assert _call(lib, lse_in=_tab(8, FAKE + 2)) == -1 and b"misaligned pointer (o_in / lse_in [0])" in err()
    assert _call(lib, nbranch=0) == -1 and b"nbranch must be 1..8" in err()
    assert _call(lib, nbranch=9) == -1 and b"nbranch must be 1..8" in err()
    assert _call(lib, ratios=[1, 2, 0, 8, 16]) == -1 and b"branch 2: bad seg_len 90 / ratio 0" in err()
    assert _call(lib, ratios=[1, -2, 4, 8, 16]) == -1 and b"ratio -2" in err()
    assert _call(lib, segs=[32, 60, 90, 0, 1000]) == -1 and b"branch 3: bad seg_len 0" in err()
    need = lib.gp_dilated_attn_bwd_workspace_bytes(2, 200, 16, 48, _i32(SCHED_A[0]), _i32(SCHED_A[1]), 5)
    assert need >= 3 * 2 * 200 * 768 * 4
    assert _call(lib, ws_bytes=need - 1) == -1 and b"workspace too small" in err()
    assert _call(lib, ws=None) == -1 and b"workspace too small" in err()
    assert _call(lib, ws=FAKE + 4, ws_bytes=need) == -1 and b"misaligned workspace" in err()
    assert _call(lib, row_stride=760) == -1 and b"row_stride 760 below H*D = 768" in err()
    assert _call(lib, d_row_stride=760) == -1 and b"d_row_stride 760 below H*D = 768" in err()
    assert _call(lib, L=0) == -1 and b"bad sizes" in err()


def test_workspace_is_monotone_in_L(lib):
    for segs, ratios in (SCHED_A, SCHED_B, ([64], [2])):
        n = len(segs)
        Ls = [1, 2, 5, 31, 32, 33, 200, 257, 1500, 4096, 4097, 70001, 70002]
        sizes = [lib.gp_dilated_attn_bwd_workspace_bytes(2, L, 16, 48, _i32(segs), _i32(ratios), n) for L in Ls]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert all(s >= 3 * 2 * L * 768 * 4 for s, L in zip(sizes, Ls))
    a, r = _i32(SCHED_A[0]), _i32(SCHED_A[1])
    f = lib.gp_dilated_attn_bwd_workspace_bytes
    assert f(2, 200, 16, 40, a, r, 5) == 0
    assert f(0, 200, 16, 48, a, r, 5) == 0 and f(2, 0, 16, 48, a, r, 5) == 0
    assert f(2, 200, 16, 48, a, r, 0) == 0 and f(2, 200, 16, 48, a, r, 9) == 0
    assert f(2, 200, 16, 48, a, _i32([1, 2, 0, 8, 16]), 5) == 0
    assert f(2, 200, 16, 48, None, r, 5) == 0
    assert f(1 << 20, 1 << 20, 16, 48, a, r, 5) == 0


def test_core_restatement_matches_reference_gradients():
    """lin -> dilated_core -> layer_norm -> lin with the fp32 attention at the seam: y, dx at dx_rows and every
    listed parameter gradient within 2e-5 max|ref| of the reference's own autograd golden.  That ties the GPU
    tests' reference (dilated_core) to the reference project."""
    got = module_backward_core(attn_fp32)
    for name, ref in module_reference().items():
        np.testing.assert_allclose(got[name], ref, rtol=0, atol=2e-5 * np.abs(ref).max(), err_msg=name)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_module_model_is_close_to_the_reference(dt):
    """The module's rounding model is the restatement plus 16-bit roundings: close to, and not equal to, the
    reference (a model that dropped a gradient would sit at rel = 1)."""
    got = module_model(dt)
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    for name, ref in module_reference().items():
        rel = np.abs(got[name] - ref).max() / np.abs(ref).max()
        assert rel <= 16 * eps, (name, rel)
