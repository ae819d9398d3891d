"""The training path's row kernels at the model width, CPU side (no GPU): gp_resid_drop_ln_fwd / _bwd and
gp_dropout_keep_mask exist under ABI 13 and reject bad arguments on the host, the workspace size behaves, the
documented Philox4x32-10 mapping is restated in numpy (pinned to the generator's known-answer vector), and a torch
restatement of the backward's closed form is checked against fp64 autograd.

The reference helpers the GPU tests (tests/test_gpu_rows_train.py) import:
  ref64         fp64 autograd of the forward written with torch ops and an explicit mask, the rounding straight-through
  format_model  today's torch lines (dropout as input * (mask / (1 - p)), drop-path, residual add, F.layer_norm in
                fp32, .to(format)) on the CPU in the format; e_model = rel_err(format_model, ref64)
Shapes: "A" add + LN, "B" add only, "C32" LN of the fp32 stream, "C16" LN of a 16-bit tensor.

Tolerances.  16-bit outputs (a, dy, the 16-bit dx) and, by the project's rule for comparisons with the same count of
roundings, every output of the kernels: e <= 2 e_model.  The fp32 outputs of the torch restatement (r, the fp32 dx,
dln_w, dln_b): e <= 2e-5, the bound test_train_host.py uses for fp32 restatements (sums of <= 1536 fp32 terms).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_attn_bwd_host import FAKE
from test_train_host import FP32_RESTATEMENT, rel_err

COLS = (768, 1024, 1536)
SHAPES = ("A", "B", "C32", "C16")
EPS = 1e-5
OUTPUTS = ("r", "a", "dx", "dy", "dw", "db")


# ----------------------------------------------------------------------------------------------
# the mask: Philox4x32-10 as the header documents it
# ----------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter [n, 4] uint32, key (k0, k1) -> [n, 4] uint32 (Salmon et al., SC'11)."""
    c = [counter[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, 1).astype(np.uint32)


def philox_keep_mask(seed, p, rows, cols):
    """gp_dropout_keep_mask in numpy: key = (low, high word of seed), counter = (low, high word of index >> 2, 0, 0),
    word (index & 3) serves the element, keep = word >= floor(p 2^32), p taken as fp32."""
    n = rows * cols
    assert n % 4 == 0
    q = np.arange(n // 4, dtype=np.uint64)
    ctr = np.zeros((n // 4, 4), dtype=np.uint32)
    ctr[:, 0] = (q & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (q >> np.uint64(32)).astype(np.uint32)
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)
    thr = int(float(np.float32(p)) * 4294967296.0)
    return (words.astype(np.uint64) >= np.uint64(thr)).astype(np.uint8).reshape(rows, cols)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 10."""
    z = philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [int(v) for v in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    m = philox_keep_mask(1234567890123, 0.1, 257, 768)
    n = m.size
    assert abs(m.mean() - 0.9) <= 5 * np.sqrt(0.1 * 0.9 / n)
    assert np.array_equal(m[:5], philox_keep_mask(1234567890123, 0.1, 5, 768))
    assert bool(philox_keep_mask(7, 0.0, 4, 768).all())


# ----------------------------------------------------------------------------------------------
# inputs and the two references
# ----------------------------------------------------------------------------------------------
def rows_inputs(rows, cols, dt, nscale=0, seed=0):
    """x, dr fp32; y (no zeros, |y| in [0.5, 1.5)), da, x16 in dt; ln w, b fp32; s: None (nscale = 0) or nscale
    drop-path factors mask / keep with keep = 0.75, the second entry a dropped path (0) when there are two or more."""
    g = torch.Generator().manual_seed(100003 * seed + 7 * rows + cols + nscale)
    x = torch.randn(rows, cols, generator=g)
    sign = torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0)
    y = (sign * (0.5 + torch.rand(rows, cols, generator=g))).to(dt)
    da = torch.randn(rows, cols, generator=g).to(dt)
    dr = torch.randn(rows, cols, generator=g)
    w = 1.0 + 0.2 * torch.randn(cols, generator=g)
    b = 0.1 * torch.randn(cols, generator=g)
    s = None
    if nscale:
        assert rows % nscale == 0
        s = torch.full((nscale,), 1.0) / 0.75
        if nscale >= 2:
            s[1] = 0.0
    return {"x": x, "x16": x.to(dt), "y": y, "da": da, "dr": dr, "w": w, "b": b, "s": s}


def _row_scale(s, rows, dtype):
    if s is None:
        return torch.ones(rows, 1, dtype=dtype)
    return s.to(dtype).repeat_interleave(rows // s.numel()).view(rows, 1)


def ref64(shape, inp, mask, p, dt, eps=EPS):
    """fp64 autograd of the forward written with torch ops and the explicit keep mask (uint8 [rows, cols] or None for
    p == 0): r = x + s keep y / (1 - p), a = LN(r) w + b, p taken as fp32.  The rounding of a to the format is
    straight-through: it passes the gradient unchanged, and the value compared is the unrounded one (against a rounded
    reference the worst element would be whichever lies nearest a rounding boundary, on either side).  Gradients
    for da at a and dr at r.  Returns the fp64 outputs the shape has, keyed as OUTPUTS."""
    rows, cols = inp["x"].shape
    w = inp["w"].double().requires_grad_(True)
    b = inp["b"].double().requires_grad_(True)
    out, heads, grads = {}, [], []
    if shape in ("A", "B"):
        x = inp["x"].double().requires_grad_(True)
        y = inp["y"].double().requires_grad_(True)
        f = _row_scale(inp["s"], rows, torch.float64) / (1.0 - float(np.float32(p)))
        if mask is not None:
            f = f * mask.double()
        r = x + f * y
        out["r"] = r.detach()
        heads.append(r)
        grads.append(inp["dr"].double())
    else:
        x = (inp["x"] if shape == "C32" else inp["x16"]).double().requires_grad_(True)
        y = None
        r = x
    if shape != "B":
        a = F.layer_norm(r, (cols,), w, b, eps)
        out["a"] = a.detach()
        heads.append(a)
        grads.append(inp["da"].double())
    torch.autograd.backward(heads, grads)
    out["dx"] = x.grad
    if y is not None:
        out["dy"] = y.grad
    if shape != "B":
        out["dw"], out["db"] = w.grad, b.grad
    return out


def format_model(shape, inp, mask, p, dt, eps=EPS):
    """Today's torch lines on the CPU in the format dt: F.dropout's arithmetic with the given mask (input * (mask /
    (1 - p))), drop_path's x * (mask / keep), the fp32 residual add, F.layer_norm in fp32 and .to(dt)."""
    rows, cols = inp["x"].shape
    w = inp["w"].clone().requires_grad_(True)
    b = inp["b"].clone().requires_grad_(True)
    out, heads, grads = {}, [], []
    if shape in ("A", "B"):
        x = inp["x"].clone().requires_grad_(True)
        y = inp["y"].clone().requires_grad_(True)
        t = y.float()
        if mask is not None:
            t = t * (mask.float() / (1.0 - p))
        if inp["s"] is not None:
            t = t * _row_scale(inp["s"], rows, torch.float32)
        r = x + t
        out["r"] = r.detach()
        heads.append(r)
        grads.append(inp["dr"])
    else:
        x = (inp["x"] if shape == "C32" else inp["x16"]).clone().requires_grad_(True)
        y = None
        r = x
    if shape != "B":
        a = F.layer_norm(r.float(), (cols,), w, b, eps).to(dt)
        out["a"] = a.detach()
        heads.append(a)
        grads.append(inp["da"])
    torch.autograd.backward(heads, grads)
    out["dx"] = x.grad
    if y is not None:
        out["dy"] = y.grad
    if shape != "B":
        out["dw"], out["db"] = w.grad, b.grad
    return out


def closed_form(shape, inp, mask, p, dt, eps=EPS):
    """The kernels' arithmetic in torch: fp32 throughout, every 16-bit output rounded once; mean / rstd recomputed
    from the saved LN input."""
    rows, cols = inp["x"].shape
    out = {}
    f = None
    if shape in ("A", "B"):
        inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - np.float32(p))
        f = (_row_scale(inp["s"], rows, torch.float32) * inv).expand(rows, cols)
        if mask is not None:
            f = f * mask.float()
        saved = inp["x"] + f * inp["y"].float()
        out["r"] = saved
    else:
        saved = (inp["x"] if shape == "C32" else inp["x16"]).float()
    dx = inp["dr"].clone() if shape in ("A", "B") else torch.zeros(rows, cols)
    if shape != "B":
        mean = saved.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((saved - mean) ** 2).mean(1, keepdim=True) + eps)
        xhat = (saved - mean) * rstd
        out["a"] = (xhat * inp["w"] + inp["b"]).to(dt)
        d = inp["da"].float()
        dxhat = d * inp["w"]
        dx = dx + rstd * (dxhat - dxhat.sum(1, keepdim=True) / cols - xhat * ((dxhat * xhat).sum(1, keepdim=True) / cols))
        out["dw"], out["db"] = (d * xhat).sum(0), d.sum(0)
    out["dx"] = dx.to(dt) if shape == "C16" else dx
    if f is not None:
        out["dy"] = (f * dx).to(dt)
    return out


def errors(got, r64, model):
    """{output: (e, e_model)} over the outputs present."""
    return {k: (rel_err(got[k].double(), r64[k]), rel_err(model[k].double(), r64[k])) for k in OUTPUTS if k in r64}


def is_16bit(shape, k):
    return k in ("a", "dy") or (k == "dx" and shape == "C16")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols", COLS)
def test_closed_form_matches_fp64_autograd(cols, dt):
    for rows in (1, 5, 257):
        for shape in SHAPES:
            p = 0.1 if shape in ("A", "B") else 0.0
            nscale = 1 if rows == 1 else (rows if rows == 5 else 1)
            inp = rows_inputs(rows, cols, dt, nscale if shape in ("A", "B") else 0)
            g = torch.Generator().manual_seed(rows + cols)
            mask = (torch.rand(rows, cols, generator=g) >= p).to(torch.uint8) if p > 0 else None
            r64, model = ref64(shape, inp, mask, p, dt), format_model(shape, inp, mask, p, dt)
            for k, (e, em) in errors(closed_form(shape, inp, mask, p, dt), r64, model).items():
                print("%s cols %d rows %3d %-3s %-2s e %.3e  e_model %.3e" % (dt, cols, rows, shape, k, e, em))
                if is_16bit(shape, k):
                    assert e <= 2 * em, (shape, rows, k, e, em)
                else:
                    assert e <= FP32_RESTATEMENT, (shape, rows, k, e)


# ----------------------------------------------------------------------------------------------
# host checks of the C ABI
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from test_abi_and_api import _lib_path
    _lib_path()
    from gigapath import _hip
    return _hip.load_library()


G = 1 << 30   # the fake buffers lie 1 GiB apart: no overlap at 8 x 768


def _fwd(lib, x=FAKE, x_is_act=0, y=FAKE + G, s=None, rps=1, p=0.1, seed=5, ln_w=FAKE + 6 * G, ln_b=FAKE + 7 * G,
         r=FAKE + 2 * G, a=FAKE + 3 * G, rows=8, cols=768, fmt=0):
    return lib.gp_resid_drop_ln_fwd(x, x_is_act, y, s, rps, p, seed, ln_w, ln_b, 1e-5, r, a, rows, cols, fmt, None)


def _bwd(lib, da=FAKE, dr=FAKE + G, saved=FAKE + 2 * G, saved_is_act=0, ln_w=FAKE + 6 * G, s=None, rps=1, p=0.1,
         seed=5, dx=FAKE + 3 * G, dy=FAKE + 4 * G, dw=FAKE + 7 * G, db=FAKE + 8 * G, ws=FAKE + 9 * G, ws_bytes=1 << 40,
         rows=8, cols=768, fmt=0):
    return lib.gp_resid_drop_ln_bwd(da, dr, saved, saved_is_act, ln_w, 1e-5, s, rps, p, seed, dx, dy, dw, db, ws,
                                    ws_bytes, rows, cols, fmt, None)


def test_symbols_are_exported_under_abi_13(lib):
    from gigapath import _hip
    assert lib.gp_abi_version() == 13 == _hip.ABI_VERSION
    for name in ("gp_resid_drop_ln_fwd", "gp_resid_drop_ln_bwd", "gp_resid_drop_ln_bwd_workspace_bytes",
                 "gp_dropout_keep_mask"):
        assert name in _hip.SIGNATURES
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_shared_argument_errors_are_rejected_on_the_host(lib, call):
    err = lib.gp_last_error_string
    assert call(lib, fmt=7) == -1 and b"bad fmt 7" in err()
    assert call(lib, fmt=2) == -1 and b"bad fmt 2" in err()                        # GP_FMT_F16_VBF16
    assert call(lib, cols=3072) == -1 and b"cols=3072 unsupported" in err()
    assert call(lib, cols=800) == -1 and b"cols=800 unsupported" in err()
    assert call(lib, rows=-1) == -1 and b"bad rows" in err()
    assert call(lib, rows=1 << 31) == -1 and b"too many rows" in err()
    for p in (1.0, -0.1, 1.5, float("nan")):
        assert call(lib, p=p) == -1 and b"outside [0, 1)" in err(), p
    assert call(lib, s=FAKE + 5 * G, rps=0) == -1 and b"must be positive" in err()
    assert call(lib, s=FAKE + 5 * G, rps=-4) == -1 and b"must be positive" in err()
    assert call(lib, s=FAKE + 5 * G, rps=3) == -1 and b"no multiple of rows_per_scale" in err()
    assert call(lib, ln_w=FAKE + 6 * G + 4) == -1 and b"misaligned" in err()


def test_forward_argument_errors(lib):
    err = lib.gp_last_error_string
    assert _fwd(lib, x=None) == -1 and b"null pointer" in err()
    assert _fwd(lib, y=None, ln_w=None, ln_b=None, a=None, r=None) == -1 and b"neither y nor ln_w" in err()
    assert _fwd(lib, ln_b=None) == -1 and b"all be given or all be null" in err()
    assert _fwd(lib, a=None) == -1 and b"all be given or all be null" in err()
    assert _fwd(lib, r=None) == -1 and b"r must be given with y" in err()
    assert _fwd(lib, y=None) == -1 and b"r must be given with y" in err()              # (C) writes no r
    assert _fwd(lib, x_is_act=1) == -1 and b"16-bit x is for the LayerNorm alone" in err()
    for kw in ({"x": FAKE + 8}, {"y": FAKE + G + 2}, {"r": FAKE + 2 * G + 4}, {"a": FAKE + 3 * G + 8}):
        assert _fwd(lib, **kw) == -1 and b"misaligned" in err(), kw
    assert _fwd(lib, r=FAKE + 4096) == -1 and b"r may alias x only as the same buffer" in err()
    for kw in ({"r": FAKE + G}, {"a": FAKE + G + 4096}, {"a": FAKE}, {"a": FAKE + 2 * G + 64}):
        assert _fwd(lib, **kw) == -1 and b"forbidden aliasing" in err(), kw
    assert _fwd(lib, rows=0, x=None, y=None, r=None, a=None) == 0                     # nothing to do


def test_backward_argument_errors(lib):
    err = lib.gp_last_error_string
    for kw in ({"da": None}, {"saved": None}, {"dx": None}):
        assert _bwd(lib, **kw) == -1 and b"null pointer" in err(), kw
    assert _bwd(lib, ln_w=None, dy=None, da=None, saved=None, dw=None, db=None) == -1 and b"neither ln_w nor dy" in err()
    assert _bwd(lib, ln_w=None) == -1 and b"must be null without ln_w" in err()
    assert _bwd(lib, ln_w=None, da=None, saved=None, dw=None, db=None, dr=None) == -1 and b"null pointer" in err()
    assert _bwd(lib, saved_is_act=1) == -1 and b"16-bit saved input is for the LayerNorm alone" in err()
    assert _bwd(lib, dw=None) == -1 and b"both be given or both be null" in err()
    assert _bwd(lib, db=None) == -1 and b"both be given or both be null" in err()
    for kw in ({"da": FAKE + 2}, {"dr": FAKE + G + 4}, {"saved": FAKE + 2 * G + 8}, {"dx": FAKE + 3 * G + 4},
               {"dy": FAKE + 4 * G + 2}):
        assert _bwd(lib, **kw) == -1 and b"misaligned" in err(), kw
    assert _bwd(lib, dx=FAKE + G + 4096) == -1 and b"dx may alias dr_in only as the same buffer" in err()
    assert _bwd(lib, dy=None, saved_is_act=1, dx=FAKE + G) == -1 and b"16-bit dx cannot alias" in err()
    for kw in ({"dx": FAKE}, {"dx": FAKE + 2 * G}, {"dx": FAKE + 4 * G}, {"dy": FAKE + 64}, {"dy": FAKE + 2 * G},
               {"dy": FAKE + G}):
        assert _bwd(lib, **kw) == -1 and b"forbidden aliasing" in err(), kw
    need = lib.gp_resid_drop_ln_bwd_workspace_bytes(8, 768)
    assert need > 0
    assert _bwd(lib, ws_bytes=need - 1) == -1 and b"workspace too small" in err()
    assert _bwd(lib, ws=None) == -1 and b"workspace too small" in err()
    assert _bwd(lib, ws=FAKE + 9 * G + 4) == -1 and b"misaligned workspace" in err()
    assert _bwd(lib, rows=0, da=None, dr=None, saved=None, dx=None, dy=None) == 0      # nothing to do


def test_keep_mask_argument_errors(lib):
    err = lib.gp_last_error_string
    f = lib.gp_dropout_keep_mask
    assert f(1, 1.0, 4, 768, FAKE, None) == -1 and b"outside [0, 1)" in err()
    assert f(1, -0.5, 4, 768, FAKE, None) == -1 and b"outside [0, 1)" in err()
    assert f(1, 0.1, 4, 770, FAKE, None) == -1 and b"multiple of 4" in err()
    assert f(1, 0.1, 4, 0, FAKE, None) == -1 and b"multiple of 4" in err()
    assert f(1, 0.1, -1, 768, FAKE, None) == -1 and b"bad rows" in err()
    assert f(1, 0.1, 1 << 31, 768, FAKE, None) == -1 and b"too many rows" in err()
    assert f(1, 0.1, 4, 768, None, None) == -1 and b"null pointer" in err()
    assert f(1, 0.1, 4, 768, FAKE + 2, None) == -1 and b"misaligned" in err()
    assert f(1, 0.1, 0, 768, None, None) == 0


def test_workspace_is_monotone_in_rows(lib):
    f = lib.gp_resid_drop_ln_bwd_workspace_bytes
    for cols in COLS:
        rows = [1, 2, 3, 4, 5, 8, 9, 257, 1024, 4096, 4097, 70001, 1 << 20]
        sizes = [f(r, cols) for r in rows]
        assert sizes[0] >= 2 * cols * 4 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] == sizes[-2]                   # the grid is capped: the partials stop growing
        assert all(s % (2 * cols * 4) == 0 for s in sizes)
        assert f(0, cols) == 0 and f(-1, cols) == 0
    assert f(8, 3072) == 0 and f(8, 800) == 0
