"""gp_linear_wgrad on the MI355X (run with -m gpu): dW = dY^T X and db = sum_rows dY in fp32 against fp64 on the
same 16-bit operands, with guards around every buffer the kernel writes or reads.

Bound, per element: |out - ref| <= 1.2 (2^-24 |ref| + M 2^-24 mag) + 1e-7 with mag = |dY|^T |X| (sum |dY| for db) --
one fp32 output rounding plus fp32 accumulation over the M rows (test_gpu_gemm_plans.py's form)."""
import pytest
import torch

from gigapath import _hip

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# S = 1 and the 64-row step edges; S = 2 with a ragged last chunk (320 + 280 rows) and that M +- 1; the two tile
# counts; the arch shapes once each (2304 x 768: S = 3, 320 + 320 + 137 rows; 768 x 3072: S = 2, 320 + 200)
SHAPES = [(1, 256, 256), (63, 256, 256), (64, 256, 256), (65, 256, 256), (1, 768, 768), (65, 768, 768),
          (599, 256, 256), (600, 256, 256), (601, 256, 256), (600, 768, 768), (601, 768, 768), (777, 2304, 768),
          (520, 768, 3072)]
GUARD = 7.0


def _operands(M, N, K, dtype, strided=False, seed=0):
    """dY [M, N] and X [M, K] as views whose buffers continue with three NaN rows (and, strided, sit inside wider
    rows: dY the middle third of [M, 3N], X with ldx = K + 64)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ybuf = torch.randn(M + 3, 3 * N if strided else N, generator=g, device="cuda").to(dtype)
    xbuf = torch.randn(M + 3, K + 64 if strided else K, generator=g, device="cuda").to(dtype)
    ybuf[M:] = float("nan")
    xbuf[M:] = float("nan")
    return (ybuf[:M, N:2 * N] if strided else ybuf[:M]), xbuf[:M, :K]


def _call(dy, x, with_db=True, ldw=None):
    """One guarded call: dW / db NaN-prefilled inside GUARD-filled buffers (two sentinel rows, the row padding),
    the workspace exactly the required bytes, NaN-filled, with a guard tail.  Returns (dW, db) after checking that
    nothing outside them changed."""
    M, N = dy.shape
    K = x.shape[1]
    ldw = ldw or K
    wbuf = torch.full((N + 2, ldw), GUARD, device="cuda")
    dw = wbuf[:N, :K]
    dw.fill_(float("nan"))
    bbuf = torch.full((N + 8,), GUARD, device="cuda")
    bbuf[:N] = float("nan")
    need = int(_hip.load_library().gp_linear_wgrad_workspace_bytes(M, N, K))
    wsbuf = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    wsbuf[need:] = 0x5A
    _hip.linear_wgrad(dy, x, dw, bbuf[:N] if with_db else None, wsbuf[:need] if need else None)
    torch.cuda.synchronize()
    assert bool((wbuf[N:] == GUARD).all()) and bool((wbuf[:N, K:] == GUARD).all()), "dW guard overwritten"
    assert bool((bbuf[N:] == GUARD).all()), "db guard overwritten"
    assert bool((wsbuf[need:] == 0x5A).all()), "workspace guard overwritten"
    if not with_db:
        assert bool(torch.isnan(bbuf[:N]).all()), "db written without being asked for"
    return dw.clone(), bbuf[:N].clone()


def _worst_ratio(out, ref, mag, M):
    bound = 1.2 * (2.0 ** -24 * ref.abs() + M * 2.0 ** -24 * mag) + 1e-7
    return float(((out.double() - ref).abs() / bound).max())


def _check(dy, x, dw, db, tag):
    M = dy.shape[0]
    y64, x64 = dy.double(), x.double()
    rw = _worst_ratio(dw, y64.t() @ x64, y64.abs().t() @ x64.abs(), M)
    rb = _worst_ratio(db, y64.sum(0), y64.abs().sum(0), M)
    print("wgrad %s: worst |err| / bound  dW %.3f  db %.3f" % (tag, rw, rb))
    assert rw <= 1.0 and rb <= 1.0, (tag, rw, rb)   # (a NaN left in dW / db fails here too)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_wgrad_matches_fp64(shape, dtype):
    M, N, K = shape
    dy, x = _operands(M, N, K, dtype)
    dw, db = _call(dy, x)
    _check(dy, x, dw, db, "%s %s" % (shape, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_wgrad_strided_operands(dtype):
    M, N, K = 600, 256, 256
    dy, x = _operands(M, N, K, dtype, strided=True)
    dw, db = _call(dy, x, ldw=K + 12)
    _check(dy, x, dw, db, "strided %s" % dtype)


@pytest.mark.parametrize("M", [65, 600], ids=["S1", "S2"])
def test_wgrad_reproducible_and_db_optional(M):
    dy, x = _operands(M, 768, 768, torch.bfloat16, seed=1)
    dw, db = _call(dy, x)
    dw2, db2 = _call(dy, x)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    dw3, _ = _call(dy, x, with_db=False)
    assert torch.equal(dw, dw3)


@pytest.mark.parametrize("M", [65, 600], ids=["S1", "S2"])
def test_wgrad_inf_stays_in_its_row(M):
    """One +Inf in dY[m, n] (a GradScaler overflow) reaches row n of dW and db[n] and nothing else."""
    dy, x = _operands(M, 256, 512, torch.float16, seed=2)
    dw, db = _call(dy, x)
    m, n = M - 2, 37
    dy[m, n] = float("inf")
    dwi, dbi = _call(dy, x)
    assert not bool(torch.isfinite(dwi[n]).any()) and not bool(torch.isfinite(dbi[n]))
    keep = torch.arange(256, device="cuda") != n
    assert torch.equal(dwi[keep], dw[keep]) and torch.equal(dbi[keep], db[keep])


def test_wgrad_rejects_bad_n():
    dy, x = _operands(64, 320, 256, torch.bfloat16)
    dw = torch.empty(320, 256, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 256"):
        _hip.linear_wgrad(dy, x, dw)
