"""gp_linear_dgrad on the MI355X (-m gpu): dX = dY W against fp64 on the same 16-bit operands, guards around dX, NaN rows
behind dY.  Bound (test_gpu_gemm._elem_ratio): 1.2 (ulp |ref| + N 2^-24 |dY| |W|) + 1e-7, ulp 2^-7 bf16 / 2^-10 fp16."""
import pytest
import torch

from gigapath import _hip
from test_gpu_gemm import _elem_ratio

pytestmark = pytest.mark.gpu

ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
FMTS = pytest.mark.parametrize("dtype", list(ULP), ids=["bf16", "fp16"])
# (M, N, K): one row, the 256-row tile edge, two row blocks + 1; several k tiles and 12 stages; the arch shapes
SHAPES = [(1, 256, 256), (255, 256, 256), (256, 256, 256), (257, 256, 256), (513, 256, 256), (257, 768, 768),
          (300, 2304, 768), (300, 3072, 768), (300, 768, 3072), (300, 3072, 1024), (300, 1536, 6144),
          (300, 256, 512, "strided")]
GUARD = 7.0


def _operands(M, N, K, dtype, strided=False, seed=0):
    """dY [M, N] before three NaN rows, W [N, K] (strided: dY the middle third of [M, 3N], ldw = K + 64, NaN pads)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ybuf = torch.randn(M + 3, 3 * N if strided else N, generator=g, device="cuda").to(dtype)
    ybuf[M:] = float("nan")
    wbuf = (torch.randn(N, K + 64 if strided else K, generator=g, device="cuda") * 0.05).to(dtype)
    wbuf[:, K:] = float("nan")
    return (ybuf[:M, N:2 * N] if strided else ybuf[:M]), wbuf[:, :K]


def _call(dy, w, ldx=None):
    """One guarded call: dX NaN-prefilled inside a GUARD-filled buffer (two sentinel rows, the row padding)."""
    M, K = dy.shape[0], w.shape[1]
    xbuf = torch.full((M + 2, ldx or K), GUARD, device="cuda").to(dy.dtype)
    dx = xbuf[:M, :K]
    dx.fill_(float("nan"))
    _hip.linear_dgrad(dy, w, dx)
    torch.cuda.synchronize()
    assert bool((xbuf[M:] == GUARD).all()) and bool((xbuf[:M, K:] == GUARD).all()), "dX guard overwritten"
    return dx.clone()


def _check(dy, w, dx, tag):
    y64, w64 = dy.double(), w.double()
    r = _elem_ratio(dx, y64 @ w64, y64.abs() @ w64.abs(), ULP[dy.dtype], dy.shape[1])
    print("dgrad %s: worst |err| / bound %.3f" % (tag, r))
    assert r <= 1.0, (tag, r)   # (a NaN left in dX fails here too)


@FMTS
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dgrad_matches_fp64(shape, dtype):
    strided = len(shape) == 4   # dY the middle third of [M, 3N], ldw = K + 64, ldx = K + 8
    dy, w = _operands(*shape[:3], dtype, strided)
    _check(dy, w, _call(dy, w, shape[2] + 8 if strided else None), "%s %s" % (shape, dtype))


def test_dgrad_reproducible_and_inf_stays_in_its_row():   # (the +Inf: a GradScaler overflow)
    M = 300
    dy, w = _operands(M, 768, 512, torch.float16, seed=2)
    dx = _call(dy, w)
    assert torch.equal(_call(dy, w), dx)
    dy[M - 2, 37] = float("inf")
    dxi = _call(dy, w)
    assert not bool(torch.isfinite(dxi[M - 2]).any())
    keep = torch.arange(M, device="cuda") != M - 2
    assert torch.equal(dxi[keep], dx[keep])


def test_dgrad_rejects_bad_n():
    dy, w = _operands(64, 320, 256, torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of 256"):
        _hip.linear_dgrad(dy, w)
