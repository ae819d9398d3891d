"""The persistent GEMM's tile plan at its edges, at kernel level (run with -m gpu on an MI355X): every branch
of make_plan / launch (csrc/gp_gemm_impl.h) and the kernels behind it -- one full round, two, a one-tile
split tail, the largest split tail and the first unsplit one above it, the shortest K-split sequences (K =
1024 / 1536: 4 / 6 K-tiles per part), a QKV-shaped launch that really splits (the reduce kernel's bf16 V third
and its LN fold), and the 1024- / 1536-wide archs' projections.

Row counts come from tests/gemm_plan.py for the CU count of this device, and every test first asserts,
through gp_gemm_workspace_bytes and that restatement of the planner, that the plan it names is the one the
library runs here.  The figures in the comments are those of 256 CUs.

Buffers: outputs are NaN-prefilled and followed by 256 sentinel rows that must stay untouched; the workspace
is exactly the planned size, NaN-prefilled (a partial never written would reach the output), and followed by
a 4 KiB guard pattern that must stay intact.

Plain outputs are held to the per-element bound test_ffn_fc1_gelu_and_statistics asserts of fc1's
pre-activation, against a . w^T + b in fp64 on the same 16-bit operands:
    |out - ref| <= 1.2 (ulp |ref| + K 2^-24 mag) + 1e-7,  ulp = 2^-7 (bf16) / 2^-10 (fp16),  mag = |a| . |w|^T + |b|
(one output rounding, <= ulp/2, plus the fp32 accumulation bound).  Each test prints its worst |d| / bound.
"""
import pytest
import torch

import gemm_plan
import test_gpu_gemm as tg
from test_gpu_gemm import ACTS, DEV, _elem_ratio, _hip, _rand, _ref64, _ulp

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT = 256          # sentinel rows after row M: a whole tile's worth past a partial last row block
NAN = float("nan")


def _workspace(nbytes):
    """(whole buffer, the nbytes-long workspace view): NaN partials, then the guard pattern."""
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    buf[:nbytes].view(torch.float32).fill_(NAN)
    buf[nbytes:] = 0xA5
    return buf, buf[:nbytes]


def _guard_intact(buf):
    return bool((buf[-GUARD:] == 0xA5).all())


def _out(M, N, dtype):
    base = torch.full((M + SENT, N), NAN, dtype=dtype, device=DEV)
    base[M:] = 7.0
    return base


def _claim(h, M, N, K, S, rem, tiles=None):
    """Assert that an M x N x K launch with a workspace runs the named plan on this device; return it."""
    G = tg._cus()
    p = gemm_plan.plan(M, N, K, G)
    assert h.gemm_workspace_bytes(M, N, K) == p.ws_bytes, (M, N, K, p)
    assert (p.S, p.rem) == (S, rem) and p.n_dp + p.rem == gemm_plan.tiles_of(M, N), (M, N, K, p)
    assert (p.ws_bytes == 0) == (S == 1)
    if tiles is not None:
        assert gemm_plan.tiles_of(M, N) == tiles
    return p


def _linear_both_plans(h, act, M, N, K, p, seed, v_bf16=False):
    """gp_linear with the planned workspace (plan p) and with none (all data-parallel): both within the
    per-element bound, nothing written past row M or past the workspace.  Returns the operands, the reference
    and the with-workspace output for further checks."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = _rand((M, K), g).to(act)
    w = _rand((N, K), g, K ** -0.5).to(act)
    b = _rand((N,), g, 0.1)
    ref, mag = _ref64(a, w, b)
    keep = None
    for use_ws in (True, False):
        buf, ws = _workspace(p.ws_bytes if use_ws else 0)
        base = _out(M, N, act)
        h.linear(a, w, b, base[:M], ws if use_ws else None, v_bf16=v_bf16)
        torch.cuda.synchronize()
        assert (base[M:] == 7.0).all(), "rows past M written"
        assert _guard_intact(buf), "workspace guard overwritten"
        if use_ws and p.ws_bytes:
            assert torch.isfinite(ws.view(torch.float32)).all()      # every planned partial was written
        out = base[:M]
        if v_bf16:
            v0 = 2 * N // 3
            r = max(_elem_ratio(out[:, :v0], ref[:, :v0], mag[:, :v0], _ulp(act), K),
                    _elem_ratio(out[:, v0:].view(torch.bfloat16), ref[:, v0:], mag[:, v0:], 2.0 ** -7, K))
        else:
            r = _elem_ratio(out, ref, mag, _ulp(act), K)
        print("gp_linear %s M=%d N=%d K=%d S=%d rem=%d ws=%s: max |d| / bound = %.3f"
              % (str(act)[6:], M, N, K, p.S if use_ws else 1, p.rem if use_ws else 0, use_ws, r))
        assert r <= 1.0, (use_ws, r)
        if use_ws:
            keep = out
    return a, w, b, ref, keep


# ---------------------------------------------------------------------------------------------------
# 1 / 2.  Plan edges at N = 256 (tiles = row blocks), the tail tile the partial one (113 rows).  On 256 CUs:
#   one_round   65,393 rows: 256 tiles = G, one tile per workgroup, no second round
#   rem1        65,649 rows: 257 tiles, one tail tile split S ways (S workgroups of the last round at work)
#   max_rem     98,161 rows (S = 2: 384 tiles, 128 split) / 81,777 (S = 4: 320 tiles, 64 split): every workgroup
#               in the tail
#   max_rem+1   256 rows more: the first remainder the plan leaves unsplit (no workspace)
#   two_rounds  130,929 rows: 512 tiles = 2 G, the tile-to-tile hand-off with no tail
EDGES = ["one_round", "rem1", "max_rem", "max_rem+1", "two_rounds"]


def _edge(edge, K, G):
    """(M, S, rem, tiles) of a named plan edge for N = 256 on G CUs."""
    S, top = gemm_plan.split_factor(K), gemm_plan.max_split_rem(K, G)
    if edge == "one_round":
        return (G - 1) * 256 + 113, 1, 0, G
    if edge == "rem1":
        return gemm_plan.rows_for(256, K, G, 1), S, 1, G + 1
    if edge == "max_rem":
        return gemm_plan.rows_for(256, K, G, top), S, top, G + top
    if edge == "max_rem+1":
        return gemm_plan.rows_for(256, K, G, top + 1), 1, 0, G + top + 1
    assert edge == "two_rounds"
    return gemm_plan.rows_for(256, K, G, 0), 1, 0, 2 * G


def _plan_edge(act, K, edge):
    h = _hip()
    M, S, rem, tiles = _edge(edge, K, tg._cus())
    assert M % 256 == 113
    p = _claim(h, M, 256, K, S, rem, tiles)
    _linear_both_plans(h, act, M, 256, K, p, seed=M + K)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("edge", EDGES)
def test_plan_edges_product_k(act, K, edge):
    """The 768-wide arch's K: S = 2 (K = 768, 6 K-tiles per part) and S = 4 (K = 3072, 12 per part)."""
    _plan_edge(act, K, edge)


@pytest.mark.parametrize("act,K,edge",
                         [(torch.bfloat16, K, e) for K in (1024, 1536) for e in EDGES] +
                         [(torch.float16, K, e) for K in (1024, 1536) for e in ("rem1", "max_rem")],
                         ids=lambda v: str(v)[6:] if isinstance(v, torch.dtype) else str(v))
def test_plan_edges_shortest_split(act, K, edge):
    """K = 1024 and 1536, S = 4: 4 and 6 K-tiles per part -- 4 is the shortest sequence the 8-phase loop runs."""
    _plan_edge(act, K, edge)


# ---------------------------------------------------------------------------------------------------
# 3.  A QKV-shaped launch whose plan splits (N = 2304, K = 768, S = 2).  "smallest": the smallest multi-round
# split plan (7,281 rows: 261 tiles, 5 split); "keyrows": the remainder of the 70k slide's key-row QKV (14,807
# rows: 522 tiles, 10 split) at the smallest row count that has it (14,705).  Nine tiles per row panel and n_dp
# = 256 / 512: the first tail panel is part data-parallel, part split.
def _qkv_rows(h, which):
    G = tg._cus()
    if which == "smallest":
        M, rem = gemm_plan.smallest_split_rows(2304, 768, G)
    else:
        rem = 10
        M = gemm_plan.rows_for(2304, 768, G, rem)
    return M, _claim(h, M, 2304, 768, 2, rem)


@pytest.mark.parametrize("fmt", ["bf16", "fp16", "fp16_vbf16"])
@pytest.mark.parametrize("which", ["smallest", "keyrows"])
def test_qkv_split_tail(fmt, which):
    """gp_linear: the per-element bound in every format; for an fp16 QKV with the bf16 V third (the reduce
    kernel's vcol0 branch) the assertions of test_fp16_qkv_with_bf16_v_third on a plan that splits: q / k
    columns bit-equal to the plain fp16 launch, V the bf16 rounding of the same accumulators."""
    h = _hip()
    M, p = _qkv_rows(h, which)
    act = torch.bfloat16 if fmt == "bf16" else torch.float16
    E, N = 768, 2304
    a, w, b, ref, out = _linear_both_plans(h, act, M, N, E, p, seed=M + 31, v_bf16=fmt == "fp16_vbf16")
    if fmt != "fp16_vbf16":
        return
    buf, ws = _workspace(p.ws_bytes)
    plain = _out(M, N, act)
    h.linear(a, w, b, plain[:M], ws)
    torch.cuda.synchronize()
    assert _guard_intact(buf) and (plain[M:] == 7.0).all()
    plain = plain[:M]
    assert torch.equal(out[:, :2 * E], plain[:, :2 * E])
    vb = out[:, 2 * E:].view(torch.bfloat16).float()
    pv = plain[:, 2 * E:].float()
    assert torch.isfinite(vb).all()
    assert tg._rel(vb, ref[:, 2 * E:].float()) <= 1e-2
    assert (vb - pv).abs().max().item() <= 2 ** -8 * pv.abs().max().item()
    # element by element: acc -> fp16 moves it by <= 2^-11 |acc| (2^-25 where subnormal), acc -> bf16 by <= 2^-8
    # |acc|, so the two roundings of one accumulator differ by <= (2^-8 + 2^-11) / (1 - 2^-11) |fp16 value|
    assert ((vb - pv).abs() <= (2.0 ** -8 + 2.0 ** -10) * pv.abs() + 2.0 ** -24).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16", "fp16_vbf16"])
@pytest.mark.parametrize("which", ["smallest", "keyrows"])
def test_qkv_split_tail_ln_fold(fmt, which):
    """gp_linear_ln (the LN-fold epilogue of the reduce kernel) on the same plans, to test_linear_ln_fold's
    criteria; with the bf16 V third, also q / k bit-equal to the plain fp16 launch and V the bf16 rounding of
    the same accumulators."""
    h = _hip()
    M, p = _qkv_rows(h, which)
    act = torch.bfloat16 if fmt == "bf16" else torch.float16
    E, N = 768, 2304
    g = torch.Generator(device=DEV).manual_seed(M + 11)
    x, s, gam, bet, xb, st0 = tg._fold_setup(g, act, M, E, N)
    w = _rand((N, E), g, E ** -0.5).to(act)
    b = _rand((N,), g, 0.1)
    c = (w.double() @ gam.double()).float()
    d = (w.double() @ bet.double() + b.double()).float()
    ln = torch.nn.functional.layer_norm(x, (E,), gam, bet, 1e-5)
    ref = ln.to(act).float() @ w.float().t() + b

    def run(v_bf16):
        st = st0.clone()
        st[E // 256] = NAN
        s_out = torch.full((M,), NAN, device=DEV)
        buf, ws = _workspace(p.ws_bytes)
        base = _out(M, N, act)
        h.linear_ln(xb, w, st, E // 256, c, d, 1e-5, s, s_out, base[:M], ws, v_bf16=v_bf16)
        torch.cuda.synchronize()
        assert (base[M:] == 7.0).all() and _guard_intact(buf)
        assert torch.isfinite(ws.view(torch.float32)).all()
        assert torch.allclose(s_out.double(), x.double().mean(1), rtol=1e-5, atol=1e-5)
        assert torch.allclose(st[E // 256, :, 1].double(),
                              1.0 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5), rtol=1e-4)
        return base[:M]

    out = run(fmt == "fp16_vbf16")
    got = out.float()
    if fmt == "fp16_vbf16":
        got = torch.cat([got[:, :2 * E], out[:, 2 * E:].view(torch.bfloat16).float()], 1)
    assert torch.isfinite(got).all()
    rel = tg._rel(got, ref)
    assert rel <= 1e-2, rel
    cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
    assert cos >= 0.99995, cos
    if fmt == "fp16_vbf16":
        plain = run(False)
        assert torch.equal(out[:, :2 * E], plain[:, :2 * E])
        vb, pv = got[:, 2 * E:], plain[:, 2 * E:].float()
        assert (vb - pv).abs().max().item() <= 2 ** -8 * pv.abs().max().item()
        assert ((vb - pv).abs() <= (2.0 ** -8 + 2.0 ** -10) * pv.abs() + 2.0 ** -24).all()    # as above


# ---------------------------------------------------------------------------------------------------
# The 24L1024d / 12L1536d archs' plain projections (gp_linear): QKV (N = 3E, K = E: the non-temporal-store
# instantiation), out-proj (E, E) and the fc2 shape (N = E, K = 4E = 4096 / 6144), at one row and at the smallest
# multi-round split plan with a partial last row block (S = 4; on 256 CUs QKV 5,489 rows: 264 tiles, 8 split /
# 3,697: 270, 14 split; N = 1024: 16,497 rows, 260 tiles, 4 split; N = 1536: 10,865 rows, 258 tiles, 2 split).
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rows", ["one", "split"])
@pytest.mark.parametrize("E", [1024, 1536])
@pytest.mark.parametrize("shape", ["qkv", "out_proj", "fc2"])
def test_linear_wide_archs(act, rows, E, shape):
    h = _hip()
    N, K = {"qkv": (3 * E, E), "out_proj": (E, E), "fc2": (E, 4 * E)}[shape]
    if rows == "one":
        M, p = 1, _claim(h, 1, N, K, 1, 0, N // 256)
    else:
        M, rem = gemm_plan.smallest_split_rows(N, K, tg._cus())
        p = _claim(h, M, N, K, 4, rem)
        assert M % 256 == 113
    _linear_both_plans(h, act, M, N, K, p, seed=M + N + K)
