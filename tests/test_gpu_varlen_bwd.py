"""gp_dilated_attn_bwd_varlen on the MI355X (run with -m gpu): the backward of packed slides against the per-slide
kernels that tests/test_gpu_dilated_bwd.py pins to the fp64 CPU gradient.

The packed launch reaches the same tile loops through another addressing, so the acceptance is bit equality: a
slide's rows of dq / dk / dv equal gp_dilated_attn_bwd (B = 1) on that slide's rows of the same qkv and dmerged.
H = 16, D = 48, pre-scaled q, bf16 and fp16.  The packs:
  B     SCHED_B, [1500, 257, 1, 700, 130]: m = 256 crosses a 128-row tile, a 94-row tail tile, a one-token slide
  A     SCHED_A, [200, 5, 31, 1, 333]: s % r != 0 with several segments -> zero-padded queries
  arch  the 12L768d schedule, [1025, 17, 2897]: several segments of branch 0, a slide under 32 tokens
Each pack's packed run and per-slide runs are computed once per format and shared by the tests.
"""
import functools

import numpy as np
import pytest
import torch

from test_dilated_bwd_host import LOG2E, SCHED_A, SCHED_B

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, D, E = 16, 48, 768
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SCHED_ARCH = ([1024, 5792, 32768, 185363, 1048576], [1, 2, 4, 8, 16])
PACKS = {"B": (SCHED_B, [1500, 257, 1, 700, 130]), "A": (SCHED_A, [200, 5, 31, 1, 333]),
         "arch": (SCHED_ARCH, [1025, 17, 2897])}
SENTINEL = -1024.0


def _hip():
    from gigapath import _hip as h
    h.load_library()
    return h


def _offsets(Ls):
    return np.concatenate([[0], np.cumsum(Ls)]).tolist()


@functools.lru_cache(maxsize=None)
def _inputs(pack, fmt):
    """(qkv [T, 3E] with q pre-scaled by D^-0.5 log2 e, dmerged [T, E]) on the device, in the format."""
    T = sum(PACKS[pack][1])
    rng = np.random.Generator(np.random.PCG64(4800 + T))
    qkv = torch.from_numpy(rng.standard_normal((T, 3 * E)).astype(np.float32))
    qkv[:, :E] *= D ** -0.5 * LOG2E
    dm = torch.from_numpy(rng.standard_normal((T, E)).astype(np.float32))
    return qkv.to(DTYPES[fmt]).to(DEV), dm.to(DTYPES[fmt]).to(DEV)


def _packed(qkv, dm, Ls, segs, ratios):
    """The varlen forward and gp_dilated_attn_bwd_varlen through the bindings -> (dqkv [T, 3E], the sentinel guard
    rows before and after it, the forward's packed outs, lses)."""
    from gigapath import runtime
    h = _hip()
    T = sum(Ls)
    vs = runtime.VarlenScratch(torch.device(DEV), Ls, H, D, segs, ratios, qkv)
    for t in vs.outs + vs.lses:
        t.zero_()
    h.dilated_attn_fwd_varlen(vs.plan, True)
    buf = torch.full((T + 2, 3 * E), SENTINEL, dtype=qkv.dtype, device=DEV)
    dqkv = buf[1:-1]
    plan = h.VarlenBwdPlan(Ls, H, D, segs, ratios).bind(qkv, vs.outs, vs.lses)
    h.dilated_attn_bwd_varlen(plan, dm, dqkv, dqkv[:, E:], dqkv[:, 2 * E:], 3 * E)
    torch.cuda.synchronize()
    return dqkv.clone(), torch.cat([buf[0], buf[-1]]), vs.outs, vs.lses


def _slide(qkv, dm, t0, L, segs, ratios):
    """gp_dilated_attn_fwd + gp_dilated_attn_bwd (B = 1) on rows [t0, t0 + L) -> (dqkv [L, 3E], outs, lses)."""
    from gigapath import runtime
    h = _hip()
    rows = qkv[t0:t0 + L]
    sc = runtime.AttentionScratch(torch.device(DEV), 1, L, H, D, segs, ratios, qkv.dtype)
    for t in sc.outs + sc.lses:
        t.zero_()
    h.dilated_attn_fwd(rows, rows[:, E:], rows[:, 2 * E:], 3 * E, 1, L, H, D, segs, ratios, sc.outs, sc.lses, 0.0, True)
    dqkv = torch.full((L, 3 * E), SENTINEL, dtype=qkv.dtype, device=DEV)
    h.dilated_attn_bwd(rows, rows[:, E:], rows[:, 2 * E:], 3 * E, 1, L, H, D, segs, ratios, sc.outs, sc.lses,
                       dm[t0:t0 + L], dqkv, dqkv[:, E:], dqkv[:, 2 * E:], 3 * E, 0.0, True)
    torch.cuda.synchronize()
    return dqkv, sc.outs, sc.lses


@functools.lru_cache(maxsize=None)
def _baseline(pack, fmt):
    """The packed run of the pack's inputs, computed once and left unchanged."""
    (segs, ratios), Ls = PACKS[pack]
    qkv, dm = _inputs(pack, fmt)
    return _packed(qkv, dm, Ls, segs, ratios)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("pack", list(PACKS))
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bit_equal_per_slide(fmt, pack):
    """The forward's o / lse regions first (as test_varlen_attention_and_merge_bit_exact_per_slide), then every
    slide's rows of dq | dk | dv."""
    (segs, ratios), Ls = PACKS[pack]
    qkv, dm = _inputs(pack, fmt)
    dqkv, guards, outs, lses = _baseline(pack, fmt)
    off = _offsets(Ls)
    o_off, l_off = [0] * len(segs), [0] * len(segs)
    for i, L in enumerate(Ls):
        want, s_outs, s_lses = _slide(qkv, dm, off[i], L, segs, ratios)
        for b in range(len(segs)):
            no, nl = s_outs[b].numel(), s_lses[b].numel()
            assert torch.equal(outs[b][o_off[b]:o_off[b] + no], s_outs[b]), ("forward o", L, b)
            assert torch.equal(lses[b][l_off[b]:l_off[b] + nl], s_lses[b]), ("forward lse", L, b)
            o_off[b] += no
            l_off[b] += nl
        got = dqkv[off[i]:off[i + 1]]
        assert torch.isfinite(got.float()).all(), (L,)
        for j, nm in enumerate(("dq", "dk", "dv")):
            a, w = got[:, j * E:(j + 1) * E], want[:, j * E:(j + 1) * E]
            ndiff = int((_bits(a.contiguous()) != _bits(w.contiguous())).sum())
            print("varlen bwd %s %s slide L=%d %s: %d elements differ, max|ref| %.3e"
                  % (fmt, pack, L, nm, ndiff, w.float().abs().max().item()))
            assert torch.equal(_bits(a.contiguous()), _bits(w.contiguous())), (nm, L, ndiff)
    assert (guards == SENTINEL).all()


@pytest.mark.parametrize("pack", ["B", "A"])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_neighbours_do_not_leak(fmt, pack):
    """Every other slide's qkv and dmerged rows NaN: the untouched slide keeps its bits (each slide in turn); the
    guard rows around dqkv survive; a second call gives the same bits."""
    (segs, ratios), Ls = PACKS[pack]
    qkv, dm = _inputs(pack, fmt)
    base, _, _, _ = _baseline(pack, fmt)
    off = _offsets(Ls)
    for i, L in enumerate(Ls):
        q2 = torch.full_like(qkv, float("nan"))
        d2 = torch.full_like(dm, float("nan"))
        q2[off[i]:off[i + 1]] = qkv[off[i]:off[i + 1]]
        d2[off[i]:off[i + 1]] = dm[off[i]:off[i + 1]]
        got, guards, _, _ = _packed(q2, d2, Ls, segs, ratios)
        assert torch.equal(_bits(got[off[i]:off[i + 1]]), _bits(base[off[i]:off[i + 1]])), (L,)
        assert (guards == SENTINEL).all()
    again, guards, _, _ = _packed(qkv, dm, Ls, segs, ratios)
    assert torch.equal(_bits(again), _bits(base))
    assert (guards == SENTINEL).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_zero_dmerged_gives_zero(fmt):
    (segs, ratios), Ls = PACKS["A"]
    qkv, dm = _inputs("A", fmt)
    got, guards, _, _ = _packed(qkv, torch.zeros_like(dm), Ls, segs, ratios)
    assert (got == 0).all() and (guards == SENTINEL).all()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_inf_stays_in_its_slide(fmt):
    """A +Inf in one slide's dmerged: that slide's dq, dk and dv are non-finite, every other slide's bits stay."""
    (segs, ratios), Ls = PACKS["B"]
    qkv, dm = _inputs("B", fmt)
    base, _, _, _ = _baseline("B", fmt)
    off = _offsets(Ls)
    hit = 1                                               # the 257-token slide
    d2 = dm.clone()
    d2[off[hit] + 100, 5 * D + 7] = float("inf")
    got, guards, _, _ = _packed(qkv, d2, Ls, segs, ratios)
    for i, L in enumerate(Ls):
        rows = slice(off[i], off[i + 1])
        if i == hit:
            for j, nm in enumerate(("dq", "dk", "dv")):
                assert not torch.isfinite(got[rows, j * E:(j + 1) * E].float()).all(), nm
        else:
            assert torch.equal(_bits(got[rows]), _bits(base[rows])), (L,)
    assert (guards == SENTINEL).all()
