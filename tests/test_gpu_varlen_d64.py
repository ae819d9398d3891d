"""Packed (varlen) batches at D = 64 on the MI355X (run with -m gpu): the LDS-DMA fast + fixup attention pair, the
E = 1024 varlen merge and LongNetViT.forward_packed on the 24L1024d arch.  H = 16, D = 64,
q pre-scaled by D^-0.5 log2 e.  The packs (T <= 4k):
  B     SCHED_B, [1500, 257, 1, 700, 130]: m = 256 meets the 256-query block edge, a tail tile, a one-token slide
  A     SCHED_A, [200, 5, 31, 1, 333]: s % r != 0, zero-padded queries and keys
  arch  the registered schedule, [1025, 17, 2897]: several segments, a slide under 32 tokens
Forward bounds against a float64 evaluation (derived): |o - ref| <= 2^-8 (|ref| + max|v|) -- p rounded
to bf16 (2^-9) and o rounded once (2^-9), a factor 2 on both; |lse - ref| <= 2^-8 -- ln(1 + 2^-9) for a sum of rounded
weights, a factor 2.  Measured worst err / bound on the MI355X (B / A / arch): o 0.51 / 0.55 /
0.31, lse 0.0003 / 0.0002 / 0.0004; B with q x 40 (every branch flagged): o 0.55, lse 0.0081.
"""
import functools

import numpy as np
import pytest
import torch

import oracle as orc
from test_dilated_bwd_host import LN2, LOG2E, SCHED_A, SCHED_B
from test_gpu_kernels import _rows_needed

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, D, E = 16, 64, 1024
SCHED_ARCH = ([1024, 5792, 32768, 185363, 1048576], [1, 2, 4, 8, 16])
PACKS = {"B": (SCHED_B, [1500, 257, 1, 700, 130]), "A": (SCHED_A, [200, 5, 31, 1, 333]),
         "arch": (SCHED_ARCH, [1025, 17, 2897])}
REDO = 0x7fc0dead                                          # the fast kernel's lse marker for the fixup pass
BOUND = 2.0 ** -8


def _hip():
    from gigapath import _hip as h
    h.load_library()
    return h


@functools.lru_cache(maxsize=None)
def _inputs(pack, gain=1):
    """qkv [T, 3E] bf16 on the device, q pre-scaled by gain D^-0.5 log2 e."""
    T = sum(PACKS[pack][1])
    rng = np.random.Generator(np.random.PCG64(6400 + T))
    qkv = torch.from_numpy(rng.standard_normal((T, 3 * E)).astype(np.float32))
    qkv[:, :E] *= gain * D ** -0.5 * LOG2E
    return qkv.bfloat16().to(DEV)


def _forward(qkv, pack):
    """gp_dilated_attn_fwd_varlen -> the VarlenScratch (plan, packed outs / lses)."""
    from gigapath import runtime
    vs = runtime.VarlenScratch(torch.device(DEV), PACKS[pack][1], H, D, *PACKS[pack][0], qkv)
    for t in vs.outs + vs.lses:
        t.zero_()
    _hip().dilated_attn_fwd_varlen(vs.plan, True)
    torch.cuda.synchronize()
    return vs


@functools.lru_cache(maxsize=None)
def _baseline(pack, gain=1):
    return _forward(_inputs(pack, gain), pack)


def _regions(pack):
    """Per slide: (token offset, L, [(o_lo, o_hi, lse_lo, lse_hi, geometry)] per branch) of the packed buffers."""
    (segs, ratios), Ls = PACKS[pack]
    oo, lo, t0, res = [0] * len(segs), [0] * len(segs), 0, []
    for L in Ls:
        br = []
        for b, (sl, r) in enumerate(zip(segs, ratios)):
            g = orc.branch_geometry(L, sl, r, H)
            no, nl = g["nseg"] * g["m"] * E, g["nseg"] * H * g["m"]
            br.append((oo[b], oo[b] + no, lo[b], lo[b] + nl, g))
            oo[b] += no
            lo[b] += nl
        res.append((t0, L, br))
        t0 += L
    return res


def _check_forward(pack, gain, need_flags):
    """Every slide's branch o / lse rows the merge reads against float64: gather, scores in log2 units (a zero-pad
    key scores 0 with v = 0), softmax, P.V.  need_flags: every branch must hold a real row whose real-key log2 sum
    lies outside +-100 -- a row the fast kernel has to flag."""
    (segs, ratios), _ = PACKS[pack]
    x = _inputs(pack, gain).double().cpu().numpy()
    vmax = np.abs(x[:, 2 * E:]).max()
    vs = _baseline(pack, gain)
    worst, flagged = [0.0, 0.0], [False] * len(segs)
    for t0, L, br in _regions(pack):
        q, k, v = (x[t0:t0 + L, i * E:(i + 1) * E].reshape(L, H, D) for i in range(3))
        for b, (o0, o1, l0, l1, g) in enumerate(br):
            nseg, m = g["nseg"], g["m"]
            idx = orc.gather_index(L, segs[b], ratios[b], H)                     # [nseg, H, m], -1: zero pad
            o = vs.outs[b][o0:o1].double().cpu().numpy().reshape(nseg, m, H, D)
            lse_t = vs.lses[b][l0:l1]
            assert not (lse_t.view(torch.int32) == REDO).any(), (pack, L, b)
            lse = lse_t.double().cpu().numpy().reshape(nseg, H, m)
            need = np.arange(m)[None, None, :] < _rows_needed(L, segs[b], ratios[b], H)[:, :, None]
            for h in range(H):
                ok = idx[:, h] >= 0                                              # [nseg, m]
                qs, ks, vv = (np.where(ok[..., None], t[np.maximum(idx[:, h], 0), h], 0.0) for t in (q, k, v))
                s = np.einsum("nid,njd->nij", qs, ks)
                mx = s.max(-1, keepdims=True)
                p = np.exp2(s - mx)
                ref_o = np.einsum("nij,njd->nid", p, vv) / p.sum(-1)[..., None]
                ref_l = (mx[..., 0] + np.log2(p.sum(-1))) * LN2
                real = mx[..., 0] + np.log2(np.maximum((p * ok[:, None, :]).sum(-1), 1e-300))
                flagged[b] |= bool((np.abs(real) > 100)[need[:, h] & ok].any())
                eo = np.abs(o[:, :, h] - ref_o) / (BOUND * (np.abs(ref_o) + vmax))
                el = np.abs(lse[:, h] - ref_l) / BOUND
                assert np.isfinite(o[:, :, h][need[:, h]]).all() and np.isfinite(lse[:, h][need[:, h]]).all()
                worst = [max(worst[0], eo[need[:, h]].max(initial=0)), max(worst[1], el[need[:, h]].max(initial=0))]
    print("varlen d64 %s gain %d: worst err / bound  o %.4f  lse %.4f  flagged %s" % (pack, gain, *worst, flagged))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    assert not need_flags or all(flagged), flagged


@pytest.mark.parametrize("pack", list(PACKS))
def test_forward_against_fp64(pack):
    _check_forward(pack, 1, False)


def test_fixup_pass_runs():
    """q scaled by 40 (fixup_9000's factor): rows of every branch leave the no-max range and come back exact."""
    _check_forward("B", 40, True)


def _same(a, b, sl=slice(None)):
    return all(torch.equal(x[sl].view(torch.int16), y[sl].view(torch.int16)) for x, y in zip(a, b))


def test_isolation_and_determinism():
    qkv, base, reg = _inputs("arch"), _baseline("arch"), _regions("arch")
    again = _forward(qkv, "arch")
    assert _same(again.outs, base.outs) and _same(again.lses, base.lses)
    for i, (t0, L, br) in enumerate(reg):
        alone = torch.full_like(qkv, float("nan"))             # every other slide NaN
        alone[t0:t0 + L] = qkv[t0:t0 + L]
        loud = qkv.clone()                                      # this slide's rows flagged and fixed
        loud[t0:t0 + L, :E] *= 40
        va, vl = _forward(alone, "arch"), _forward(loud, "arch")
        for j, (_, _, brj) in enumerate(reg):
            for b, (o0, o1, l0, l1, _) in enumerate(brj):
                for v in ([va] if j == i else [vl]):            # va: slide i kept; vl: every slide but i kept
                    assert _same([v.outs[b]], [base.outs[b]], slice(o0, o1)), (i, j, b)
                    assert _same([v.lses[b].view(torch.int32)], [base.lses[b].view(torch.int32)], slice(l0, l1)), (i, j, b)


@pytest.mark.parametrize("with_ln", [True, False])
@pytest.mark.parametrize("pack", list(PACKS))
def test_varlen_merge_equals_the_per_slide_merge(pack, with_ln):
    """gp_branch_merge_ln_varlen at E = 1024 is gp_branch_merge_ln (B = 1) on each slide's regions, bit for bit."""
    h, vs, (segs, ratios) = _hip(), _baseline(pack), PACKS[pack][0]
    rng = np.random.Generator(np.random.PCG64(7))
    w, b_ = (torch.from_numpy(rng.standard_normal(E).astype(np.float32)).to(DEV) if with_ln else None for _ in "wb")
    T = sum(PACKS[pack][1])
    got, want = (torch.full((T, E), -1024.0, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    h.branch_merge_ln_varlen(vs.plan, w, b_, 1e-5, got)
    for t0, L, br in _regions(pack):
        h.branch_merge_ln([vs.outs[b][o0:o1] for b, (o0, o1, _, _, _) in enumerate(br)],
                          [vs.lses[b][l0:l1] for b, (_, _, l0, l1, _) in enumerate(br)], segs, ratios, 1, L, H, D,
                          w, b_, 1e-5, want[t0:t0 + L])
    torch.cuda.synchronize()
    assert _same([got], [want]) and torch.isfinite(got.float()).all()


@pytest.mark.parametrize("train", [False, True])
def test_forward_packed_on_the_24l1024d_arch(train, monkeypatch):
    """gigapath_slide_enc24l1024d cut to depth 2, slides of 300, 1 and 1100 tiles: eval against the fp32 oracle per
    slide, the packed attention launched once per layer (the inference engine's last layer runs for the CLS rows
    alone, through gp_cls_attn_merge_ln, when runtime.CLS_TAIL is on); under enable_training() the call is the slides
    one at a time through forward(), bit for bit, with no packed launch."""
    from functools import partial
    from gigapath import _hip as hip, runtime, slide_encoder
    from gigapath.torchscale.model import LongNetConfig
    from test_gpu_model import check_vectors
    from test_gpu_train_packed import _slides
    cfg = dict(orc.arch_config("gigapath_slide_enc24l1024d"), depth=2)
    monkeypatch.setitem(LongNetConfig.CONFIGS, "LongNet_2_layers_1024_dim", LongNetConfig._cfg(2, 1024))
    m = slide_encoder.LongNetViT(in_chans=1536, embed_dim=1024, depth=2, mlp_ratio=4, dropout=0.0, drop_path_rate=0.0,
                                 norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    W = orc.make_weights(cfg, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    m = m.to(DEV)
    calls, real = [], hip.dilated_attn_fwd_varlen
    monkeypatch.setattr(hip, "dilated_attn_fwd_varlen", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    sizes = [300, 1, 1100]
    syn = lambda i, n: orc.synthetic_slide(n, seed_x=40 + i, seed_c=90 + i)   # noqa: E731  (_slides' seeds)
    slides = _slides(sizes)
    if not train:
        with torch.no_grad():
            got = m.eval().forward_packed(slides, all_layer_embed=True)
        assert len(calls) == 2 - (1 if runtime.CLS_TAIL else 0)
        Wt = {k: torch.from_numpy(v) for k, v in W.items()}
        for i, n in enumerate(sizes):
            x, c = syn(i, n)
            ref = torch.stack(orc.slide_encoder_forward(Wt, x, c, cfg, all_layer_embed=True)).numpy()
            check_vectors("24l1024d depth 2 packed vs oracle", "slide %d" % n, torch.stack(got[i]).cpu().numpy(), ref)
        return
    m.enable_training().train()                                # the varlen backward covers D = 48: per-slide fallback
    packed = m.forward_packed(slides, all_layer_embed=True)
    assert len(calls) == 0 and all(t.grad_fn is not None for o in packed for t in o)
    for (x, c), o in zip(slides, packed):
        assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(o, m(x[None], c[None], all_layer_embed=True)))
