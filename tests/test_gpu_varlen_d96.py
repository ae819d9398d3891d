"""Packed (varlen) batches at D = 96 on the MI355X (run with -m gpu): the D = 96 LDS-DMA fast + fixup attention pair,
the E = 1536 varlen merge and forward_packed on the 12L1536d arch.  H = 16, bf16, q NOT pre-scaled (the kernel scales
the fp32 scores by D^-0.5 log2 e).  Packs B / A / arch and the derived bounds |o - ref| <= 2^-8 (|ref| + max|v|),
|lse - ref| <= 2^-8 are test_gpu_varlen_d64's (they do not depend on D); measured worst err / bound: DESIGN §3.16."""
import functools

import numpy as np
import pytest
import torch

import oracle as orc
from test_dilated_bwd_host import LN2, LOG2E
from test_gpu_kernels import _rows_needed
from test_gpu_varlen_d64 import BOUND, PACKS, REDO, _regions as _regions64, _same

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, D, E = 16, 96, 1536


@functools.lru_cache(maxsize=None)
def _inputs(pack, gain=1):
    T = sum(PACKS[pack][1])
    qkv = torch.from_numpy(np.random.Generator(np.random.PCG64(9600 + T)).standard_normal((T, 3 * E)).astype(np.float32))
    qkv[:, :E] *= gain
    return qkv.bfloat16().to(DEV)


def _forward(qkv, pack):
    from gigapath import _hip, runtime
    vs = runtime.VarlenScratch(torch.device(DEV), PACKS[pack][1], H, D, *PACKS[pack][0], qkv)
    for t in vs.outs + vs.lses:
        t.zero_()
    _hip.dilated_attn_fwd_varlen(vs.plan, False)
    torch.cuda.synchronize()
    return vs


_baseline = functools.lru_cache(maxsize=None)(lambda pack, gain=1: _forward(_inputs(pack, gain), pack))


def _regions(pack):
    """The D = 64 test's per-slide regions (same packs, same H), the o offsets scaled from E = 1024 rows to 1536."""
    return [(t0, L, [(o0 // 1024 * E, o1 // 1024 * E, l0, l1, g) for o0, o1, l0, l1, g in br])
            for t0, L, br in _regions64(pack)]


@pytest.mark.parametrize("pack,gain", [("B", 1), ("A", 1), ("arch", 1), ("B", 40)])
def test_forward_against_fp64(pack, gain):
    """The rows the merge reads against float64: gather, scores times D^-0.5 log2 e (a zero-pad key scores 0 with
    v = 0), softmax, P.V.  gain 40: every branch must hold a needed real row whose real-key log2 sum lies outside
    +-100 -- asserted from the reference alone -- so the fixup pass runs."""
    (segs, ratios), _ = PACKS[pack]
    x, vs = _inputs(pack, gain).double().cpu().numpy(), _baseline(pack, gain)
    vmax = np.abs(x[:, 2 * E:]).max()
    worst, flagged = [0.0, 0.0], [False] * len(segs)
    for t0, L, br in _regions(pack):
        q, k, v = (x[t0:t0 + L, i * E:(i + 1) * E].reshape(L, H, D) for i in range(3))
        for b, (o0, o1, l0, l1, g) in enumerate(br):
            nseg, m = g["nseg"], g["m"]
            idx = orc.gather_index(L, segs[b], ratios[b], H)                     # [nseg, H, m], -1: zero pad
            o = vs.outs[b][o0:o1].double().cpu().numpy().reshape(nseg, m, H, D)
            assert not (vs.lses[b][l0:l1].view(torch.int32) == REDO).any(), (pack, L, b)
            lse = vs.lses[b][l0:l1].double().cpu().numpy().reshape(nseg, H, m)
            need = np.arange(m)[None, None, :] < _rows_needed(L, segs[b], ratios[b], H)[:, :, None]
            for h in range(H):
                ok, nd = idx[:, h] >= 0, need[:, h]                              # [nseg, m]
                qs, ks, vv = (np.where(ok[..., None], t[np.maximum(idx[:, h], 0), h], 0.0) for t in (q, k, v))
                s = np.einsum("nid,njd->nij", qs, ks) * (D ** -0.5 * LOG2E)
                mx = s.max(-1, keepdims=True)
                p = np.exp2(s - mx)
                ref_o = np.einsum("nij,njd->nid", p, vv) / p.sum(-1)[..., None]
                ref_l = (mx[..., 0] + np.log2(p.sum(-1))) * LN2
                real = mx[..., 0] + np.log2(np.maximum((p * ok[:, None, :]).sum(-1), 1e-300))
                flagged[b] |= bool((np.abs(real) > 100)[nd & ok].any())
                eo = np.abs(o[:, :, h] - ref_o) / (BOUND * (np.abs(ref_o) + vmax))
                el = np.abs(lse[:, h] - ref_l) / BOUND
                assert np.isfinite(o[:, :, h][nd]).all() and np.isfinite(lse[:, h][nd]).all()
                worst = [max(worst[0], eo[nd].max(initial=0)), max(worst[1], el[nd].max(initial=0))]
    print("varlen d96 %s gain %d: worst err / bound  o %.4f  lse %.4f  flagged %s" % (pack, gain, *worst, flagged))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    assert gain == 1 or all(flagged), flagged


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
                v = va if j == i else vl                        # va: slide i kept; vl: every slide but i kept
                assert _same([v.outs[b]], [base.outs[b]], slice(o0, o1)), (i, j, b)
                assert _same([v.lses[b].view(torch.int32)], [base.lses[b].view(torch.int32)], slice(l0, l1)), (i, j, b)


@pytest.mark.parametrize("with_ln", [True, False])
@pytest.mark.parametrize("pack", list(PACKS))
def test_varlen_merge_equals_the_per_slide_merge(pack, with_ln):
    """gp_branch_merge_ln_varlen at E = 1536 is gp_branch_merge_ln (B = 1) on each slide's regions, bit for bit."""
    from gigapath import _hip
    vs, (segs, ratios) = _baseline(pack), PACKS[pack][0]
    rng = np.random.Generator(np.random.PCG64(7))
    w, b_ = (torch.from_numpy(rng.standard_normal(E).astype(np.float32)).to(DEV) if with_ln else None for _ in "wb")
    got, want = (torch.full((sum(PACKS[pack][1]), E), -1024.0, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    _hip.branch_merge_ln_varlen(vs.plan, w, b_, 1e-5, got)
    for t0, L, br in _regions(pack):
        _hip.branch_merge_ln([vs.outs[b][o0:o1] for b, (o0, o1, _, _, _) in enumerate(br)],
                             [vs.lses[b][l0:l1] for b, (_, _, l0, l1, _) in enumerate(br)], segs, ratios, 1, L, H, D,
                             w, b_, 1e-5, want[t0:t0 + L])
    torch.cuda.synchronize()
    assert _same([got], [want]) and torch.isfinite(got.float()).all()


@pytest.mark.parametrize("train", [False, True])
def test_forward_packed_on_the_12l1536d_arch(train, monkeypatch):
    """gigapath_slide_enc12l1536d cut to depth 2, slides of 300, 1 and 1100 tiles: eval against the fp32 oracle per
    slide with one packed attention launch per full layer (the last layer is the CLS tail's when runtime.CLS_TAIL is
    on); under enable_training() no packed launch, and forward()'s bits per slide."""
    from gigapath import _hip as hip, runtime, slide_encoder
    from gigapath.torchscale.model import LongNetConfig
    from test_gpu_model import check_vectors
    from test_gpu_train_packed import _slides
    cfg = dict(orc.arch_config("gigapath_slide_enc12l1536d"), depth=2)
    monkeypatch.setitem(LongNetConfig.CONFIGS, "LongNet_2_layers_1536_dim", LongNetConfig._cfg(2, 1536))
    m = slide_encoder.LongNetViT(in_chans=1536, embed_dim=1536, depth=2, mlp_ratio=4, dropout=0.0, drop_path_rate=0.0,
                                 norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6))
    W = orc.make_weights(cfg, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    m = m.to(DEV)
    calls, real = [], hip.dilated_attn_fwd_varlen
    monkeypatch.setattr(hip, "dilated_attn_fwd_varlen", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    sizes = [300, 1, 1100]
    slides = _slides(sizes)
    if train:
        packed = m.enable_training().train().forward_packed(slides, all_layer_embed=True)
        assert len(calls) == 0 and all(t.grad_fn is not None for o in packed for t in o)
        for (x, c), o in zip(slides, packed):
            assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(o, m(x[None], c[None], all_layer_embed=True)))
        return
    with torch.no_grad():
        got = m.eval().forward_packed(slides, all_layer_embed=True)
    assert len(calls) == 2 - (1 if runtime.CLS_TAIL else 0)
    Wt = {k: torch.from_numpy(v) for k, v in W.items()}
    for i, n in enumerate(sizes):
        x, c = orc.synthetic_slide(n, seed_x=40 + i, seed_c=90 + i)             # _slides' seeds
        ref = torch.stack(orc.slide_encoder_forward(Wt, x, c, cfg, all_layer_embed=True)).numpy()
        check_vectors("12l1536d depth 2 packed vs oracle", "slide %d" % n, torch.stack(got[i]).cpu().numpy(), ref)
