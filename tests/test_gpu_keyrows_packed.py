"""The key-row tail on packed slides (-m gpu): the per-slide list attention, listed merge and CLS row
maps, bit-exact against the full packed entry points on the same inputs, and forward_packed with
runtime.KEYROW_TAIL_PACKED on / off on test_gpu_keyrows.py's max_wsi_size = 16,384 schedule (engages from L = 3,134)."""
import numpy as np
import pytest
import torch

import oracle as orc
from test_gpu_keyrows import (ARCH, CFG, D, DEV, E, FMTS, H, RATIOS, SCALED, SEGS, _hip, _listed_mask, _make_model,
                              _qkv, _with_switch)
from test_gpu_model import check_vectors

pytestmark = pytest.mark.gpu


def _packed_plan(Ls, segs, ratios):                      # every slide lists its own S_i, whatever its share
    from gigapath import runtime
    return runtime.packed_key_row_plan(Ls, segs, ratios, max_share=1.0)


def _varlen(h, dq, Ls, segs, ratios, fill):
    plan = h.VarlenPlan(Ls, H, D, segs, ratios)
    outs = [torch.full((n,), fill, dtype=dq.dtype, device=DEV) for n in plan.o_elems]
    lses = [torch.full((n,), fill, dtype=torch.float32, device=DEV) for n in plan.lse_elems]
    return plan.bind(dq, outs, lses), outs, lses


def _compare_packed_list_launch(h, dq, vbf, Ls, segs, ratios, groups):
    """The full varlen launch and the list launch: listed rows bit-identical, every other element untouched."""
    SENT = 777.0
    full, full_o, full_l = _varlen(h, dq, Ls, segs, ratios, 0.0)
    h.dilated_attn_fwd_varlen(full, True, v_bf16=vbf)
    vplan, got_o, got_l = _varlen(h, dq, Ls, segs, ratios, SENT)
    h.dilated_attn_fwd_rows(h.AttnRowsPlanVarlen(vplan, groups), True, v_bf16=vbf)
    torch.cuda.synchronize()
    sent16 = torch.full((1,), SENT, dtype=dq.dtype).view(torch.int16).item()
    for b, (sl, r, (off, idx)) in enumerate(zip(segs, ratios, groups)):
        fo, go = full_o[b].view(torch.int16).cpu(), got_o[b].view(torch.int16).cpu()
        fl, gl = full_l[b].view(torch.int32).cpu(), got_l[b].view(torch.int32).cpu()
        g0 = o0 = l0 = 0
        for L in Ls:                                     # the slide's groups and its o / lse regions
            geo = orc.branch_geometry(L, sl, r, H)
            ng, nrow = geo["nseg"] * r, geo["nseg"] * geo["m"]
            mask = _listed_mask(1, L, sl, r, (off[g0:g0 + ng + 1], idx))[0]          # [nseg, m, H]
            so, sg = fo[o0:o0 + nrow * E].view(geo["nseg"], geo["m"], H, D), go[o0:o0 + nrow * E].view(geo["nseg"], geo["m"], H, D)
            assert torch.equal(sg[mask], so[mask]), (b, L, "o of listed rows")
            assert (sg[~mask] == sent16).all(), (b, L, "o of unlisted rows")
            ml = mask.permute(0, 2, 1)
            sl_f, sl_g = fl[l0:l0 + nrow * H].view(geo["nseg"], H, geo["m"]), gl[l0:l0 + nrow * H].view(geo["nseg"], H, geo["m"])
            assert torch.equal(sl_g[ml], sl_f[ml]), (b, L, "lse of listed rows")
            assert (sl_g[~ml].view(torch.float32) == SENT).all(), (b, L, "lse of unlisted rows")
            g0, o0, l0 = g0 + ng, o0 + nrow * E, l0 + nrow * H
    return full_o, full_l


@pytest.mark.parametrize("fmt", ["bf16", "f16_vbf16"])
@pytest.mark.parametrize("name,Ls,sched", [("scaled", [2500, 17, 3300], SCALED), ("product", [6001, 1025], (SEGS, RATIOS))])
def test_packed_list_launch_matches_varlen_launch(name, fmt, Ls, sched):
    h = _hip()
    segs, ratios = sched
    plan = _packed_plan(Ls, segs, ratios)
    if name == "scaled":
        assert plan["n"][1] == 17, "the 17-token slide (shorter than one key tile) lists all of its tokens"
    cnts = np.concatenate([np.diff(off) for off, _ in plan["groups"]])
    assert (cnts == 0).any(), "a group with an empty list"
    assert ((cnts > 0) & (cnts < 32)).any(), "a list of fewer than 32 rows"
    assert (cnts % 256 != 0).any(), "a list that ends mid-block"
    assert any(L % min(sl, L) for L in Ls for sl in segs), "a tail segment shorter than its nominal length"
    dq, vbf = _qkv(1, sum(Ls), seed=sum(Ls), fmt=fmt)
    _compare_packed_list_launch(h, dq, vbf, Ls, segs, ratios, plan["groups"])


def test_packed_list_launch_overflow_fixup():
    """test_gpu_keyrows.py's overflow construction as the SECOND slide of a pack: the list launch's fixup pass."""
    h = _hip()
    L0, L = 200, 300
    rng = np.random.default_rng(21)
    qkv = torch.from_numpy(rng.standard_normal((L0 + L, 3 * E)).astype(np.float32)) * 0.3
    s = qkv[L0:]
    s[:, 0:2 * D] = 0.0
    s[:, 0] = s[:, D] = 8.0
    s[:, E:E + 2 * D] = 0.0
    s[150, E] = 25.0
    s[:, E + D] = torch.from_numpy((np.arange(L) // 64) * 3.75).float()
    dq = qkv.bfloat16().to(DEV).contiguous()
    groups = [(np.array([0, 2, 8], dtype=np.int32), np.array([0, 7, 0, 5, 31, 32, 150, 299], dtype=np.int32))]
    full_o, full_l = _compare_packed_list_launch(h, dq, False, [L0, L], [300], [1], groups)
    assert torch.isfinite(full_o[0].float()).all() and torch.isfinite(full_l[0]).all()   # (the fixup pass did run)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("ln", [True, False])
def test_packed_list_merge_matches_varlen_merge(fmt, ln):
    h = _hip()
    dt = FMTS[fmt][0]
    Ls, T = [6001, 17, 1025], 6001 + 17 + 1025
    rows = _packed_plan(Ls, SEGS, RATIOS)["rows"]
    rng = np.random.default_rng(5)
    vplan = h.VarlenPlan(Ls, H, D, SEGS, RATIOS)
    outs = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dt).to(DEV) for n in vplan.o_elems]
    lses = [torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 3).to(DEV) for n in vplan.lse_elems]
    for l in lses:
        l[::97] = 0.0                                                   # lse == 0 counts as uncovered (:46)
    vplan.bind(torch.zeros(T, 3 * E, dtype=dt, device=DEV), outs, lses)
    lw = torch.from_numpy((1 + 0.1 * rng.standard_normal(E)).astype(np.float32)).to(DEV) if ln else None
    lb = torch.from_numpy((0.1 * rng.standard_normal(E)).astype(np.float32)).to(DEV) if ln else None
    full = torch.zeros(T, E, dtype=dt, device=DEV)
    h.branch_merge_ln_varlen(vplan, lw, lb, 1e-5, full)
    got = torch.full((rows.size, E), 7.0, dtype=dt, device=DEV)
    h.branch_merge_ln_rows_varlen(vplan, torch.from_numpy(rows).to(DEV), lw, lb, 1e-5, got)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), full[torch.from_numpy(rows.astype(np.int64)).to(DEV)].view(torch.int16))


@pytest.mark.parametrize("fmt", ["bf16", "f16_vbf16"])
def test_cls_kernel_with_per_slide_maps(fmt):
    """Each slide's compact rows hold its S_i plus 300 unread tokens, then poisoned with NaN."""
    h = _hip()
    Ls = [6001, 2500]
    tok_off = np.concatenate([[0], np.cumsum(Ls)]).astype(np.int64)
    plan = _packed_plan(Ls, SEGS, RATIOS)
    comp, maps, extras, c_off = [], [], [], [0]
    for i, L in enumerate(Ls):
        s_i = plan["rows"][plan["off"][i]:plan["off"][i] + plan["n"][i]].astype(np.int64) - tok_off[i]
        extra = np.setdiff1d(np.arange(L), s_i)[:300]
        c = np.sort(np.concatenate([s_i, extra]))
        m = np.full(L, -1, dtype=np.int32)
        m[c] = np.arange(c.size, dtype=np.int32)
        comp.append(c + tok_off[i]); maps.append(m); extras.append(np.isin(c, extra)); c_off.append(c_off[-1] + c.size)
    dq, vbf = _qkv(1, int(tok_off[-1]), seed=11, fmt=fmt)
    lens = torch.tensor(Ls, dtype=torch.int64, device=DEV)
    ws = torch.empty(h.cls_attn_workspace_bytes(max(Ls), 2, H, D, SEGS, RATIOS), dtype=torch.uint8, device=DEV)

    def run(qkv, off, **kw):
        out = torch.full((2, E), float("nan"), dtype=dq.dtype, device=DEV)
        h.cls_attn_merge_ln(qkv, qkv[:, E:], qkv[:, 2 * E:], 3 * E, off, lens, max(Ls), H, D, SEGS, RATIOS, None, None,
                            1e-5, out, ws, 0.0, True, v_bf16=vbf, **kw)
        torch.cuda.synchronize()
        return out.view(torch.int16).cpu()

    want = run(dq, torch.from_numpy(tok_off[:-1]).to(DEV))
    cq = dq[torch.from_numpy(np.concatenate(comp)).to(DEV)].contiguous()
    kw = dict(row_map=torch.from_numpy(np.concatenate(maps)).to(DEV), map_rows=c_off[-1],
              map_off=torch.from_numpy(tok_off[:-1]).to(DEV))
    off = torch.tensor(c_off[:-1], dtype=torch.int64, device=DEV)
    assert torch.equal(run(cq, off, **kw), want)
    cq[torch.from_numpy(np.concatenate(extras)).to(DEV)] = float("nan")
    assert torch.equal(run(cq, off, **kw), want)


NS = (3199, 3500, 600)


@pytest.fixture(scope="module")
def model():
    return _make_model(max_wsi_size=16384)


def _packed_run(model, monkeypatch, on, timed=True):
    from gigapath import runtime
    monkeypatch.setattr(runtime, "KEYROW_TAIL_PACKED", on)
    slides = []
    for i, N in enumerate(NS):
        x, coords = orc.synthetic_slide(N, seed_x=1 + i)
        slides.append((torch.from_numpy(x[0]).to(DEV), torch.from_numpy(coords[0]).to(DEV)))
    run = lambda: torch.stack([torch.cat(o, 0) for o in model.forward_packed(slides, all_layer_embed=True)], 1)  # noqa: E731
    return _with_switch(model, monkeypatch, True, run, timed)


def test_model_packed_on_off_and_graph_replay(model, monkeypatch):
    depth, cfg = CFG["depth"], orc.arch_config(ARCH, max_wsi_size=16384)
    on, spans_on = _packed_run(model, monkeypatch, True)
    off, spans_off = _packed_run(model, monkeypatch, False)
    assert {"keyrow_attn", "keyrow_merge"} <= spans_on and not {"keyrow_attn", "keyrow_merge"} & spans_off
    model.use_hip_graphs, model.graph_min_uses = True, 1   # one captured packed graph, replayed twice, == eager
    try:
        reps = [_packed_run(model, monkeypatch, True, timed=False)[0] for _ in range(2)]
        assert len(model._graphs) == 1 and all(torch.equal(rep, on) for rep in reps)
    finally:
        model.use_hip_graphs, model.graph_min_uses = False, 2
        for k in list(model._graphs):
            model._drop_graph(k)
        model._graph_seen.clear()
    on, off = on.cpu().numpy(), off.cpu().numpy()
    assert np.array_equal(on[:depth - 1], off[:depth - 1])
    Wt = {k: torch.from_numpy(v) for k, v in orc.make_weights(CFG, seed=0).items()}
    for i, N in enumerate(NS):
        x, coords = orc.synthetic_slide(N, seed_x=1 + i)
        with torch.no_grad():
            ref = torch.stack(orc.slide_encoder_forward(Wt, x, coords, cfg, all_layer_embed=True)).numpy()
        for name, got in (("on", on), ("off", off)):
            for slot in (depth - 1, depth):
                check_vectors("packed key-row tail N=%d %s slot %d" % (N, name, slot), "embed", got[slot, i:i + 1],
                              ref[slot], 0.0)
