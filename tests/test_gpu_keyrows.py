"""The key-row tail (run with -m gpu on an MI355X): the second-to-last encoder layer and the last
layer's QKV GEMM for the rows the CLS query's keys name.

Kernel level, all bit-exact against the full entry points on the same inputs: the query-list attention launch
(gp_dilated_attn_fwd_rows) on the listed rows with every other row left at a sentinel, the listed-token merge
(gp_branch_merge_ln_rows), and the CLS kernel reading compact rows through a row map (gp_cls_attn_merge_ln_map).

Model level: with the switch on and off (runtime.KEYROW_TAIL) embeddings 0 .. depth-2 are bit-identical and the
last two pass tests/test_gpu_model.py's check against the CPU oracle.  Sizes: the product schedule engages from
L = 7,842 tokens on, so B = 1 runs N = 7,841 (the oracle forward there is most of the test's ~25 s; no golden
entry exists at that size, so the check is check_vectors with no reference deviation, as for N = 4,097); B = 2
runs a model built with max_wsi_size = 16,384, whose five-branch schedule (1024 .. 4096) engages from L = 3,134,
at N = 3,199, against the oracle of that schedule."""
import numpy as np
import pytest
import torch

import oracle as orc
from test_gpu_cls_tail import _check_last
from test_gpu_model import check_vectors

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = "gigapath_slide_enc12l768d"
CFG = orc.arch_config(ARCH)
SEGS, RATIOS, H, D = CFG["segment_length"], CFG["dilated_ratio"], 16, 48
E = H * D
SCALED = ([64, 362, 2048], [1, 2, 4])
FMTS = {"bf16": (torch.bfloat16, False), "fp16": (torch.float16, False), "f16_vbf16": (torch.float16, True)}


def _hip():
    from gigapath import _hip
    _hip.load_library()
    return _hip


def _plan(L, segs, ratios):
    from gigapath import runtime
    return runtime.key_row_plan(L, segs, ratios)


def _qkv(B, L, seed, fmt="bf16"):
    """[B*L, 3E] device qkv with the product path's pre-scaled q (values exact in bf16 and fp16)."""
    dt, vbf = FMTS[fmt]
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.standard_normal((B * L, 3 * E)).astype(np.float32))
    t[:, :E] *= D ** -0.5 * 1.4426950408889634
    t = t.bfloat16().half().float()
    dq = t.to(dt)
    if vbf:
        dq[:, 2 * E:] = t[:, 2 * E:].bfloat16().view(torch.float16)
    return dq.to(DEV).contiguous(), vbf


def _attn_buffers(B, L, segs, ratios, dt, sentinel=None):
    outs, lses = [], []
    for sl, r in zip(segs, ratios):
        geo = orc.branch_geometry(L, sl, r, H)
        n_o, n_l = B * geo["nseg"] * geo["m"] * H * D, B * geo["nseg"] * H * geo["m"]
        if sentinel is None:
            outs.append(torch.zeros(n_o, dtype=dt, device=DEV))
            lses.append(torch.zeros(n_l, dtype=torch.float32, device=DEV))
        else:
            outs.append(torch.full((n_o,), sentinel, dtype=dt, device=DEV))
            lses.append(torch.full((n_l,), sentinel, dtype=torch.float32, device=DEV))
    return outs, lses


def _listed_mask(B, L, sl, r, group):
    """[B, nseg, m, H] bool: (sparse row, head) pairs of the branch that the list launch must write."""
    geo = orc.branch_geometry(L, sl, r, H)
    off, idx = group
    mask = np.zeros((B, geo["nseg"], geo["m"], H), dtype=bool)
    for n in range(geo["nseg"]):
        for j in range(r):
            rows = idx[off[n * r + j]:off[n * r + j + 1]]
            h0 = j * geo["hpg"]
            mask[:, n, rows, h0:min(H, h0 + geo["hpg"])] = True
    return torch.from_numpy(mask)


def _compare_list_launch(h, dq, vbf, B, L, segs, ratios, groups):
    """Runs the full launch and the list launch; listed rows bit-identical, the rest untouched."""
    SENT = 777.0
    full_o, full_l = _attn_buffers(B, L, segs, ratios, dq.dtype)
    h.dilated_attn_fwd(dq, dq[:, E:], dq[:, 2 * E:], 3 * E, B, L, H, D, segs, ratios, full_o, full_l, 0.0, True,
                       v_bf16=vbf)
    got_o, got_l = _attn_buffers(B, L, segs, ratios, dq.dtype, sentinel=SENT)
    plan = h.AttnRowsPlan(dq, B, L, H, D, segs, ratios, groups, got_o, got_l)
    h.dilated_attn_fwd_rows(plan, True, v_bf16=vbf)
    torch.cuda.synchronize()
    sent16 = torch.full((1,), SENT, dtype=dq.dtype).view(torch.int16).item()
    for b, (sl, r) in enumerate(zip(segs, ratios)):
        geo = orc.branch_geometry(L, sl, r, H)
        mask = _listed_mask(B, L, sl, r, groups[b])
        shape = (B, geo["nseg"], geo["m"], H)
        fo = full_o[b].view(torch.int16).cpu().view(*shape, D)
        go = got_o[b].view(torch.int16).cpu().view(*shape, D)
        assert mask.any()
        assert torch.equal(go[mask], fo[mask]), (b, "o of listed rows")
        assert (go[~mask] == sent16).all(), (b, "o of unlisted rows")
        ml = mask.permute(0, 1, 3, 2)                                   # lse: [B, nseg, H, m]
        fl = full_l[b].view(torch.int32).cpu().view(B, geo["nseg"], H, geo["m"])
        gl = got_l[b].view(torch.int32).cpu().view(B, geo["nseg"], H, geo["m"])
        assert torch.equal(gl[ml], fl[ml]), (b, "lse of listed rows")
        assert (got_l[b].cpu().view(B, geo["nseg"], H, geo["m"])[~ml] == SENT).all(), (b, "lse of unlisted rows")
    return full_o, full_l


# ------------------------------------------------------------------ attention over a query list
@pytest.mark.parametrize("name,fmt,B,L,sched", [
    ("scaled", "bf16", 2, 2500, SCALED), ("scaled", "f16_vbf16", 2, 2500, SCALED),
    ("product", "bf16", 1, 6001, (SEGS, RATIOS))])
def test_attention_list_launch_matches_full_launch(name, fmt, B, L, sched):
    h = _hip()
    segs, ratios = sched
    _, _, groups = _plan(L, segs, ratios)
    # what these shapes are here to cover
    cnts = np.concatenate([np.diff(off) for off, _ in groups])
    assert (cnts == 0).any(), "a group with an empty list"
    assert name != "scaled" or ((cnts > 0) & (cnts < 32)).any(), "a list of fewer than 32 rows"
    assert (cnts % 256 != 0).any(), "a list that ends mid-block"
    assert any(L % min(sl, L) for sl in segs), "a tail segment shorter than its nominal length"
    dq, vbf = _qkv(B, L, seed=L + B, fmt=fmt)
    _compare_list_launch(h, dq, vbf, B, L, segs, ratios, groups)


def test_attention_list_launch_overflow_fixup():
    """test_gpu_kernels.py's no-max overflow construction (head 0: one key 200 log2 units up, so exp2 overflows
    fp32; head 1: scores climbing 30 per tile): the listed rows are flagged by the fast kernel and recomputed
    by the list launch's own fixup pass, bit for bit as the full launch's."""
    h = _hip()
    L = 300
    rng = np.random.default_rng(21)
    qkv = torch.from_numpy(rng.standard_normal((L, 3 * E)).astype(np.float32)) * 0.3
    qkv[:, 0:2 * D] = 0.0
    qkv[:, 0] = 8.0
    qkv[:, D] = 8.0
    qkv[:, E:E + 2 * D] = 0.0
    qkv[150, E] = 25.0
    qkv[:, E + D] = torch.from_numpy((np.arange(L) // 64) * 3.75).float()
    dq = qkv.bfloat16().to(DEV).contiguous()
    rows = np.array([0, 5, 31, 32, 150, 299], dtype=np.int32)
    groups = [(np.array([0, rows.size], dtype=np.int32), rows)]
    full_o, full_l = _compare_list_launch(h, dq, False, 1, L, [300], [1], groups)
    o = full_o[0].float().cpu().view(L, H, D)
    assert torch.isfinite(o).all() and torch.isfinite(full_l[0]).all()          # (the fixup pass did run)
    v = dq[:, 2 * E:].float().cpu().view(L, H, D)
    assert (o[5, 0] - v[150, 0]).abs().max().item() <= 1e-2 * max(1.0, v[150, 0].abs().max().item())


# ------------------------------------------------------------------ merge over a token list
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("ln", [True, False])
def test_list_merge_matches_full_merge(fmt, ln):
    h = _hip()
    dt = FMTS[fmt][0]
    B, L = 2, 6001
    rows, _, _ = _plan(L, SEGS, RATIOS)
    rng = np.random.default_rng(5)
    outs, lses = [], []
    for sl, r in zip(SEGS, RATIOS):
        geo = orc.branch_geometry(L, sl, r, H)
        outs.append(torch.from_numpy(rng.standard_normal(B * geo["nseg"] * geo["m"] * E).astype(np.float32)).to(dt).to(DEV))
        l = rng.standard_normal(B * geo["nseg"] * H * geo["m"]).astype(np.float32) * 3
        l[::97] = 0.0                                                   # lse == 0 counts as uncovered (:46)
        lses.append(torch.from_numpy(l).to(DEV))
    lw = torch.from_numpy((1 + 0.1 * rng.standard_normal(E)).astype(np.float32)).to(DEV) if ln else None
    lb = torch.from_numpy((0.1 * rng.standard_normal(E)).astype(np.float32)).to(DEV) if ln else None
    full = torch.zeros(B * L, E, dtype=dt, device=DEV)
    h.branch_merge_ln(outs, lses, SEGS, RATIOS, B, L, H, D, lw, lb, 1e-5, full)
    drows = torch.from_numpy(rows).to(DEV)
    got = torch.full((B * rows.size, E), 7.0, dtype=dt, device=DEV)
    h.branch_merge_ln_rows(outs, lses, SEGS, RATIOS, B, L, drows, H, D, lw, lb, 1e-5, got)
    torch.cuda.synchronize()
    idx = (torch.arange(B)[:, None] * L + torch.from_numpy(rows.astype(np.int64))[None, :]).reshape(-1).to(DEV)
    assert torch.equal(got.view(torch.int16), full[idx].view(torch.int16))


# ------------------------------------------------------------------ CLS kernel on compact rows
@pytest.mark.parametrize("fmt", ["bf16", "f16_vbf16"])
def test_cls_kernel_with_row_map(fmt):
    """Two slides; the compact buffer holds S plus 300 tokens the CLS query never reads.  Mapped output ==
    unmapped output on the full buffer, also with those extra rows poisoned with NaN."""
    h = _hip()
    B, L = 2, 6001
    rows, _, _ = _plan(L, SEGS, RATIOS)
    extra = np.setdiff1d(np.arange(L), rows)[:300]
    comp = np.sort(np.concatenate([rows, extra])).astype(np.int64)
    row_map = np.full(L, -1, dtype=np.int32)
    row_map[comp] = np.arange(comp.size, dtype=np.int32)
    n = comp.size
    dq, vbf = _qkv(B, L, seed=11, fmt=fmt)
    rng = np.random.default_rng(3)
    lw = torch.from_numpy((1 + 0.1 * rng.standard_normal(E)).astype(np.float32)).to(DEV)
    lb = torch.from_numpy((0.1 * rng.standard_normal(E)).astype(np.float32)).to(DEV)
    lens = torch.full((B,), L, dtype=torch.int64, device=DEV)
    ws = torch.empty(h.cls_attn_workspace_bytes(L, B, H, D, SEGS, RATIOS), dtype=torch.uint8, device=DEV)

    def run(qkv, off, **kw):
        out = torch.full((B, E), float("nan"), dtype=dq.dtype, device=DEV)
        h.cls_attn_merge_ln(qkv, qkv[:, E:], qkv[:, 2 * E:], 3 * E, off, lens, L, H, D, SEGS, RATIOS, lw, lb, 1e-5,
                            out, ws, 0.0, True, v_bf16=vbf, **kw)
        torch.cuda.synchronize()
        return out.view(torch.int16).cpu()

    want = run(dq, torch.arange(B, dtype=torch.int64, device=DEV) * L)
    gather = (torch.arange(B)[:, None] * L + torch.from_numpy(comp)[None, :]).reshape(-1).to(DEV)
    cq = dq[gather].contiguous()
    off = torch.arange(B, dtype=torch.int64, device=DEV) * n
    dmap = torch.from_numpy(row_map).to(DEV)
    assert torch.equal(run(cq, off, row_map=dmap, map_rows=n), want)
    poison = torch.from_numpy(np.isin(comp, extra)).repeat(B).to(DEV)
    cq[poison] = float("nan")
    assert torch.equal(run(cq, off, row_map=dmap, map_rows=n), want)


# ------------------------------------------------------------------ model
def _make_model(**kw):
    from gigapath import slide_encoder
    m = slide_encoder.create_model("", ARCH, 1536, **kw)
    W = orc.make_weights(CFG, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def model():
    return _make_model()


def _with_switch(model, monkeypatch, on, fn, timed=True):
    """fn() with runtime.KEYROW_TAIL = on and a fresh engine state; returns (result, TIMER span names).
    timed=False leaves the span timer off (a timed forward is never captured into a HIP graph)."""
    from gigapath import runtime
    eng = model.encoder.engine
    monkeypatch.setattr(runtime, "KEYROW_TAIL", on)
    for t in (eng._ws, eng._pws):
        t.clear()
    runtime.TIMER.reset()
    runtime.TIMER.enabled = timed
    try:
        with torch.no_grad():
            res = fn()
        torch.cuda.synchronize()
        return res, set(runtime.TIMER.events)
    finally:
        runtime.TIMER.enabled = False
        runtime.TIMER.reset()
        for t in (eng._ws, eng._pws):
            t.clear()


def _on_off(model, monkeypatch, N, B):
    x, coords = orc.synthetic_slide(N, B=B)
    xt, ct = torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV)
    run = lambda: torch.stack(model(xt, ct, all_layer_embed=True)).cpu().numpy()   # noqa: E731
    on, spans_on = _with_switch(model, monkeypatch, True, run)
    off, spans_off = _with_switch(model, monkeypatch, False, run)
    assert "keyrow_merge" in spans_on and "keyrow_attn" in spans_on and "keyrow_merge" not in spans_off
    depth = CFG["depth"]
    assert on.shape == off.shape == (depth + 1, B, 768)
    assert np.array_equal(on[:depth - 1], off[:depth - 1])
    return x, coords, on, off


def test_model_on_off_product_schedule(model, golden_meta, monkeypatch):
    N, B, depth = 7841, 1, CFG["depth"]
    x, coords, on, off = _on_off(model, monkeypatch, N, B)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    Wt = {k: torch.from_numpy(v) for k, v in orc.make_weights(CFG, seed=0).items()}
    with torch.no_grad():
        ref = torch.stack(orc.slide_encoder_forward(Wt, x, coords, CFG, all_layer_embed=True)).numpy()
    for name, got in (("key rows on", on), ("key rows off", off)):
        for slot in (depth - 1, depth):
            _check_last(golden_meta, "key-row tail N=%d B=%d %s slot %d" % (N, B, name, slot), got[slot], ref[slot],
                        N, B)


def test_model_on_off_batch_of_two_scaled_schedule(monkeypatch):
    N, B, depth = 3199, 2, CFG["depth"]
    cfg = orc.arch_config(ARCH, max_wsi_size=16384)
    m = _make_model(max_wsi_size=16384)
    assert list(m.encoder.layers[0].self_attn.args.segment_length) == cfg["segment_length"]
    x, coords, on, off = _on_off(m, monkeypatch, N, B)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    Wt = {k: torch.from_numpy(v) for k, v in orc.make_weights(CFG, seed=0).items()}
    with torch.no_grad():
        ref = torch.stack(orc.slide_encoder_forward(Wt, x, coords, cfg, all_layer_embed=True)).numpy()
    for name, got in (("key rows on", on), ("key rows off", off)):
        for slot in (depth - 1, depth):
            check_vectors("key-row tail scaled N=%d B=%d %s slot %d" % (N, B, name, slot), "embed", got[slot],
                          ref[slot], 0.0)


def test_engagement(model, monkeypatch):
    """Taken at N = 10,000 with the CLS readout; not at N = 4,097 (62 % of the rows are needed), under
    global_pool, on the packed forward, or with the switch off."""
    def fwd(N, packed=False):
        x, coords = orc.synthetic_slide(N)
        xt, ct = torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV)
        if packed:
            return lambda: model.forward_packed([(xt[0], ct[0])], all_layer_embed=True)
        return lambda: model(xt, ct, all_layer_embed=True)

    taken = lambda on, fn: "keyrow_merge" in _with_switch(model, monkeypatch, on, fn)[1]   # noqa: E731
    assert taken(True, fwd(10000))
    assert not taken(False, fwd(10000))
    assert not taken(True, fwd(4097))
    assert not taken(True, fwd(10000, packed=True))
    model.global_pool = True
    try:
        assert not taken(True, fwd(10000))
    finally:
        model.global_pool = False


def test_graph_replay_matches_eager(model, monkeypatch):
    x, coords = orc.synthetic_slide(10000)
    xt, ct = torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV)
    run = lambda: torch.stack(model(xt, ct, all_layer_embed=True))   # noqa: E731
    eager, spans = _with_switch(model, monkeypatch, True, run)
    assert "keyrow_merge" in spans
    model.use_hip_graphs, model.graph_min_uses = True, 1
    try:
        reps = [_with_switch(model, monkeypatch, True, run, timed=False)[0] for _ in range(2)]
        assert len(model._graphs) == 1
    finally:
        model.use_hip_graphs, model.graph_min_uses = False, 2
        for k in list(model._graphs):
            model._drop_graph(k)
        model._graph_seen.clear()
    for rep in reps:
        assert torch.equal(rep, eager)
