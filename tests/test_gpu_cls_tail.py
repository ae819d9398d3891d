"""The last encoder layer for the CLS rows only (run with -m gpu on an MI355X).

Kernel level: gp_cls_attn_merge_ln against row 0 of oracle.branch_attention + oracle.merge_branches +
LayerNorm in fp32 on the CPU, on the product schedule.  The bound is not a constant: on the same inputs the
existing pair (gp_dilated_attn_fwd_ex with the query window [0, 1) + gp_branch_merge_ln_window(0, 1)) is run
too, and the new kernel's max abs error against the oracle must not exceed the pair's by more than one ulp
of the 16-bit output format at the output's magnitude (the final rounding alone can flip one ulp).

Model level: the same model and input with the tail on and off (runtime.CLS_TAIL): every embedding but the
last is bit-identical, the last passes the model tolerance of tests/test_gpu_model.py against the oracle.
"""
import numpy as np
import pytest
import torch

import oracle as orc
from conftest import record_parity
from test_gpu_model import check_tiny, check_vectors

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = orc.arch_config("gigapath_slide_enc12l768d")
SEGS, RATIOS, H = CFG["segment_length"], CFG["dilated_ratio"], 16
LN2, LOG2E = 0.6931471805599453, 1.4426950408889634
CHUNK = 256                       # keys per work item of gp_cls_attn_merge_ln's first launch


def _hip():
    from gigapath import _hip
    _hip.load_library()
    return _hip


# ------------------------------------------------------------------ kernel: shared inputs and references
_CASES = {}


def _case(L, D, prescaled, zero_q=False):
    """(qkv fp32 [L, 3E] whose values are exact in bf16 AND fp16, ln_w, ln_b, oracle row 0 [E]) -- built once
    per (L, D, prescaled) and shared by the three formats.  prescaled: q carries D^-1/2 * log2(e), so the
    oracle's scale is ln 2."""
    key = (L, D, prescaled, zero_q)
    if key not in _CASES:
        E = H * D
        rng = np.random.default_rng(1000 * D + L + (7 if prescaled else 0))
        qkv = torch.from_numpy(rng.standard_normal((L, 3 * E)).astype(np.float32))
        if prescaled:
            qkv[:, :E] *= D ** -0.5 * LOG2E
        if zero_q:
            qkv[:, :E] = 0.0
        qkv = qkv.bfloat16().half().float()          # 8 significant bits inside fp16's range: exact in both
        assert torch.equal(qkv.bfloat16().float(), qkv) and torch.equal(qkv.half().float(), qkv)
        lw = torch.from_numpy((1 + 0.1 * rng.standard_normal(E)).astype(np.float32))
        lb = torch.from_numpy((0.1 * rng.standard_normal(E)).astype(np.float32))
        _CASES[key] = (qkv, lw, lb, _oracle_row0(qkv, L, D, LN2 if prescaled else None, lw, lb))
    return _CASES[key]


def _oracle_row0(qkv, L, D, scale, lw, lb):
    E = H * D
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(1, L, H, D) for i in range(3))
    outs, lses = [], []
    for sl, r in zip(SEGS, RATIOS):
        o, l = orc.branch_attention(q, k, v, sl, r, **({"scale": scale} if scale else {}))
        outs.append(o)
        lses.append(l)
    row = orc.merge_branches(outs, lses, L, SEGS, RATIOS)[0, :1]
    return torch.nn.functional.layer_norm(row, (E,), lw, lb, 1e-5)[0]


FMTS = {"bf16": (torch.bfloat16, False), "fp16": (torch.float16, False), "f16_vbf16": (torch.float16, True)}


def _device_qkv(qkv, D, fmt):
    dt, vbf = FMTS[fmt]
    E = H * D
    dq = qkv.to(dt)
    if vbf:
        dq[:, 2 * E:] = qkv[:, 2 * E:].bfloat16().view(torch.float16)
    return dq.to(DEV).contiguous(), vbf


def _run_cls(h, dq, offs, lens, D, prescaled, lw, lb, vbf=False):
    E, n = H * D, len(offs)
    off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV)
    ws = torch.empty(h.cls_attn_workspace_bytes(max(lens), n, H, D, SEGS, RATIOS), dtype=torch.uint8, device=DEV)
    out = torch.full((n, E), float("nan"), dtype=dq.dtype, device=DEV)
    h.cls_attn_merge_ln(dq, dq[:, E:], dq[:, 2 * E:], 3 * E, off, ln, max(lens), H, D, SEGS, RATIOS, lw.to(DEV),
                        lb.to(DEV), 1e-5, out, ws, 0.0, prescaled, v_bf16=vbf)
    torch.cuda.synchronize()
    return out.float().cpu()


def _run_pair(h, dq, L, D, prescaled, lw, lb, vbf=False):
    """The existing entry points restricted to token 0: windowed attention + windowed merge."""
    E = H * D
    outs, lses = [], []
    for sl, r in zip(SEGS, RATIOS):
        geo = orc.branch_geometry(L, sl, r, H)
        outs.append(torch.zeros(geo["nseg"] * geo["m"] * H * D, dtype=dq.dtype, device=DEV))
        lses.append(torch.zeros(geo["nseg"] * H * geo["m"], dtype=torch.float32, device=DEV))
    descs = [h.attn_branch(sl, r, dq[:, E:], dq[:, 2 * E:], 3 * E, 0, False, o, l)
             for sl, r, o, l in zip(SEGS, RATIOS, outs, lses)]
    h.dilated_attn_fwd_ex(dq, 3 * E, 0, 1, L, H, D, 0, 1, descs, 0.0, prescaled, v_bf16=vbf)
    out = torch.empty(1, E, dtype=dq.dtype, device=DEV)
    h.branch_merge_ln_window(outs, lses, SEGS, RATIOS, 1, L, 0, 1, H, D, lw.to(DEV), lb.to(DEV), 1e-5, out)
    torch.cuda.synchronize()
    return out.float().cpu()[0]


def _ulp(dt, ref):
    """One ulp of the output format at the largest reference magnitude."""
    bits = 7 if dt == torch.bfloat16 else 10
    return 2.0 ** (np.floor(np.log2(ref.abs().max().item())) - bits)


def _cos(a, b):
    a, b = a.double(), b.double()
    return float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()))


def _check_vs_pair(name, L, D, prescaled, fmt):
    h = _hip()
    qkv, lw, lb, ref = _case(L, D, prescaled)
    dq, vbf = _device_qkv(qkv, D, fmt)
    got = _run_cls(h, dq, [0], [L], D, prescaled, lw, lb, vbf)[0]
    pair = _run_pair(h, dq, L, D, prescaled, lw, lb, vbf)
    assert torch.isfinite(got).all()
    e_new, e_pair = (got - ref).abs().max().item(), (pair - ref).abs().max().item()
    bound = e_pair + _ulp(dq.dtype, ref)
    mx = ref.abs().max().item()
    print("%s L=%d D=%d %s: new %.3e pair %.3e bound %.3e" % (name, L, D, fmt, e_new, e_pair, bound))
    record_parity("cls kernel %s L=%d D=%d %s" % (name, L, D, fmt), "new", e_new / mx, _cos(got, ref), bound / mx, 0.0)
    record_parity("cls kernel %s L=%d D=%d %s" % (name, L, D, fmt), "pair", e_pair / mx, _cos(pair, ref), bound / mx, 0.0)
    assert e_new <= bound, (name, L, D, fmt, e_new, e_pair)


# L = 1025: s = 1025 is odd for r = 2 (m = 513, the last key is token 1024); 256 / 512: m_0 = 256 / m_1 = 256 and
# m_0 = 512, exactly on a key-chunk boundary; 513: m_0 = 513 and m_1 = 257, one past it
PRODUCT_LENGTHS = [1, 2, 17, 1025, 5793, 6001, CHUNK, 2 * CHUNK, 2 * CHUNK + 1]


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("L", PRODUCT_LENGTHS)
def test_cls_kernel_product_path(L, fmt):
    """D = 48 with q pre-scaled (the engine's layout), all three formats."""
    _check_vs_pair("prescaled", L, 48, True, fmt)


@pytest.mark.parametrize("D,fmt", [(48, "bf16"), (48, "fp16"), (64, "bf16"), (96, "bf16")])
def test_cls_kernel_plain_scale_and_head_dims(D, fmt):
    """softmax_scale = D^-1/2 applied by the kernel (q not pre-scaled): D = 48, and the other archs' 64 / 96."""
    _check_vs_pair("plain", 1025, D, False, fmt)


def test_cls_kernel_zero_query_single_token():
    """L = 1 with q = 0: every covered lse is log 1 = 0 -> -1e8 (dilated_attention.py:46), as the uncovered
    entries are, so the merge is the uniform average over all five branches, uncovered zeros included."""
    h = _hip()
    qkv, lw, lb, ref = _case(1, 48, True, zero_q=True)
    dq, _ = _device_qkv(qkv, 48, "bf16")
    got = _run_cls(h, dq, [0], [1], 48, True, lw, lb)[0]
    # (tests/test_gpu_kernels.py::test_branch_merge_vs_oracle's tolerance for merge + LN outputs)
    assert (got - ref).abs().max().item() <= 2 ** -7 * max(1.0, ref.abs().max().item())


def test_cls_kernel_three_slides_at_offsets():
    """Three slides of different lengths (one of them a single token) in one call, at non-zero offsets; the
    rows between the slides hold NaN, so a key read outside a slide shows."""
    h = _hip()
    lens, D = [300, 1, 1025], 48
    E = H * D
    offs, rows, refs, lw, lb = [], 3, [], None, None
    for L in lens:
        offs.append(rows)
        rows += L + 2
    buf = torch.full((rows, 3 * E), float("nan"), dtype=torch.bfloat16)
    for off, L in zip(offs, lens):
        qkv, lw_, lb_, _ = _case(L, D, True)
        lw, lb = (lw_, lb_) if lw is None else (lw, lb)
        buf[off:off + L] = qkv.bfloat16()
        refs.append(_oracle_row0(qkv, L, D, LN2, lw, lb))
    got = _run_cls(h, buf.to(DEV), offs, lens, D, True, lw, lb)
    for i, ref in enumerate(refs):
        assert (got[i] - ref).abs().max().item() <= 2 ** -7 * max(1.0, ref.abs().max().item()), (i, lens[i])


# ------------------------------------------------------------------ model
@pytest.fixture(scope="module")
def model():
    from gigapath import slide_encoder
    m = slide_encoder.create_model("", "gigapath_slide_enc12l768d", 1536)
    W = orc.make_weights(CFG, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    return m.to(DEV).eval()


_ORACLE = {}


def _oracle_forward(N, B=1, all_layer_embed=True):
    key = (N, B, all_layer_embed)
    if key not in _ORACLE:
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        Wt = {k: torch.from_numpy(v) for k, v in orc.make_weights(CFG, seed=0).items()}
        x, coords = orc.synthetic_slide(N, B=B)
        with torch.no_grad():
            _ORACLE[key] = torch.stack(orc.slide_encoder_forward(Wt, x, coords, CFG,
                                                                 all_layer_embed=all_layer_embed)).numpy()
    return _ORACLE[key]


def _with_tail(model, monkeypatch, on, fn):
    """fn() with runtime.CLS_TAIL = on and a fresh engine state (no workspace or graph of the other setting)."""
    from gigapath import runtime
    eng = model.encoder.engine
    monkeypatch.setattr(runtime, "CLS_TAIL", on)
    for t in (eng._ws, eng._pws):
        t.clear()
    try:
        with torch.no_grad():
            return fn()
    finally:
        for t in (eng._ws, eng._pws):
            t.clear()


def _ref_dev(golden_meta, N, B):
    """(the reference's own bf16-vs-fp32 deviation at this size, whether it is a tiny-slide case)."""
    for e in golden_meta["tiny"]["cases"]:
        if e["N"] == N and e["B"] == B:
            return e["ref_bf16_rel_vec_max"], True
    for e in golden_meta["e2e"]:
        if e["N"] == N and e["B"] == B:
            return e.get("ref_bf16_rel_inf", 0.0), False
    return 0.0, False


def _check_last(golden_meta, test, got, ref, N, B):
    """The check tests/test_gpu_model.py applies at this size (check_tiny for its tiny slides, else
    check_vectors with the reference's own bf16 deviation), on the last embedding [B, E]."""
    dev, tiny = _ref_dev(golden_meta, N, B)
    if tiny:
        check_tiny(test, got, ref, dev)
    else:
        check_vectors(test, "last_embed", got, ref, dev)


@pytest.mark.parametrize("N,B", [(1, 1), (600, 2), (1024, 1), (4097, 1)])
def test_tail_on_off_all_layer_embed(model, golden_meta, monkeypatch, N, B):
    x, coords = orc.synthetic_slide(N, B=B)
    xt, ct = torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV)
    run = lambda: torch.stack(model(xt, ct, all_layer_embed=True)).cpu().numpy()   # noqa: E731
    on = _with_tail(model, monkeypatch, True, run)
    off = _with_tail(model, monkeypatch, False, run)
    depth = CFG["depth"]
    assert on.shape == off.shape == (depth + 1, B, 768)
    assert np.array_equal(on[:depth], off[:depth])
    ref = _oracle_forward(N, B)
    for name, got in (("tail on", on), ("tail off", off)):
        _check_last(golden_meta, "cls tail N=%d B=%d %s" % (N, B, name), got[depth], ref[depth], N, B)


def test_tail_is_taken_and_skipped(model, monkeypatch):
    """The tail runs exactly when the readout is the CLS row: ClsRows buffers exist after a CLS forward with
    the tail on, not with it off or under global_pool."""
    x, coords = orc.synthetic_slide(300)
    xt, ct = torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV)
    eng = model.encoder.engine

    def probe():
        model(xt, ct, all_layer_embed=True)
        return eng.ws.cls is not None

    assert _with_tail(model, monkeypatch, True, probe)
    assert not _with_tail(model, monkeypatch, False, probe)
    model.global_pool = True
    try:
        assert not _with_tail(model, monkeypatch, True, probe)
    finally:
        model.global_pool = False


def test_tail_on_off_final_output_only(model, golden_meta, monkeypatch):
    """all_layer_embed=False: encoder.layer_norm + norm of the CLS rows read the tail's rows."""
    N = 1024
    x, coords = orc.synthetic_slide(N)
    xt, ct = torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV)
    run = lambda: torch.stack(model(xt, ct)).cpu().numpy()   # noqa: E731
    on = _with_tail(model, monkeypatch, True, run)
    off = _with_tail(model, monkeypatch, False, run)
    ref = _oracle_forward(N, 1, all_layer_embed=False)
    for name, got in (("tail on", on), ("tail off", off)):
        _check_last(golden_meta, "cls tail final-only N=%d %s" % (N, name), got[0], ref[0], N, 1)


def test_tail_on_off_forward_packed(model, golden_meta, monkeypatch):
    sizes = [1, 1023, 1024, 300]
    slides = []
    for n in sizes:
        x, c = orc.synthetic_slide(n)
        slides.append((torch.from_numpy(x[0]).to(DEV), torch.from_numpy(c[0]).to(DEV)))
    run = lambda: [torch.stack(o).cpu().numpy() for o in model.forward_packed(slides, all_layer_embed=True)]  # noqa: E731
    on = _with_tail(model, monkeypatch, True, run)
    off = _with_tail(model, monkeypatch, False, run)
    depth = CFG["depth"]
    for i, n in enumerate(sizes):
        assert np.array_equal(on[i][:depth], off[i][:depth]), n
        ref = _oracle_forward(n)
        for name, got in (("tail on", on[i]), ("tail off", off[i])):
            _check_last(golden_meta, "cls tail packed N=%d %s" % (n, name), got[depth], ref[depth], n, 1)


def test_global_pool_does_not_take_the_tail(model, monkeypatch):
    x, coords = orc.synthetic_slide(600, B=2)
    xt, ct = torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV)
    model.global_pool = True
    try:
        run = lambda: torch.stack(model(xt, ct, all_layer_embed=True) + model(xt, ct))   # noqa: E731
        on = _with_tail(model, monkeypatch, True, run)
        off = _with_tail(model, monkeypatch, False, run)
    finally:
        model.global_pool = False
    assert torch.equal(on, off)


def test_tail_graph_replay_matches_eager(model, monkeypatch):
    """The tail inside a captured HIP graph (plain and packed forward) replays bit-identically to eager."""
    x, coords = orc.synthetic_slide(1024)
    xt, ct = torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV)
    slides = []
    for n in (1, 300, 1025):
        xs, cs = orc.synthetic_slide(n)
        slides.append((torch.from_numpy(xs[0]).to(DEV), torch.from_numpy(cs[0]).to(DEV)))

    def run():
        plain = torch.stack(model(xt, ct, all_layer_embed=True))
        packed = torch.stack([torch.stack(o) for o in model.forward_packed(slides, all_layer_embed=True)])
        return plain, packed

    eager = _with_tail(model, monkeypatch, True, run)
    model.use_hip_graphs, model.graph_min_uses = True, 1
    try:
        reps = [_with_tail(model, monkeypatch, True, run) for _ in range(2)]
        assert len(model._graphs) == 2
    finally:
        model.use_hip_graphs, model.graph_min_uses = False, 2
        for k in list(model._graphs):
            model._drop_graph(k)
        model._graph_seen.clear()
    for rep in reps:
        assert torch.equal(rep[0], eager[0]) and torch.equal(rep[1], eager[1])
