"""gp_dilated_attn_bwd2_varlen on the MI355X (run with -m gpu): the packed attention backward at H = 16, D = 64, bf16,
q pre-scaled (q' = q D^-0.5 log2 e), after the packed D = 64 forward and the merge without LN.

Parity is test_gpu_dilated_bwd's rule per slide: e_kernel <= 2 e_model per gradient against the fp32 restatement
(test_dilated_bwd_host.dilated_core) differentiated with respect to q', exact zeros where the reference is identically
zero.  Its _parity runs unchanged; its _kernel is replaced by the slide's rows of the packed result.  The packed D = 64
forward is not the dense forward's bits, so no bit equality with gp_dilated_attn_bwd is asked.  The packs:
  A  SCHED_A, [200, 5, 31, 1, 333]: a single key, s % r != 0 with zero-pad rows, slides whose tail row is the next CLS
  B  SCHED_B, [1500, 257, 1, 700, 130]: a tail inside a 64-row tile, several 256-row own blocks, blocks partly past nq
Measured ratios: DESIGN §3.19.
"""
import functools
from functools import partial

import numpy as np
import pytest
import torch

import oracle as orc
import test_dilated_bwd_host as host
import test_gpu_dilated_bwd as tgd
import test_train_host as th
from test_gpu_model import close_enough
from test_gpu_train_packed import _grads, _slides

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, D, E = 16, 64, 1024
QS = D ** -0.5 * host.LOG2E
PACKS = {"A": (host.SCHED_A, [200, 5, 31, 1, 333]), "B": (host.SCHED_B, [1500, 257, 1, 700, 130])}
SENTINEL = -1024.0


@functools.lru_cache(maxsize=None)
def _inputs(pack, qk_scale=1.0):
    """Per slide test_gpu_dilated_bwd's draws (q, k, v [1, L, H, D], dm [1, L, E] bf16 on the CPU)."""
    return [tgd._inputs(6400 + 10 * i + L, 1, L, D, torch.bfloat16, qk_scale=qk_scale, q_scale=QS)
            for i, L in enumerate(PACKS[pack][1])]


def _pack(slides):
    qkv = torch.cat([torch.cat([t.reshape(-1, E) for t in s[:3]], 1) for s in slides], 0).to(DEV).contiguous()
    return qkv, torch.cat([s[3].reshape(-1, E) for s in slides], 0).to(DEV).contiguous()


def _packed(qkv, dm, pack):
    """The packed forward, the merge and gp_dilated_attn_bwd2_varlen -> (dqkv [T, 3E], the guard rows around it)."""
    from gigapath import _hip as h, runtime
    (segs, ratios), Ls = PACKS[pack]
    vs = runtime.VarlenScratch(torch.device(DEV), Ls, H, D, segs, ratios, qkv)
    for t in vs.outs + vs.lses:
        t.zero_()
    h.dilated_attn_fwd_varlen(vs.plan, True)
    h.branch_merge_ln_varlen(vs.plan, None, None, 0.0, torch.empty(sum(Ls), E, dtype=qkv.dtype, device=DEV))
    buf = torch.full((sum(Ls) + 2, 3 * E), SENTINEL, dtype=qkv.dtype, device=DEV)
    dqkv = buf[1:-1]
    plan = h.VarlenBwd2Plan(Ls, H, D, segs, ratios).bind(qkv, vs.outs, vs.lses)
    h.dilated_attn_bwd2_varlen(plan, dm, dqkv, dqkv[:, E:], dqkv[:, 2 * E:], 3 * E)
    torch.cuda.synchronize()
    return dqkv.clone(), torch.cat([buf[0], buf[-1]])


@functools.lru_cache(maxsize=None)
def _baseline(pack):
    return _packed(*_pack(_inputs(pack)), pack)


def _check_parity(name, pack, slides, dqkv, monkeypatch):
    t0 = 0
    for (q, k, v, dm), L in zip(slides, PACKS[pack][1]):
        rows = dqkv[t0:t0 + L].cpu()
        got = tuple(rows[:, j * E:(j + 1) * E].reshape(1, L, H, D) for j in range(3))
        monkeypatch.setattr(tgd, "_kernel", lambda *a, **kw: got)
        tgd._parity("varlen bwd2 d64 %s L%d" % (name, L), q, k, v, dm, *PACKS[pack][0], prescaled=True)
        t0 += L


@pytest.mark.parametrize("pack", list(PACKS))
def test_parity_per_slide(pack, monkeypatch):
    dqkv, guards = _baseline(pack)
    assert (guards.float() == SENTINEL).all()
    _check_parity(pack, pack, _inputs(pack), dqkv, monkeypatch)


def test_parity_sharp_softmax(monkeypatch):
    """q, k scaled x4: sharp, near one-hot P."""
    slides = _inputs("B", 4.0)
    _check_parity("B sharp", "B", slides, _packed(*_pack(slides), "B")[0], monkeypatch)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("case", ["zero", "twice", "guards", "nan_neighbours", "inf"])
def test_exact_cases(case):
    pack = "B" if case == "twice" else "A"
    Ls = PACKS[pack][1]
    off = np.concatenate([[0], np.cumsum(Ls)]).tolist()
    qkv, dm = _pack(_inputs(pack))
    base, guards = _baseline(pack)
    if case == "zero":                      # dmerged = 0 gives zeros
        assert (_packed(qkv, torch.zeros_like(dm), pack)[0] == 0).all()
    elif case == "twice":                   # no atomics, no inter-workgroup waits: equal bits
        assert torch.equal(_bits(_packed(qkv, dm, pack)[0]), _bits(base))
    elif case == "guards":                  # the rows around dqkv survive, every row between them is written
        assert (guards.float() == SENTINEL).all()
        assert torch.isfinite(base.float()).all() and (base.float() != SENTINEL).all()
    elif case == "nan_neighbours":          # every other slide's qkv and dmerged NaN: the slide keeps its bits
        for i in range(len(Ls)):
            q2, d2 = torch.full_like(qkv, float("nan")), torch.full_like(dm, float("nan"))
            q2[off[i]:off[i + 1]], d2[off[i]:off[i + 1]] = qkv[off[i]:off[i + 1]], dm[off[i]:off[i + 1]]
            got, g2 = _packed(q2, d2, pack)
            assert torch.equal(_bits(got[off[i]:off[i + 1]]), _bits(base[off[i]:off[i + 1]])), Ls[i]
            assert (g2.float() == SENTINEL).all()
    else:                                   # a +Inf in one slide's dmerged stays in that slide
        hit = 2                             # the 31-token slide
        d2 = dm.clone()
        d2[off[hit] + 17, 5 * D + 3] = float("inf")
        got, _ = _packed(qkv, d2, pack)
        for i in range(len(Ls)):
            rows = slice(off[i], off[i + 1])
            if i == hit:
                assert all(not torch.isfinite(got[rows, j * E:(j + 1) * E].float()).all() for j in range(3))
            else:
                assert torch.equal(_bits(got[rows]), _bits(base[rows])), Ls[i]


# ----------------------------------------------------------------------------------------------
# the 24L1024d arch cut to depth 2 (as test_gpu_varlen_d64 builds it): packed training with the switch on
# ----------------------------------------------------------------------------------------------
TILES = [300, 1, 1100]
CFG = dict(orc.arch_config("gigapath_slide_enc24l1024d"), depth=2)


def _model_reference(dt):
    """test_gpu_train_packed._model_reference for this arch: train_model per slide on the CPU -> parameter gradients."""
    W = th.leaf_weights(CFG)
    loss = 0
    for i, n in enumerate(TILES):
        x, c = orc.synthetic_slide(n, seed_x=40 + i, seed_c=90 + i)
        loss = loss + th.weighted_loss(th.train_model(W, torch.from_numpy(x), c, CFG, dt))
    loss.backward()
    return {k: t.grad.double().numpy() for k, t in W.items() if t.grad is not None}


def test_forward_packed_trains_the_24l1024d_arch(monkeypatch):
    """enable_training(native_attn_bwd2=True) + forward_packed against the same slides through forward() one at a time
    with the switch off: outputs by close_enough, parameter gradients within 4 e_model (test_gpu_train_packed's rule);
    the packed forward and the new backward launch once per layer."""
    from gigapath import _hip as hip, slide_encoder
    from gigapath.torchscale.model import LongNetConfig
    monkeypatch.setitem(LongNetConfig.CONFIGS, "LongNet_2_layers_1024_dim", LongNetConfig._cfg(2, 1024))
    model = slide_encoder.LongNetViT(in_chans=1536, embed_dim=1024, depth=2, mlp_ratio=4, dropout=0.0,
                                     drop_path_rate=0.0, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_weights(CFG, seed=0).items()}, strict=True)
    model = model.to(DEV).enable_training(native_attn_bwd2=True).train()
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = hip.dilated_attn_fwd_varlen, hip.dilated_attn_bwd2_varlen
    count = lambda nm, fn: lambda *a, **k: (calls.__setitem__(nm, calls[nm] + 1), fn(*a, **k))[1]   # noqa: E731
    monkeypatch.setattr(hip, "dilated_attn_fwd_varlen", count("fwd", fwd))
    monkeypatch.setattr(hip, "dilated_attn_bwd2_varlen", count("bwd", bwd))
    slides = _slides(TILES)
    packed = model.forward_packed(slides, all_layer_embed=True)
    assert all(t.shape == (1, E) and t.grad_fn is not None for o in packed for t in o)
    sum(th.weighted_loss(o) for o in packed).backward()
    assert calls == {"fwd": 2, "bwd": 2}
    gp = _grads(model)
    model.enable_training(native_attn_bwd2=False)
    for p in model.parameters():
        p.grad = None
    seq = []
    for x, c in slides:
        outs = model(x[None], c[None], all_layer_embed=True)
        th.weighted_loss(outs).backward()
        seq.append([o.detach() for o in outs])
    gs = _grads(model)
    assert calls == {"fwd": 2, "bwd": 2}
    for i in range(3):
        for k in range(3):
            rel, cos, ok = close_enough(packed[i][k].detach().cpu().numpy(), seq[i][k].cpu().numpy())
            assert ok, (i, k, rel, cos)
    ref, mod = _model_reference(None), _model_reference(torch.bfloat16)
    assert set(gp) == set(gs) and len(gp) > 30
    worst = 0.0
    for k in sorted(gp):
        d = np.abs(gp[k] - gs[k]).max()
        lim = 4 * (np.abs(mod[k]).max() if k.endswith("k_proj.bias") else np.abs(mod[k] - ref[k]).max())
        worst = max(worst, d / lim if lim else (0.0 if d == 0 else float("inf")))
        assert d <= lim, (k, d, lim)
    print("24l1024d depth 2 worst |packed - sequential| / (4 e_model): %.3f" % worst)
