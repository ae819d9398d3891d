"""gp_dilated_attn_bwd2 on the MI355X (run with -m gpu): test_gpu_dilated_bwd's checks with the second backward as the
kernel.  Its _kernel / _parity run unchanged; the `bwd2` fixture routes their _hip.dilated_attn_bwd call to
_hip.dilated_attn_bwd2, so the limit is the same rule: e_kernel <= 2 e_model per gradient against the fp32 reference,
exact zeros where the reference is identically zero.  q is pre-scaled (q' = q D^-0.5 log2 e, the reference
differentiated with respect to q').  Measured ratios: DESIGN §3.18."""
import pytest
import torch

import test_dilated_bwd_host as host
import test_gpu_dilated_bwd as tgd
import test_gpu_train as tgt
from test_gpu_dilated_bwd import DTYPES, SCHEDS, SENTINEL, _inputs

pytestmark = pytest.mark.gpu
D = 48
QS = D ** -0.5 * host.LOG2E
# a single key; s % r != 0 with zero-pad queries and keys; several segments and a tail segment; a tail inside a 64-row
# tile; more than one 256-row own block (L = 1500: branch 0's segments of 256, branch 1 with m = 256) and own blocks
# partly past nq
SHAPES = [("A", 2, 1), ("A", 2, 5), ("A", 2, 31), ("A", 2, 200), ("B", 2, 257), ("B", 1, 1500)]


@pytest.fixture
def bwd2(monkeypatch):
    from gigapath import _hip
    _hip.load_library()
    monkeypatch.setattr(_hip, "dilated_attn_bwd", _hip.dilated_attn_bwd2)


def _kernel2(q, k, v, dm, sched, **kw):
    return tgd._kernel(q, k, v, dm, *SCHEDS[sched], prescaled=True, **kw)


@pytest.mark.parametrize("sched,B,L", SHAPES)
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd2_parity(bwd2, fmt, sched, B, L):
    """test_bwd_parity's own draws (its seed), with q pre-scaled."""
    q, k, v, dm = _inputs(1000 * D + L, B, L, D, DTYPES[fmt], q_scale=QS)
    tgd._parity("bwd2 %s %s B%d L%d" % (fmt, sched, B, L), q, k, v, dm, *SCHEDS[sched], prescaled=True)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd2_parity_sharp_softmax(bwd2, fmt):
    """q, k scaled x4: sharp, near one-hot P."""
    q, k, v, dm = _inputs(7, 2, 257, D, DTYPES[fmt], qk_scale=4.0, q_scale=QS)
    tgd._parity("bwd2 %s sharp B L257" % fmt, q, k, v, dm, *SCHEDS["B"], prescaled=True)


@pytest.mark.parametrize("case", ["zero", "twice", "guards", "nan_fill", "inf"])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_bwd2_exact_cases(bwd2, fmt, case):
    sched, L = ("B", 1500) if case == "twice" else ("A", 200)
    q, k, v, dm = _inputs(21, 1 if case == "twice" else 2, L, D, DTYPES[fmt], q_scale=QS)
    if case == "zero":                      # dmerged = 0 gives zeros
        assert all((g == 0).all() for g in _kernel2(q, k, v, torch.zeros_like(dm), sched))
    elif case == "twice":                   # no atomics, no inter-workgroup waits: equal bits
        a, b = _kernel2(q, k, v, dm, sched), _kernel2(q, k, v, dm, sched)
        assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))
    elif case == "guards":                  # the rows around dqkv survive, every row between them is written
        grads, guards, _ = _kernel2(q, k, v, dm, sched, full=True)
        assert (guards.float() == SENTINEL).all()
        assert all(torch.isfinite(g.float()).all() and (g.float() != SENTINEL).all() for g in grads)
    elif case == "nan_fill":                # rows the forward leaves unwritten are not read
        assert all(torch.isfinite(g.float()).all() for g in _kernel2(q, k, v, dm, sched, nan_fill=True))
    else:                                   # a non-finite dmerged reaches dq, dk and dv
        dm[1, 77, 5 * D + 3] = float("inf")
        assert all(not torch.isfinite(g.float()).all() for g in _kernel2(q, k, v, dm, sched))


@pytest.fixture(scope="module")
def layer_refs():
    return {fmt: tgt._layer_reference(2, 257, dt) for fmt, dt in (("fp32", None),) + tuple(tgt.DTYPES.items())}


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_encoder_layer_with_native_attn_bwd2(fmt, layer_refs, monkeypatch):
    """One EncoderLayer (SCHED_B, dropout 0), the switch on against off: y in bits (the forward is untouched); each arm
    within its own bound 2 e_model of the fp32 model, so the arms within the sum of the two."""
    from gigapath import _hip
    calls, kernel = [], _hip.dilated_attn_bwd2
    monkeypatch.setattr(_hip, "dilated_attn_bwd2", lambda *a: calls.append(1) or kernel(*a))
    x, gy = tgt._layer_inputs(2, 257)

    def run(on):
        layer = tgt._layer()
        layer.self_attn.native_attn_bwd2 = on
        xd = x.to(tgt.DEV).requires_grad_(True)
        with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
            y = layer(xd)[0]
        y.backward(gy.to(tgt.DEV))
        got = {k: p.grad.double().cpu().numpy() for k, p in layer.named_parameters()}
        got["dx"] = xd.grad.double().cpu().numpy()
        return y.detach(), got

    y_off, got_off = run(False)
    assert not calls
    y_on, got_on = run(True)
    assert calls == [1] and torch.equal(y_on, y_off)
    tgt.check_gradients("bwd2 off %s" % fmt, got_off, layer_refs["fp32"], layer_refs[fmt])
    tgt.check_gradients("bwd2 on %s" % fmt, got_on, layer_refs["fp32"], layer_refs[fmt])
