"""The native data gradient behind the training path (-m gpu), dgrad on and wgrad on or off.  Function (1024 wide):
the output of F.linear in bits; dX within test_gpu_dgrad's bound of fp64 and no further from it than torch's (x 1.05:
summation order alone); dW / db within test_gpu_wgrad's bound (wgrad off: within one 16-bit rounding).  Layer (768 wide,
_hip.DGRAD_TORCH_FASTER emptied): the switch-off output in bits, e <= 2 e_model, one kernel call per projection."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_train as tgt
from gigapath import _hip, runtime
from test_gpu_dgrad import ULP
from test_gpu_gemm import _elem_ratio
from test_gpu_wgrad import _worst_ratio

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wgrad", [True, False], ids=["wgrad", "torch-wgrad"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_linear_grad_function(dtype, wgrad):
    M, E, scales = 257, 1024, ((64 ** -0.5) * runtime.LOG2E, 1.0, 1.0)
    assert _hip.linear_dgrad_supported(M, 3 * E, E)
    g = torch.Generator(device="cuda").manual_seed(3)
    x0, gy = (torch.randn(M, c, generator=g, device="cuda").to(dtype) for c in (E, 3 * E))
    leaves = [(torch.randn(E, E, generator=g, device="cuda") * 0.03, torch.randn(E, generator=g, device="cuda"))
              for _ in scales]
    w_act = torch.cat([w * s for (w, _), s in zip(leaves, scales)], 0).to(dtype)
    b_act = torch.cat([b * s for (_, b), s in zip(leaves, scales)], 0).to(dtype)

    x = x0.clone().requires_grad_(True)
    parts = [(w.clone().requires_grad_(True), b.clone().requires_grad_(True), s) for (w, b), s in zip(leaves, scales)]
    y = runtime.linear_grad(x, parts, wgrad=wgrad, dgrad=True)
    y.backward(gy)
    xt = x0.clone().requires_grad_(True)
    yt = F.linear(xt, w_act, b_act)
    yt.backward(gy)
    assert torch.equal(y, yt)
    g64, x64, w64 = gy.double(), x0.double(), w_act.double()
    ref_x = g64 @ w64
    ratio = _elem_ratio(x.grad, ref_x, g64.abs() @ w64.abs(), ULP[dtype], 3 * E)
    e, et = float((x.grad.double() - ref_x).abs().max()), float((xt.grad.double() - ref_x).abs().max())
    print("linear_grad %s dX: worst |err| / bound %.3f  e %.3e  e_torch %.3e" % (dtype, ratio, e, et))
    assert ratio <= 1.0 and e <= 1.05 * et, (ratio, e, et)
    ref_w, mag_w = g64.t() @ x64, g64.abs().t() @ x64.abs()
    ref_b, mag_b = g64.sum(0), g64.abs().sum(0)
    for i, (w, b, s) in enumerate(parts):
        rows = slice(i * E, (i + 1) * E)
        for nm, got, ref, mag in (("dW", w.grad, ref_w[rows] * s, mag_w[rows] * s),
                                  ("db", b.grad, ref_b[rows] * s, mag_b[rows] * s)):
            r = _worst_ratio(got, ref, mag, M) if wgrad else _elem_ratio(got, ref, mag, ULP[dtype], M)
            print("linear_grad %s part %d %s: worst |err| / bound %.3f" % (dtype, i, nm, r))
            assert r <= 1.0, (i, nm, r)


@pytest.fixture(scope="module")
def layer_refs():
    return {fmt: tgt._layer_reference(1, 1500, dt) for fmt, dt in (("fp32", None),) + tuple(tgt.DTYPES.items())}


@pytest.mark.parametrize("wgrad", [True, False], ids=["wgrad", "torch-wgrad"])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_encoder_layer_with_native_dgrad(fmt, wgrad, layer_refs, monkeypatch):
    monkeypatch.setattr(_hip, "DGRAD_TORCH_FASTER", frozenset())     # the kernel serves the 768-wide layer too
    assert all(_hip.linear_dgrad_supported(1500, n, k) for n, k in ((2304, 768), (768, 768), (3072, 768), (768, 3072)))
    calls, kernel = [], _hip.linear_dgrad
    monkeypatch.setattr(_hip, "linear_dgrad", lambda dy, w: calls.append(tuple(w.shape)) or kernel(dy, w))
    x, gy = tgt._layer_inputs(1, 1500)

    def run(wg, dg):
        layer = tgt._layer()
        for m in (layer.self_attn, layer.ffn):
            m.native_wgrad, m.native_dgrad = wg, dg
        xd = x.to(tgt.DEV).requires_grad_(True)
        with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
            y = layer(xd)[0]
        y.backward(gy.to(tgt.DEV))
        got = {k: p.grad.double().cpu().numpy() for k, p in layer.named_parameters()}
        got["dx"] = xd.grad.double().cpu().numpy()
        return y.detach(), got

    y_off = run(False, False)[0]
    y_on, got = run(wgrad, True)
    assert sorted(calls) == [(768, 768), (768, 3072), (2304, 768), (3072, 768)]   # fc2, out-proj, QKV, fc1
    assert torch.equal(y_on, y_off)
    tgt.check_gradients("dgrad %s 1x1500" % fmt, got, layer_refs["fp32"], layer_refs[fmt])
