"""The native weight gradients behind the training path (run with -m gpu): runtime.linear_grad against the same call
through F.linear autograd, and one EncoderLayer with the switch on against the format model.

Function: the output and dX in bits; dW / db per part within test_gpu_wgrad's bound of fp64 and no further from it
than the torch arm (which rounds dW to 16 bits once more).  Layer: the limit of test_gpu_train.py, e <= 2 e_model per
gradient, and the switch-off output in bits."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_train as tgt
from gigapath import runtime
from test_gpu_wgrad import _worst_ratio

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_linear_grad_function(dtype):
    M, E, qs = 257, 768, (48 ** -0.5) * runtime.LOG2E
    g = torch.Generator(device="cuda").manual_seed(3)
    x0 = torch.randn(M, E, generator=g, device="cuda").to(dtype)
    gy = torch.randn(M, 3 * E, generator=g, device="cuda").to(dtype)
    scales = (qs, 1.0, 1.0)
    leaves = [(torch.randn(E, E, generator=g, device="cuda") * 0.03, torch.randn(E, generator=g, device="cuda"))
              for _ in scales]

    def arm(native):
        x = x0.clone().requires_grad_(True)
        parts = [(w.clone().requires_grad_(True), b.clone().requires_grad_(True), s)
                 for (w, b), s in zip(leaves, scales)]
        if native:
            y = runtime.linear_grad(x, parts)
        else:
            y = F.linear(x, torch.cat([w * s for w, _, s in parts], 0).to(dtype),
                         torch.cat([b * s for _, b, s in parts], 0).to(dtype))
        y.backward(gy)
        return y.detach(), x.grad, [(w.grad, b.grad) for w, b, _ in parts]

    y, dx, grads = arm(True)
    yt, dxt, grads_t = arm(False)
    assert torch.equal(y, yt) and torch.equal(dx, dxt)
    g64, x64 = gy.double(), x0.double()
    ref_w, mag_w = g64.t() @ x64, g64.abs().t() @ x64.abs()
    ref_b, mag_b = g64.sum(0), g64.abs().sum(0)
    for i, s in enumerate(scales):
        rows = slice(i * E, (i + 1) * E)
        for nm, got, got_t, ref, mag in (("dW", grads[i][0], grads_t[i][0], ref_w[rows] * s, mag_w[rows] * s),
                                         ("db", grads[i][1], grads_t[i][1], ref_b[rows] * s, mag_b[rows] * s)):
            assert got.dtype == torch.float32
            ratio = _worst_ratio(got, ref, mag, M)
            e, et = float((got.double() - ref).abs().max()), float((got_t.double() - ref).abs().max())
            print("linear_grad %s part %d %s: worst |err| / bound %.3f  e %.3e  e_torch %.3e" % (dtype, i, nm, ratio, e, et))
            assert ratio <= 1.0 and e <= et, (i, nm, ratio, e, et)


@pytest.fixture(scope="module")
def layer_refs():
    return {fmt: tgt._layer_reference(1, 1500, dt) for fmt, dt in (("fp32", None),) + tuple(tgt.DTYPES.items())}


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_encoder_layer_with_native_wgrad(fmt, layer_refs):
    x, gy = tgt._layer_inputs(1, 1500)

    def run(native):
        layer = tgt._layer()
        layer.self_attn.native_wgrad = layer.ffn.native_wgrad = native
        xd = x.to(tgt.DEV).requires_grad_(True)
        with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
            y = layer(xd)[0]
        y.backward(gy.to(tgt.DEV))
        got = {"dx": xd.grad.double().cpu().numpy()}
        for k, p in layer.named_parameters():
            assert p.grad is not None and p.grad.dtype == p.dtype, k
            got[k] = p.grad.double().cpu().numpy()
        return y.detach(), got

    y_off, _ = run(False)
    y_on, got = run(True)
    assert torch.equal(y_on, y_off)
    tgt.check_gradients("wgrad %s 1x1500" % fmt, got, layer_refs["fp32"], layer_refs[fmt])
