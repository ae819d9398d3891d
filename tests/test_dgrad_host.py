"""gp_linear_dgrad without a GPU: its argument errors are rejected on the host before any launch, and
runtime.linear_grad with the dgrad switch on leaves CPU tensors to F.linear."""
import pytest
import torch
import torch.nn.functional as F

from test_attn_bwd_host import FAKE


@pytest.mark.parametrize("kw,msg", [
    ({"N": 320}, b"N=320 must be a positive multiple of 256"),
    ({"K": 800}, b"K=800 must be a positive multiple of 256"),
    ({"M": 0}, b"M=0 outside [1, 2^31)"),
    ({"fmt": 7}, b"bad fmt 7"),
    ({"ldy": 772}, b"bad leading dimensions"),
], ids=lambda v: "-".join(v) if isinstance(v, dict) else None)
def test_argument_errors_are_rejected_on_the_host(kw, msg):
    from test_abi_and_api import _lib_path
    _lib_path()
    from gigapath import _hip
    lib = _hip.load_library()
    a = {**dict(dy=FAKE, w=2 * FAKE, dx=3 * FAKE, M=300, N=768, K=768, fmt=0), **kw}
    rc = lib.gp_linear_dgrad(a["dy"], a.get("ldy", a["N"]), a["w"], a["K"], a["dx"], a["K"], a["M"], a["N"], a["K"],
                             a["fmt"], None)
    assert rc == -1 and msg in lib.gp_last_error_string()


def test_switch_is_set_per_module_and_by_enable_training():
    from gigapath import _hip, runtime, slide_encoder
    from gigapath.torchscale.component.feedforward_network import FeedForwardNetwork
    box = torch.nn.Sequential(FeedForwardNetwork(256, 512))
    assert runtime.dgrad_enabled(box[0]) == runtime.TRAIN_DGRAD
    for flag in (True, False):
        slide_encoder.LongNetViT.enable_training(box, True, native_dgrad=flag)
        assert runtime.dgrad_enabled(box[0]) == flag and box[0].native_wgrad is None
    assert _hip.linear_dgrad_supported(70001, 3072, 1024) and not _hip.linear_dgrad_supported(64, 320, 1024)
    assert not any(_hip.linear_dgrad_supported(70001, *nk) for nk in _hip.DGRAD_TORCH_FASTER)   # left to torch


@pytest.mark.parametrize("wgrad", [False, True])
def test_linear_grad_on_cpu_is_f_linear(wgrad):
    from gigapath import runtime
    g = torch.Generator().manual_seed(0)
    x0, gy = torch.randn(5, 256, generator=g).bfloat16(), torch.randn(5, 512, generator=g).bfloat16()
    w0, b0 = torch.randn(512, 256, generator=g) * 0.05, torch.randn(512, generator=g)
    outs = []
    for native in (True, False):
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        y = runtime.linear_grad(x, [(w, b, 1.0)], wgrad=wgrad, dgrad=True) if native else \
            F.linear(x, w.bfloat16(), b.bfloat16())
        y.backward(gy)
        outs.append((y.detach(), x.grad, w.grad, b.grad))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
