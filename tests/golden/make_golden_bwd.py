"""Generate tests/golden/dilated_attention_bwd.npz by backpropagating through the REFERENCE's own
DilatedAttention (fp32, the harness's fp32 attention at the flash_attn_func seam).

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_bwd.py
The output is data: a seeded upstream gradient and the gradients the reference's autograd returns for the
module, weights, x, segs and ratios of dilated_attention_custom.npz.  The harness's attention restatement is
differentiable as written (its slice assignments are recorded by autograd); the LSEs reach the output only
through scattering's torch.no_grad() block, so they carry no gradient.

To keep the file under 1 MB, gy is drawn from PCG64(11), rounded to fp16 and stored as fp16 (it is used as
those exact values), and dx is stored for the token rows listed in dx_rows (every fourth row and the last
three; every row of dx depends on every branch and segment of its batch element).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # repo root (for oracle)
sys.path.insert(0, HERE)

import ref_harness  # noqa: E402
import oracle as orc  # noqa: E402
from make_golden import make_dilated_module  # noqa: E402

PRE = "encoder.layers.0.self_attn."
PARAMS = ("q_proj.bias", "k_proj.bias", "v_proj.bias", "out_proj.bias", "inner_attn_ln.weight", "inner_attn_ln.bias")


def main():
    _, da, cfgmod = ref_harness.load_reference()
    g = np.load(os.path.join(HERE, "dilated_attention_custom.npz"))
    segs, ratios = [int(s) for s in g["segs"]], [int(r) for r in g["ratios"]]
    cfg = orc.arch_config("gigapath_slide_enc12l768d")
    mod = make_dilated_module(da, cfgmod, 768, 16, segs, ratios)
    W = orc.make_weights(cfg, seed=0, perturb=True)
    mod.load_state_dict({k[len(PRE):]: torch.from_numpy(v) for k, v in W.items() if k.startswith(PRE)}, strict=True)

    x = torch.from_numpy(g["x"]).requires_grad_(True)
    gy16 = np.random.Generator(np.random.PCG64(11)).standard_normal(g["y"].shape).astype(np.float16)
    y = mod(x, x, x)[0]
    assert np.abs(y.detach().numpy() - g["y"]).max() <= 2e-5 * np.abs(g["y"]).max()   # the forward golden's module
    y.backward(torch.from_numpy(gy16.astype(np.float32)))

    L = x.shape[1]
    rows = np.unique(np.concatenate([np.arange(0, L, 4), np.arange(L - 3, L)])).astype(np.int64)
    out = {"gy": gy16, "dx_rows": rows, "dx": x.grad.numpy()[:, rows]}
    params = dict(mod.named_parameters())
    for name in PARAMS:
        out["d_" + name] = params[name].grad.numpy()
    path = os.path.join(HERE, "dilated_attention_bwd.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
