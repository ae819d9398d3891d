"""Generate tests/golden/train_grads_N1300.npz by backpropagating through the REFERENCE's own slide encoder
(dropout 0, drop-path 0), twice: in fp32 with ref_harness as it stands (the harness's fp32 attention at the
flash_attn_func seam), and in fp64 (model.double(), fp64 inputs, an fp64 restatement of flash_attn_func bound at the
seam by this script after loading; nothing in the harness changes).

The fp32 run is the golden the GPU tests compare against (train_grads_N1300.npz, _w.npz).  The fp64 run is what the
fp32 restatement is pinned to: in fp32 the reference's own backward carries rounding of up to 3.6e-5 of max|ref|
(layer 5's d q_proj.weight: the q gradients of the middle layers are small differences of large terms), more than the
2e-5 the restatement is held to.  It is stored as a float16 correction to the fp32 run's arrays
(train_grads_N1300_f64.npz; test_train_host.load_train_golden(fp64=True) applies it).

Run in the build container only (needs the reference checkout):  python tests/golden/make_golden_train.py
The output is data: the loss, the reference outputs, and the gradients the reference's autograd returns for the
seeded weights and synthetic_slide(1300) -- the smallest slide whose first branch has two segments.  The loss is a
seeded, fp16-stored weighting of the 13 all_layer_embed outputs (tests/test_train_host.py: loss_weights).

To keep every file under 1 MB the 2-D weight rows go to a second file, train_grads_N1300_w.npz, and the golden
stores dx at every 16th tile, the cls_token / norm.* / patch_embed.proj.bias gradients, every 1-D parameter gradient
of layers 0, 5 and 11 and eight seeded rows of each of their 2-D weight gradients ("d:<name>", with "rows:<name>"
naming the rows), as float32.  Per stored gradient it also records the deviation of the format model
(test_train_host.train_model with a 16-bit dt) from the fp32 model, e_model = max|d| / max|fp32|, for bf16
("em_bf16:<key>") and fp16 ("em_f16:<key>"): the GPU test's tolerance is twice that.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "prov-gigapath-replication_amd"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_harness  # noqa: E402
import oracle as orc  # noqa: E402
import test_train_host as tth  # noqa: E402
from test_attn_bwd_host import attn_fp32  # noqa: E402

ARCH = "gigapath_slide_enc12l768d"


def flash_attn_fp64(q, k, v, dropout=0.0, bias=None, softmax_scale=None, is_causal=False):
    """flash_attn_func (torchscale/component/flash_attention.py:13-16) restated in the inputs' precision:
    q, k, v [B, L, H, D] -> (out [B, L, H, D], lse [B, H, L])."""
    assert bias is None and not is_causal and dropout == 0.0
    return attn_fp32(q, k, v, softmax_scale)


def reference_gradients(double=True):
    se, _, _ = ref_harness.load_reference()
    mha = sys.modules["torchscale.component.multihead_attention"]
    mha.flash_attn_func = flash_attn_fp64 if double else ref_harness.flash_attn_fp32
    cfg = orc.arch_config(ARCH)
    model = se.create_model("", ARCH, 1536, dropout=0.0, drop_path_rate=0.0)
    W = orc.make_weights(cfg, seed=0)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    assert not unexpected and all(k == "pos_embed" for k in missing), (missing, unexpected)
    model.eval()                                         # dropout 0 / drop-path 0: the mode changes nothing
    x_np, coords = orc.synthetic_slide(tth.GOLDEN_N)
    x = torch.from_numpy(np.asarray(x_np, dtype=np.float32))
    if double:
        model = model.double()
        x = x.double()
    x.requires_grad_(True)
    outs = model(x, torch.from_numpy(np.asarray(coords)), all_layer_embed=True)
    assert all(o.dtype == x.dtype for o in outs)
    loss = tth.weighted_loss(outs)
    loss.backward()
    res = {"loss": float(loss), "dx": x.grad.double().numpy(),
           "outs": torch.stack([o.detach() for o in outs]).double().numpy()}
    for k, p in model.named_parameters():
        if p.grad is not None:
            res[k] = p.grad.double().numpy()
    return res, {k: v.shape for k, v in W.items()}


def stored(ref, shapes):
    """What the golden keeps of a full set of gradients (see the module docstring), as float64."""
    out = {"outs": ref["outs"], "dx": ref["dx"][:, ::16]}
    for name, rows in tth.golden_selection(shapes).items():
        if rows is not None:
            out["rows:" + name] = rows.astype(np.int64)
        out["d:" + name] = ref[name] if rows is None else ref[name][rows]
    return out


def main():
    ref, shapes = reference_gradients(double=False)
    out = {k: (v if k.startswith("rows:") else v.astype(np.float32)) for k, v in stored(ref, shapes).items()}
    out["loss"] = np.float64(ref["loss"])
    # the fp64 run, as a correction to the fp32 run's arrays: (fp64 - fp32) / max|fp64 - fp32| in float16 (the
    # correction is <= 3.6e-5 of max|ref|, so its float16 rounding is below 2e-8 of max|ref|)
    ref64, _ = reference_gradients(double=True)
    corr = {"loss64": np.float64(ref64["loss"])}
    for key, v64 in stored(ref64, shapes).items():
        if key.startswith("rows:"):
            continue
        c = v64 - out[key].astype(np.float64)
        sc = max(np.abs(c).max(), 1e-300)
        corr["c:" + key] = (c / sc).astype(np.float16)
        corr["s:" + key] = np.float64(sc)
    fp32 = tth.model_gradients(None)
    for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        fm = tth.model_gradients(dt)
        for key in tth.golden_gradient_keys(out):
            a, b = tth.select_like_golden(fm, key, out), tth.select_like_golden(fp32, key, out)
            out["em_%s:%s" % (tag, key)] = np.float64(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
            if key.endswith("k_proj.bias"):      # true gradient zero: the model's own magnitude is the yardstick
                out["abs_%s:%s" % (tag, key)] = np.float64(np.abs(a).max())
        out["em_%s:outs" % tag] = np.float64(np.abs(fm["outs"] - fp32["outs"]).max() / np.abs(fp32["outs"]).max())
    # the restatement is the reference's function: against the fp64 run, and the fp32 run for comparison
    fp64 = tth.model_gradients(None, double=True)
    g64 = tth.apply_fp64_correction(dict(out), corr)
    for key in tth.golden_gradient_keys(out):
        if key.endswith("k_proj.bias"):
            continue
        scale = np.abs(g64[key]).max()
        rel = [np.abs(tth.select_like_golden(m, key, out) - g64[key]).max() / scale for m in (fp64, fp32)]
        print("%-58s model fp64 %.2e fp32 %.2e  reference in fp32 %.2e   e_model bf16 %.2e  f16 %.2e"
              % (key, rel[0], rel[1], np.abs(out[key] - g64[key]).max() / scale, out["em_bf16:" + key],
                 out["em_f16:" + key]))
    # three files, each under the 1 MiB limit for a committed file: the 2-D weight rows and the fp64 correction
    wide = {k: v for k, v in out.items() if k.split(":")[0] in ("d", "rows") and k.endswith(".weight")
            and out["d:" + k.split(":", 1)[1]].ndim == 2}
    main_part = {k: v for k, v in out.items() if k not in wide}
    for part, name in ((main_part, "train_grads_N%d.npz"), (wide, "train_grads_N%d_w.npz"),
                       (corr, "train_grads_N%d_f64.npz")):
        path = os.path.join(HERE, name % tth.GOLDEN_N)
        np.savez_compressed(path, **part)
        print("wrote", path, os.path.getsize(path), "bytes", len(part), "arrays")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
