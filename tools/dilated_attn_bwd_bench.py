"""Forward + backward of the dilated attention core (q, k, v -> merged rows before inner_attn_ln) at the 70k slide's
shape, by two routes, both 16-bit formats, in one process:

  fused  runtime.dilated_attention_grad: gp_dilated_attn_fwd + gp_branch_merge_ln, backward gp_dilated_attn_bwd
  seam   the reference's DilatedAttention core around flash_attn_func under autograd: per branch three gathers
         (zero pads), flash_attn_func (gp_seg_attn_fwd / gp_seg_attn_bwd), the scatter, then the LSE merge with
         no-grad weights -- tests/test_dilated_bwd_host.dilated_core with its index tensors built once and kept
         on the device, so that no host work sits between the launches that are timed

The arms alternate round by round.  One JSON line per format: median ms per forward + backward of each route over
`rounds` x `iters` calls (HIP events on the launch stream, after `warmup` untimed calls of each), min / max per
route (the round-to-round spread), the ratio, and torch.cuda.max_memory_allocated of one forward + backward of each
route above what was allocated before it (the fused route's grow-only workspace is allocated by then: its size is
reported next to it).

    python tools/dilated_attn_bwd_bench.py [--L 70001] [--rounds 7] [--iters 3] [--warmup 2]
                                           [--out profiles/dilated_attn_bwd_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prov-gigapath-replication_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import oracle as orc  # noqa: E402
from gigapath import _hip, runtime  # noqa: E402
from gigapath.torchscale.component.flash_attention import flash_attn_func  # noqa: E402

H, D = 16, 48
SEGS = [1024, 5792, 32768, 185363, 1048576]      # LongNetViT.get_optimal_segment_length(262144, 256)
RATIOS = [1, 2, 4, 8, 16]


class SeamCore:
    """dilated_core of tests/test_dilated_bwd_host.py with the gather / scatter index tensors cached on the device."""

    def __init__(self, L, dev):
        self.L = L
        hcol = torch.arange(H, device=dev)
        self.br = []
        for sl, r in zip(SEGS, RATIOS):
            tok = torch.from_numpy(orc.gather_index(L, sl, r, H)).to(dev)          # [nseg, H, m], -1 = zero pad
            tok = torch.where(tok < 0, torch.full_like(tok, L), tok)
            hidx = hcol.view(1, H, 1).expand_as(tok).contiguous()
            n_idx, i_idx = (torch.from_numpy(a).to(dev) for a in orc.scatter_index(L, sl, r, H))   # [L, H]
            cov = n_idx >= 0
            self.br.append((tok, hidx, n_idx.clamp(min=0), i_idx.clamp(min=0), hcol.view(1, H).expand(L, H).contiguous(),
                            cov))

    def __call__(self, q, k, v):
        B, L = q.shape[0], self.L
        dense_o, dense_l = [], []
        for tok, hidx, nn_, ii, hh, cov in self.br:
            nseg, _, m = tok.shape

            def gather(t):
                tp = torch.cat([t, t.new_zeros(B, 1, H, D)], dim=1)
                return tp[:, tok, hidx].permute(0, 1, 3, 2, 4).reshape(B * nseg, m, H, D)

            o, lse = flash_attn_func(gather(q), gather(k), gather(v))
            o = o.view(B, nseg, m, H, D)
            lse = lse.view(B, nseg, H, m)
            dense_o.append(o[:, nn_, ii, hh] * cov[None, :, :, None].to(o.dtype))
            with torch.no_grad():
                ld = lse.float()[:, nn_, hh, ii]
                dense_l.append(torch.where(cov[None] & (ld != 0), ld, torch.full_like(ld, -1e8)))
        with torch.no_grad():
            mx = torch.stack(dense_l, 0).max(0)[0]
            w = [torch.exp(l - mx) for l in dense_l]
            wsum = torch.stack(w, 0).sum(0)
            w = [t / wsum for t in w]
        out = 0
        for od, wi in zip(dense_o, w):
            out = out + od * wi[..., None].to(od.dtype)
        return out.reshape(B, L, H * D)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=70001)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _hip.load_library()
    dev = torch.device("cuda")
    L, E = args.L, H * D
    core = SeamCore(L, dev)
    lines = []
    for dt, fmt in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        g = torch.Generator(device=dev).manual_seed(L)
        q, k, v = (torch.randn(1, L, H, D, device=dev, generator=g) for _ in range(3))
        dm = torch.randn(L, E, device=dev, generator=g).to(dt)
        qs = (D ** -0.5) * runtime.LOG2E                                   # folded into the Q projection on this route
        qkv = torch.cat([(q * qs).view(L, E), k.view(L, E), v.view(L, E)], 1).to(dt).requires_grad_(True)
        ql, kl, vl = (t.to(dt).requires_grad_(True) for t in (q, k, v))

        def fused():
            qkv.grad = None
            runtime.dilated_attention_grad(qkv, 1, L, H, D, SEGS, RATIOS, True).backward(dm)

        def seam():
            ql.grad = kl.grad = vl.grad = None
            core(ql, kl, vl).backward(dm.view(1, L, E))

        for _ in range(args.warmup):
            fused()
            seam()
        torch.cuda.synchronize()
        tf, ts = [], []
        for _ in range(args.rounds):                                       # interleaved arms
            tf.append(timed(fused, args.iters))
            ts.append(timed(seam, args.iters))
        mem_f, mem_s = peak_of(fused), peak_of(seam)
        assert torch.isfinite(qkv.grad.float()).all() and torch.isfinite(ql.grad.float()).all()
        # the two routes compute the same gradients (dq of the fused route is with respect to q' = q qs)
        dk_rel = ((qkv.grad[:, E:2 * E].float() - kl.grad.view(L, E).float()).abs().max() /
                  kl.grad.float().abs().max()).item()
        ws = _hip.load_library().gp_dilated_attn_bwd_workspace_bytes(1, L, H, D, _hip._i32_array(SEGS),
                                                                     _hip._i32_array(RATIOS), len(SEGS)) / 2 ** 20
        mf, ms = statistics.median(tf), statistics.median(ts)
        rec = {"tool": "dilated_attn_bwd_bench", "fmt": fmt, "L": L, "H": H, "D": D, "segs": SEGS, "ratios": RATIOS,
               "fused_ms": round(mf, 3), "seam_ms": round(ms, 3), "seam_over_fused": round(ms / mf, 3),
               "fused_ms_min_max": [round(min(tf), 3), round(max(tf), 3)],
               "seam_ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
               "fused_peak_mib": round(mem_f, 1), "fused_workspace_mib": round(ws, 1),
               "seam_peak_mib": round(mem_s, 1),
               "dk_fused_vs_seam_max_rel": round(dk_rel, 5),
               "rounds": args.rounds, "iters": args.iters, "warmup": args.warmup,
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
