"""Forward and backward at the flash_attn_func seam at the 70k slide's five launch shapes, both
16-bit formats, in one process: gp_seg_attn_fwd[_f16] against gp_seg_attn_bwd on the same tensors.

One JSON line per (format, shape): median ms per call of forward and backward over `rounds` x `iters` launches
(HIP events on the launch stream, after `warmup` untimed calls of each), their ratio, and the backward's TF/s
counting 10 D L^2 FLOPs per (batch, head) -- five L x L x D products.

    python tools/attn_bwd_bench.py [--rounds 7] [--iters 5] [--warmup 3] [--out profiles/attn_bwd_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prov-gigapath-replication_amd"))
import torch  # noqa: E402

from gigapath import _hip  # noqa: E402

SHAPES = ((69, 1024), (13, 2896), (3, 8192), (1, 8751), (1, 4376))   # (nbatch, seqlen) of the 70k slide's branches
H, D = 16, 48


def timed(fn, rounds, iters):
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _hip.load_library()
    dev = torch.device("cuda")
    lines = []
    for dt, fmt in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        for nb, sl in SHAPES:
            g = torch.Generator(device=dev).manual_seed(sl)
            q, k, v, do = (torch.randn(nb, sl, H, D, device=dev, generator=g).to(dt) for _ in range(4))
            o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
            lse = torch.empty(nb, H, sl, dtype=torch.float32, device=dev)

            def fwd():
                _hip.seg_attn_fwd(q, k, v, o, lse)

            def bwd():
                _hip.seg_attn_bwd(q, k, v, o, lse, do, dq, dk, dv)

            for _ in range(args.warmup):
                fwd()
                bwd()
            torch.cuda.synchronize()
            tf, tb = timed(fwd, args.rounds, args.iters), timed(bwd, args.rounds, args.iters)
            mf, mb = statistics.median(tf), statistics.median(tb)
            assert torch.isfinite(dq.float()).all() and torch.isfinite(dk.float()).all() and torch.isfinite(dv.float()).all()
            rec = {"tool": "attn_bwd_bench", "fmt": fmt, "nbatch": nb, "seqlen": sl, "H": H, "D": D,
                   "fwd_ms": round(mf, 4), "bwd_ms": round(mb, 4), "bwd_over_fwd": round(mb / mf, 3),
                   "bwd_tflops": round(10.0 * D * sl * sl * nb * H / (mb * 1e-3) / 1e12, 2),
                   "fwd_ms_min_max": [round(min(tf), 4), round(max(tf), 4)],
                   "bwd_ms_min_max": [round(min(tb), 4), round(max(tb), 4)],
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
