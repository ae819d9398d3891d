"""Training-step measurements of the slide encoder, fused against GIGAPATH_TRAIN_FFN_FUSED=0 and against
GIGAPATH_TRAIN_ROWS_FUSED=0, in one process:

  (a) op    runtime.gelu_layernorm_grad forward + backward at [M, F] (default 70,001 x 3,072), bf16 and fp16,
            against runtime.gelu_layernorm_torch (the plain torch composition): median ms, peak MiB above what was
            allocated before the call, and gp_gelu_layernorm_bwd alone with its achieved bytes/s over the
            algorithmic bytes (2 bytes x M x F for each of h, dy and dh) against the 6.29 TB/s HBM rate
  (b) step  one training step of LongNetViT at N tiles (default 70,000): forward with all_layer_embed, a scalar
            loss, backward; the finetune defaults (dropout 0.1, drop-path 0.1), bf16 and fp16 autocast; three
            interleaved arms: everything fused, the FFN middle on torch, the model-width rows on torch
  (c) rows  runtime.resid_drop_ln_grad forward + backward (the add + LN call) at [M, E] (default 70,001 x 768,
            p = 0.1, one drop-path factor) against its torch composition, and every row kernel alone (add + LN, add,
            LN of the fp32 stream, LN of a 16-bit tensor; forward and backward; the add shapes at p = 0.1 and p = 0)
            with its achieved bytes/s over the algorithmic bytes against the 6.29 TB/s HBM rate

  (d) packed  one training step (forward with all_layer_embed, a scalar loss, backward) of a mixed-length batch in
            one process, two interleaved arms: LongNetViT.forward_packed (one varlen attention backward per layer),
            and the same slides one per forward() call with gradients accumulated (the path without packing).  Two
            batches: 16 slides of batch.mixed_batch_sizes(16, 500, 8000) (launch-bound) and 8 slides of
            mixed_batch_sizes(8, 2000, 100000) (compute-bound); bf16 and fp16; ms (min - max), peak MiB, tiles/s

The arms alternate round by round (HIP events on the launch stream, `warmup` untimed calls of each arm first,
median over `rounds` x `iters`).  One JSON line per (part, format).

    python tools/train_step_bench.py [--parts op,step,rows] [--M 70001] [--F 3072] [--E 768] [--N 70000]
                                     [--rounds 7] [--iters 3] [--warmup 2] [--out profiles/train_step_bench.json]
    python tools/train_step_bench.py --parts packed --out profiles/train_packed_bench.json
    python tools/train_step_bench.py --profile-steps 2          # fused steps only: the program of a
                                                                # rocprofv3 --kernel-trace --stats run of its own
    python tools/train_step_bench.py --profile-steps 2 --profile-packed   # the same for packed steps (small batch)
    python tools/train_step_bench.py --shares KERNEL_STATS.csv  # attention / GEMM / GELU+LN / rows / rest shares
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prov-gigapath-replication_amd"))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_of(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def ab(fused, plain, args):
    for _ in range(args.warmup):
        fused()
        plain()
    tf, tp = [], []
    for _ in range(args.rounds):                                           # interleaved arms
        tf.append(timed(fused, args.iters))
        tp.append(timed(plain, args.iters))
    mf, mp = statistics.median(tf), statistics.median(tp)
    return {"fused_ms": round(mf, 3), "unfused_ms": round(mp, 3), "unfused_over_fused": round(mp / mf, 3),
            "fused_ms_min_max": [round(min(tf), 3), round(max(tf), 3)],
            "unfused_ms_min_max": [round(min(tp), 3), round(max(tp), 3)],
            "fused_peak_mib": round(peak_of(fused), 1), "unfused_peak_mib": round(peak_of(plain), 1)}


def abn(arms, args):
    """ab for any number of named arms, interleaved round by round: {name}_ms, {name}_ms_min_max, {name}_peak_mib."""
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn, args.iters))
    rec = {}
    for k, fn in arms.items():
        rec[k + "_ms"] = round(statistics.median(times[k]), 3)
        rec[k + "_ms_min_max"] = [round(min(times[k]), 3), round(max(times[k]), 3)]
        rec[k + "_peak_mib"] = round(peak_of(fn), 1)
    return rec


def bench_op(args, dt, fmt):
    import torch
    from gigapath import _hip, runtime
    dev = torch.device("cuda")
    M, F = args.M, args.F
    g = torch.Generator(device=dev).manual_seed(M)
    h = (1.5 * torch.randn(M, F, device=dev, generator=g)).to(dt).requires_grad_(True)
    dy = torch.randn(M, F, device=dev, generator=g).to(dt)
    w = torch.nn.Parameter(1.0 + 0.2 * torch.randn(F, device=dev, generator=g))
    b = torch.nn.Parameter(0.1 * torch.randn(F, device=dev, generator=g))

    def run(fn):
        def go():
            h.grad = w.grad = b.grad = None
            fn(h, w, b, 1e-5).backward(dy)
        return go

    rec = {"tool": "train_step_bench", "part": "op", "fmt": fmt, "M": M, "F": F}
    rec.update(ab(run(runtime.gelu_layernorm_grad), run(runtime.gelu_layernorm_torch), args))
    # the backward kernel alone
    dh, dw, db = torch.empty_like(dy), torch.empty(F, device=dev), torch.empty(F, device=dev)
    hd, wd = h.detach(), w.detach()

    def kernel():
        _hip.gelu_layernorm_bwd(hd, dy, wd, 1e-5, dh, dw, db)

    kernel()
    tk = statistics.median(timed(kernel, args.iters) for _ in range(args.rounds))
    nbytes = 3 * 2 * M * F
    rec.update({"bwd_kernel_ms": round(tk, 4), "bwd_algorithmic_bytes": nbytes,
                "bwd_bytes_per_s": round(nbytes / (tk * 1e-3), 0),
                "bwd_share_of_hbm_rate": round(nbytes / (tk * 1e-3) / HBM_BYTES_PER_S, 3)})
    return rec


def make_step(args, fmt):
    import numpy as np
    import torch
    import oracle as orc
    from gigapath import slide_encoder
    dev = torch.device("cuda")
    cfg = orc.arch_config("gigapath_slide_enc12l768d")
    model = slide_encoder.create_model("", "gigapath_slide_enc12l768d", 1536, dropout=0.1, drop_path_rate=0.1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_weights(cfg, seed=0).items()}, strict=True)
    model = model.to(dev).enable_training().train()
    x, coords = orc.synthetic_slide(args.N)
    x = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dev)
    coords = torch.from_numpy(np.asarray(coords)).to(dev)
    model.validate_positions = False                                       # no host sync inside the timed step

    def step():
        for p in model.parameters():
            p.grad = None
        with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
            outs = model(x, coords, all_layer_embed=True)
        sum(o.float().square().mean() for o in outs).backward()

    return step


def bench_step(args, fmt):
    from gigapath import runtime
    step = make_step(args, fmt)

    def arm(ffn, rows):
        def go():
            runtime.TRAIN_FFN_FUSED, runtime.TRAIN_ROWS_FUSED = ffn, rows
            step()
        return go

    rec = {"tool": "train_step_bench", "part": "step", "fmt": fmt, "N": args.N, "dropout": 0.1, "drop_path": 0.1}
    try:
        rec.update(abn({"fused": arm(True, True), "ffn_unfused": arm(False, True), "rows_unfused": arm(True, False)},
                       args))
    finally:
        runtime.TRAIN_FFN_FUSED = runtime.TRAIN_ROWS_FUSED = True
    rec["rows_unfused_over_fused"] = round(rec["rows_unfused_ms"] / rec["fused_ms"], 3)
    rec["ffn_unfused_over_fused"] = round(rec["ffn_unfused_ms"] / rec["fused_ms"], 3)
    return rec


PACKED_BATCHES = {"small": (16, 500, 8000), "large": (8, 2000, 100000)}


def make_packed_steps(args, fmt, which):
    """(packed step, sequential step, tiles) for one of PACKED_BATCHES on one model."""
    import torch
    import oracle as orc
    from gigapath import batch, slide_encoder
    dev = torch.device("cuda")
    cfg = orc.arch_config("gigapath_slide_enc12l768d")
    model = slide_encoder.create_model("", "gigapath_slide_enc12l768d", 1536, dropout=0.1, drop_path_rate=0.1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in orc.make_weights(cfg, seed=0).items()}, strict=True)
    model = model.to(dev).enable_training().train()
    model.validate_positions = False                                       # no host sync inside the timed step
    sizes = batch.mixed_batch_sizes(*PACKED_BATCHES[which])
    slides = []
    for i, n in enumerate(sizes):
        x, c = orc.synthetic_slide(n, seed_x=100 + i, seed_c=200 + i)
        slides.append((torch.from_numpy(x[0]).to(dev), torch.from_numpy(c[0]).to(dev)))

    def loss_of(outs):
        return sum(o.float().square().mean() for o in outs)

    def packed():
        for p in model.parameters():
            p.grad = None
        with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
            outs = model.forward_packed(slides, all_layer_embed=True)
        sum(loss_of(o) for o in outs).backward()

    def sequential():
        for p in model.parameters():
            p.grad = None
        for x, c in slides:
            with torch.autocast("cuda", torch.float16, enabled=fmt == "fp16"):
                outs = model(x[None], c[None], all_layer_embed=True)
            loss_of(outs).backward()

    return packed, sequential, sizes


def bench_packed(args, fmt, which):
    packed, sequential, sizes = make_packed_steps(args, fmt, which)
    rec = {"tool": "train_step_bench", "part": "packed", "fmt": fmt, "batch": which, "slides": len(sizes),
           "tiles": int(sum(sizes)), "sizes": sizes, "dropout": 0.1, "drop_path": 0.1}
    for _ in range(args.warmup):
        packed()
        sequential()
    times = {"packed": [], "sequential": []}
    for _ in range(args.rounds):                                           # interleaved arms
        times["packed"].append(timed(packed, args.iters))
        times["sequential"].append(timed(sequential, args.iters))
    for k, fn in (("packed", packed), ("sequential", sequential)):
        med = statistics.median(times[k])
        rec[k + "_ms"] = round(med, 3)
        rec[k + "_ms_min_max"] = [round(min(times[k]), 3), round(max(times[k]), 3)]
        rec[k + "_rounds_ms"] = [round(t, 3) for t in times[k]]
        rec[k + "_peak_mib"] = round(peak_of(fn), 1)
        rec[k + "_tiles_per_s"] = round(sum(sizes) / (med * 1e-3), 0)
    rec["sequential_over_packed"] = round(rec["sequential_ms"] / rec["packed_ms"], 3)
    rec["every_packed_round_below_every_sequential_round"] = max(times["packed"]) < min(times["sequential"])
    return rec


def bench_rows(args, dt, fmt):
    import torch
    from gigapath import _hip, runtime
    dev = torch.device("cuda")
    M, E, p = args.M, args.E, 0.1
    g = torch.Generator(device=dev).manual_seed(M)
    x = torch.randn(M, E, device=dev, generator=g).requires_grad_(True)
    y = torch.randn(M, E, device=dev, generator=g).to(dt).requires_grad_(True)
    da = torch.randn(M, E, device=dev, generator=g).to(dt)
    dr = torch.randn(M, E, device=dev, generator=g)
    ln = torch.nn.LayerNorm(E, eps=1e-5).to(dev)
    s = torch.ones(1, device=dev)

    def arm(flag):
        def go():
            runtime.TRAIN_ROWS_FUSED = flag
            x.grad = y.grad = ln.weight.grad = ln.bias.grad = None
            r, a = runtime.resid_drop_ln_grad(x, y, ln, p, s, True)
            torch.autograd.backward([r, a], [dr, da])
        return go

    rec = {"tool": "train_step_bench", "part": "rows", "fmt": fmt, "M": M, "E": E, "p": p}
    try:
        rec.update(abn({"fused": arm(True), "unfused": arm(False)}, args))
    finally:
        runtime.TRAIN_ROWS_FUSED = True
    rec["unfused_over_fused"] = round(rec["unfused_ms"] / rec["fused_ms"], 3)
    # every kernel alone: bytes per element read + written, by the algorithm
    xd, yd, x16 = x.detach(), y.detach(), x.detach().to(dt)
    w, b = ln.weight.detach(), ln.bias.detach()
    r, a = torch.empty_like(xd), torch.empty_like(yd)
    dx, dy, dx16 = torch.empty_like(xd), torch.empty_like(yd), torch.empty_like(yd)
    dw, db = torch.empty(E, device=dev), torch.empty(E, device=dev)
    kernels = {}
    for q in (p, 0.0):
        tag = "_p%g" % q
        kernels["add_ln_fwd" + tag] = (12, lambda q=q: _hip.resid_drop_ln_fwd(xd, yd, s, q, 7, w, b, 1e-5, r, a))
        kernels["add_ln_bwd" + tag] = (16, lambda q=q: _hip.resid_drop_ln_bwd(da, dr, r, w, 1e-5, s, q, 7, dx, dy, dw, db))
        kernels["add_fwd" + tag] = (10, lambda q=q: _hip.resid_drop_ln_fwd(xd, yd, s, q, 7, None, None, 0.0, r, None))
        kernels["add_bwd" + tag] = (6, lambda q=q: _hip.resid_drop_ln_bwd(None, dr, None, None, 0.0, s, q, 7, None, dy))
    kernels["ln32_fwd"] = (6, lambda: _hip.resid_drop_ln_fwd(xd, None, None, 0.0, 0, w, b, 1e-5, None, a))
    kernels["ln32_bwd"] = (10, lambda: _hip.resid_drop_ln_bwd(da, None, xd, w, 1e-5, None, 0.0, 0, dx, None, dw, db))
    kernels["ln16_fwd"] = (4, lambda: _hip.resid_drop_ln_fwd(x16, None, None, 0.0, 0, w, b, 1e-5, None, a))
    kernels["ln16_bwd"] = (6, lambda: _hip.resid_drop_ln_bwd(da, None, x16, w, 1e-5, None, 0.0, 0, dx16, None, dw, db))
    rec["kernels"] = {}
    for name, (bpe, fn) in kernels.items():
        fn()
        tk = statistics.median(timed(fn, args.iters) for _ in range(args.rounds))
        nbytes = bpe * M * E
        rec["kernels"][name] = {"ms": round(tk, 4), "bytes_per_element": bpe, "algorithmic_bytes": nbytes,
                                "bytes_per_s": round(nbytes / (tk * 1e-3), 0),
                                "share_of_hbm_rate": round(nbytes / (tk * 1e-3) / HBM_BYTES_PER_S, 3)}
    return rec


def shares(path):
    """Attention / GEMM / GELU+LN / model-width rows / rest shares of a rocprofv3 --kernel-trace --stats
    kernel_stats CSV."""
    tot, groups = 0.0, {"attention": 0.0, "gemm": 0.0, "gelu_ln": 0.0, "rows": 0.0, "rest": 0.0}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            low = name.lower()
            if "gelu_ln" in low:
                key = "gelu_ln"
            elif "rows_fwd_kernel" in low or "rows_bwd_" in low:
                key = "rows"
            elif "attn" in low or "branch_merge" in low or "dilated" in low:
                key = "attention"
            elif "cijk" in low or "gemm" in low:
                key = "gemm"
            else:
                key = "rest"
            groups[key] += ns
            tot += ns
    return {"tool": "train_step_bench", "part": "shares", "csv": os.path.basename(path), "total_ms": round(tot / 1e6, 3),
            **{k + "_share": round(v / tot, 4) for k, v in groups.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="op,step")
    ap.add_argument("--M", type=int, default=70001)
    ap.add_argument("--F", type=int, default=3072)
    ap.add_argument("--E", type=int, default=768)
    ap.add_argument("--N", type=int, default=70000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--profile-packed", action="store_true")
    ap.add_argument("--shares", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.shares:
        lines.append(shares(args.shares))
    elif args.profile_steps:
        import torch
        step = make_packed_steps(args, "bf16", "small")[0] if args.profile_packed else make_step(args, "bf16")
        for _ in range(args.profile_steps):
            step()
        torch.cuda.synchronize()
        return
    else:
        import torch
        from gigapath import _hip
        _hip.load_library()
        for part in args.parts.split(","):
            for dt, fmt in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
                if part == "packed":
                    recs = [bench_packed(args, fmt, which) for which in PACKED_BATCHES]
                elif part == "step":
                    recs = [bench_step(args, fmt)]
                else:
                    recs = [{"op": bench_op, "rows": bench_rows}[part](args, dt, fmt)]
                for rec in recs:
                    rec["rounds"], rec["iters"], rec["warmup"] = args.rounds, args.iters, args.warmup
                    rec["device"] = torch.cuda.get_device_name(0)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                torch.cuda.empty_cache()
    if args.shares:
        print(json.dumps(lines[0]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.shares else "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
