"""Same-process, interleaved A/B of the key-row tail on the whole eager forward
(all_layer_embed=True): per round every arm runs one forward; reports each arm's median / min / max forward
time, the round-to-round spread of the off arm, and the median per-kernel spans (runtime.TIMER) of a few extra
timed rounds.

    python tools/keyrow_ab.py [--tiles 70000] [--rounds 15] [--warmup 2] [--out x.json]

Arms: off = GIGAPATH_KEYROW_TAIL=0, on = the default.  Every arm has its own model instance (same weights), so
its workspace, row lists and work table stay allocated between rounds.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "prov-gigapath-replication_amd"))
import torch  # noqa: E402

from gigapath import runtime, slide_encoder  # noqa: E402
from bench import make_slide  # noqa: E402

ARMS = {"off": False, "on": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=70000)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds first (round 0 also records the outputs)")
    ap.add_argument("--span-rounds", type=int, default=3)
    ap.add_argument("--arms", default="off,on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    arms = args.arms.split(",")
    dev = torch.device("cuda")
    with contextlib.redirect_stdout(sys.stderr):
        first = slide_encoder.create_model("", "gigapath_slide_enc12l768d", 1536).to(dev).eval()
        models = {}
        for a in arms:
            m = first if not models else slide_encoder.create_model("", "gigapath_slide_enc12l768d", 1536).to(dev).eval()
            m.load_state_dict(first.state_dict())
            m.use_hip_graphs = False
            models[a] = m
    x, coords = make_slide(args.tiles)
    xt, ct = torch.from_numpy(x).to(dev), torch.from_numpy(coords).to(dev)
    times = {a: [] for a in arms}
    spans = {a: {} for a in arms}
    outs = {}
    with torch.no_grad():
        for rnd in range(args.warmup + args.rounds + args.span_rounds):
            timed = rnd >= args.warmup + args.rounds
            for a in arms:
                runtime.KEYROW_TAIL = ARMS[a]
                runtime.TIMER.reset()
                runtime.TIMER.enabled = timed
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = models[a](xt, ct, all_layer_embed=True)
                e1.record()
                torch.cuda.synchronize()
                runtime.TIMER.enabled = False
                if rnd == 0:
                    outs[a] = torch.stack(out).float().clone()
                elif rnd < args.warmup:
                    pass
                elif not timed:
                    times[a].append(e0.elapsed_time(e1))
                else:
                    for k, (n, ms) in runtime.TIMER.totals_ms().items():
                        spans[a].setdefault(k, []).append((n, ms))
    res = []
    ref = outs[arms[0]]
    for a in arms:
        ts = times[a]
        d = outs[a] - ref
        row = {"arm": a, "forward_ms_median": round(statistics.median(ts), 3), "forward_ms_min": round(min(ts), 3),
               "forward_ms_max": round(max(ts), 3), "forward_ms_all": [round(t, 3) for t in ts],
               "layers_identical_to_first_arm": int((d.abs().amax(dim=(1, 2)) == 0).sum().item()),
               "max_rel_diff_vs_first_arm": (d.abs().max() / ref.abs().max()).item(),
               "span_ms": {k: {"launches": v[0][0], "ms": round(statistics.median(ms for _, ms in v), 4)}
                           for k, v in sorted(spans[a].items())}}
        print(json.dumps({k: v for k, v in row.items() if k != "forward_ms_all"}), flush=True)
        res.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({"tiles": args.tiles, "rounds": args.rounds, "warmup_rounds": args.warmup, "results": res}, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
