"""A/B of the packed key-row tail: forward_packed with runtime.KEYROW_TAIL_PACKED off / on, alternated in
one process on one device.  Workloads: the C5 batch of bench.py --mode mixed (32 slides of 2k-100k tiles) and one
70k-tile slide through forward_packed.  Eager launches (no HIP graph), each timed step between device synchronises;
prints one JSON object and, with --out, writes it to a file.

    python tools/keyrow_packed_ab.py --rounds 3 --steps 3 --out profiles/keyrow_packed_bench_ab.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "prov-gigapath-replication_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
import oracle  # noqa: E402
from gigapath import batch, runtime, slide_encoder  # noqa: E402

ARCH = "gigapath_slide_enc12l768d"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="off / on alternations per workload")
    ap.add_argument("--steps", type=int, default=3, help="timed forwards per switch setting and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    W = oracle.make_weights(oracle.arch_config(ARCH), seed=0)
    model = slide_encoder.create_model("", ARCH, 1536)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    model = model.to(dev).eval()
    model.use_hip_graphs = False

    def slides_of(sizes):
        out = []
        for i, n in enumerate(sizes):
            x, c = bench.make_slide(n, seed=100 + 2 * i)
            out.append((torch.from_numpy(x[0]).to(dev), torch.from_numpy(c[0]).to(dev)))
        return out

    res = {"arch": ARCH, "rounds": args.rounds, "steps": args.steps, "launches": "eager", "workloads": {}}
    for name, sizes in (("c5_mixed_32", batch.mixed_batch_sizes(n_slides=32)), ("one_slide_70k", [70000])):
        slides = slides_of(sizes)
        segs, ratios = model.encoder.args.segment_length, model.encoder.args.dilated_ratio
        plan = runtime.packed_key_row_plan([n + 1 for n in sizes], segs, ratios)
        T = sum(sizes) + len(sizes)
        times, outs = {False: [], True: []}, {}
        for rnd in range(args.rounds + 1):               # round 0 warms both settings up (untimed)
            for on in (False, True):
                runtime.KEYROW_TAIL_PACKED = on
                for _ in range(args.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with torch.no_grad():
                        o = model.forward_packed(slides, all_layer_embed=True)
                    torch.cuda.synchronize()
                    if rnd:
                        times[on].append((time.perf_counter() - t0) * 1e3)
                outs[on] = torch.stack([torch.cat(s, 0) for s in o], 1).float()
        runtime.KEYROW_TAIL_PACKED = False
        d = (outs[True] - outs[False]).abs()
        off_ms, on_ms = statistics.median(times[False]), statistics.median(times[True])
        res["workloads"][name] = {
            "slides": len(sizes), "tiles": int(sum(sizes)), "packed_tokens": int(T),
            "listed_rows": int(plan["n"].sum()), "listed_share": float(plan["n"].sum()) / T,
            "engages": bool(plan["n"].sum() <= runtime.KEYROW_MAX_SHARE * T),
            "off_ms": [round(t, 3) for t in times[False]], "on_ms": [round(t, 3) for t in times[True]],
            "off_median_ms": round(off_ms, 3), "on_median_ms": round(on_ms, 3),
            "on_over_off": round(on_ms / off_ms, 4),
            "embeds_0_to_depth_minus_2_bit_identical": bool(torch.equal(outs[True][:-2], outs[False][:-2])),
            "last_two_max_abs_diff": float(d[-2:].max()), "last_two_max_abs": float(outs[False][-2:].abs().max())}
        del slides
        model.encoder.engine._pws.clear()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
