"""Rates of mrl_table_grad_batch_mat / mrl_table_grad_queue on random pairs at MERL dims.  Device-resident arrays,
events around the call, 3 warm-up + 10 timed launches, medians with min / max.
  single   mrl_table_grad_batch, the single-material call — the one part that also runs on a checkout from before these calls
           existed: --root names that checkout (built), and its JSON is merged in with --parent
  mat      four targets, random ids, one table_grad_mat call — against the route without it: per material a torch mask-compaction
           of the three streams plus one table_grad call (the compaction is timed: it is part of that route)
  queue    table_grad_queue over an ascending queue of 100 %, 50 % and 10 % of the slots

    python tools/table_grad_mat_rates.py --part single --root ../parent --out parent.json
    python tools/table_grad_mat_rates.py [--log2n 24] [--parent parent.json ...] [--out profiles/table_grad_mat_rates.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (90, 90, 180)
TARGETS = 4


def timed(gpu, call, warmup=3, steps=10):
    for _ in range(warmup):
        call()
    gpu.synchronize()
    ms = []
    for _ in range(steps):
        gpu.timer_start(); call(); ms.append(gpu.timer_stop())
    return ms


def row(ms, n):
    med = statistics.median(ms)
    return {"ms": ms, "median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "units_per_s": n / (med * 1e-3)}


def show(label, r):
    print(f"{label:44s} median {r['median_ms']:9.3f} ms  [{r['min_ms']:.3f}, {r['max_ms']:.3f}]  {r['units_per_s'] / 1e9:.3f} G units/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--part", choices=("all", "single"), default="all")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and library are measured")
    ap.add_argument("--parent", action="append", default=[], help="JSON of a --part single run on the parent commit (repeatable)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_grad_mat_rates.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from mitsuba_customization_amd import host
    n = 1 << args.log2n
    result = {"n": n, "dims": DIMS, "lookup": "trilinear", "device": None, "library": host.build_info(), "warmup": 3, "steps": 10}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        ids = [gpu.upload_table(np.ones((3,) + DIMS), (1.0, 1.0, 1.0)) for _ in range(TARGETS)]
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        g = torch.randn((n, 3), dtype=torch.float32, device="cuda")
        G1 = torch.zeros((3,) + DIMS, dtype=torch.float64, device="cuda")
        result["single"] = row(timed(gpu, lambda: gpu.table_grad(wi, wo, g, material=ids[0], out=G1)), n)
        show("single material, mrl_table_grad_batch", result["single"])
        if args.part == "all":
            cells = int(np.prod(DIMS))
            G = torch.zeros((TARGETS * 3 * cells,), dtype=torch.float64, device="cuda")
            mat = torch.tensor(ids, dtype=torch.int32, device="cuda")[torch.randint(0, TARGETS, (n,), device="cuda")].contiguous()
            result["mat"] = {"targets": TARGETS}
            result["mat"]["one_call"] = row(timed(gpu, lambda: gpu.table_grad_mat(wi, wo, g, ids, mat=mat, out=G)), n)
            show(f"{TARGETS} targets, one table_grad_mat call", result["mat"]["one_call"])
            views = [G[k * 3 * cells:(k + 1) * 3 * cells].view((3,) + DIMS) for k in range(TARGETS)]

            def compacted():
                for k, mid in enumerate(ids):
                    at = torch.nonzero(mat == mid).squeeze(1)
                    gpu.table_grad(wi[at], wo[at], g[at], material=mid, out=views[k])
            result["mat"]["compaction_plus_single_calls"] = row(timed(gpu, compacted), n)
            show(f"{TARGETS} x (torch compaction + table_grad)", result["mat"]["compaction_plus_single_calls"])
            result["mat"]["speedup_median"] = result["mat"]["compaction_plus_single_calls"]["median_ms"] / result["mat"]["one_call"]["median_ms"]
            result["queue"] = {}
            for percent in (100, 50, 10):
                m = n * percent // 100
                queue = torch.sort(torch.randperm(n, device="cuda")[:m]).values.to(torch.int32).contiguous()
                count = torch.tensor([m], dtype=torch.int32, device="cuda")
                r = row(timed(gpu, lambda: gpu.table_grad_queue(wi, wo, g, queue, count, ids, mat=mat, out=G)), m)
                result["queue"][f"{percent}%"] = r
                show(f"queue, {percent} % of the slots", r)
    if args.parent:
        runs = [json.load(open(p)) for p in args.parent]
        meds = [r["single"]["median_ms"] for r in runs]
        ours = result["single"]["median_ms"]
        result["single_on_parent"] = {"library": runs[0]["library"], "runs": [r["single"] for r in runs], "medians_ms": meds,
                                      "this_commit_median_ms": ours,
                                      "within_parent_spread": min(r["single"]["min_ms"] for r in runs) <= ours <= max(r["single"]["max_ms"] for r in runs)}
        print(f"single material: parent medians {meds} ms, this commit {ours:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
