"""Rates of mrl_table_grad_batch: the plain planar-atomic kernel against the gradient-brick kernel (wave-uniform
merge choice, never merged, always merged) on random pairs, on a coherent set and on one repeated pair, with mrl_eval_batch on the same inputs as the
transform-only floor.  Device-resident arrays, events around the call, 3 warm-up + 10 timed launches, median.

    python tools/table_grad_rates.py [--log2n 24] [--out profiles/table_grad_rates.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"naive_planar_atomics": 1, "bricks_auto (shipped)": 0, "bricks_never_merged": 2, "bricks_always_merged": 3}
ATOMIC_CEILING_TBS = 1.3          # contiguous global float atomics, added bytes per second


def timed(gpu, call, warmup=3, steps=10):
    for _ in range(warmup):
        call()
    gpu.synchronize()
    ms = []
    for _ in range(steps):
        gpu.timer_start(); call(); ms.append(gpu.timer_stop())
    return ms


def main():
    import torch
    from mitsuba_customization_amd import host, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_grad_rates.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    dims = (90, 90, 180)
    result = {"n": n, "dims": dims, "lookup": "trilinear", "device": None, "library": host.build_info(), "warmup": 3, "steps": 10,
              "added_bytes_per_unit": 8 * 3 * 8, "atomic_ceiling_TBs": ATOMIC_CEILING_TBS, "sets": {}}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        mid = gpu.upload_table(np.ones((3,) + dims), (1.0, 1.0, 1.0))
        g = torch.randn((n, 3), dtype=torch.float32, device="cuda")
        G = torch.zeros((3,) + dims, dtype=torch.float64, device="cuda")
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        wi_r, wo_r, _ = gpu.generate_pairs(0x5EED, 0, n)
        wi_c, wo_c = [torch.from_numpy(a).cuda() for a in synth.coherent_pairs(n)]
        # every unit the same pair (one pixel of an image-based capture seen again and again): the case the in-wave merge is for
        wi_1, wo_1 = wi_c[:1].expand(n, 3).contiguous(), wo_c[:1].expand(n, 3).contiguous()
        for name, (wi, wo) in {"random_pairs": (wi_r, wo_r), "coherent_2deg_cone": (wi_c, wo_c), "one_cell": (wi_1, wo_1)}.items():
            rows = {}
            ms = timed(gpu, lambda: gpu.eval(wi, wo, material=mid, out=rgb))
            rows["mrl_eval_batch (floor)"] = {"ms": ms}
            for label, variant in VARIANTS.items():
                gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
                ms = timed(gpu, lambda: gpu.table_grad(wi, wo, g, material=mid, out=G))
                rows[label] = {"ms": ms}
            gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)
            for label, row in rows.items():
                med = statistics.median(row["ms"])
                row.update({"median_ms": med, "min_ms": min(row["ms"]), "max_ms": max(row["ms"]), "units_per_s": n / (med * 1e-3)})
                if "floor" not in label:
                    row["added_TBs"] = n * result["added_bytes_per_unit"] / (med * 1e-3) / 1e12
                    row["fraction_of_atomic_ceiling"] = row["added_TBs"] / ATOMIC_CEILING_TBS
                print(f"{name:20s} {label:26s} median {med:9.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  {row['units_per_s'] / 1e9:.3f} G units/s", flush=True)
            naive, ship = rows["naive_planar_atomics"], rows["bricks_auto (shipped)"]
            rows["acceptance"] = {"shipped_faster_than_naive": ship["max_ms"] < naive["min_ms"],
                                  "speedup_median": naive["median_ms"] / ship["median_ms"]}
            result["sets"][name] = rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
