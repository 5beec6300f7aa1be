"""Rates of mrl_ggx_grad_batch: the gradient alone and the gradient with the normal matrix on the gold-like metal at
alpha 0.05 and 0.3, with mrl_eval_batch on the same material and inputs in the same process as the baseline — the workaround the
call replaces is central differences, 14 eval launches (before their reductions).  Device-resident generate_pairs inputs, events
around the whole call, 3 warm-up + 10 timed launches, median [min, max].

    python tools/ggx_grad_rates.py [--log2n 24] [--out profiles/ggx_grad_rates.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHAS = (0.05, 0.3)
ETA, K = (0.143, 0.375, 1.442), (3.983, 2.386, 1.603)          # gold-like
EVALS_OF_CENTRAL_DIFFERENCES = 14


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
    from mitsuba_customization_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ggx_grad_rates.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    result = {"n": n, "eta": ETA, "k": K, "device": None, "library": host.build_info(), "warmup": 3, "steps": 10,
              "evals_of_central_differences": EVALS_OF_CENTRAL_DIFFERENCES, "alphas": {}}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        g = torch.randn((n, 3), dtype=torch.float32, device="cuda")
        h = torch.randn((n, 3), dtype=torch.float32, device="cuda").abs()
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        G = torch.zeros(7, dtype=torch.float64, device="cuda")
        N = torch.zeros((7, 7), dtype=torch.float64, device="cuda")
        for alpha in ALPHAS:
            mid = gpu.ggx(alpha, ETA, K)
            rows = {
                "mrl_eval_batch (baseline)": {"ms": timed(gpu, lambda: gpu.eval(wi, wo, material=mid, out=rgb))},
                "gradient": {"ms": timed(gpu, lambda: gpu.ggx_grad(wi, wo, g, mid, out=G))},
                "gradient + normal": {"ms": timed(gpu, lambda: gpu.ggx_grad(wi, wo, g, mid, curvature=h, normal=True, out=(G, N)))},
            }
            gpu.release_material(mid)
            for label, row in rows.items():
                med = statistics.median(row["ms"])
                row.update({"median_ms": med, "min_ms": min(row["ms"]), "max_ms": max(row["ms"]), "units_per_s": n / (med * 1e-3)})
                print(f"alpha {alpha:5g} {label:26s} median {med:8.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  {row['units_per_s'] / 1e9:.3f} G units/s", flush=True)
            ev, gr, gn = rows["mrl_eval_batch (baseline)"], rows["gradient"], rows["gradient + normal"]
            rows["acceptance"] = {"slowest_gradient_over_fastest_eval": gr["max_ms"] / ev["min_ms"],
                                  "slowest_gradient_normal_over_fastest_eval": gn["max_ms"] / ev["min_ms"],
                                  "gradient_faster_than_14_evals": gr["max_ms"] < EVALS_OF_CENTRAL_DIFFERENCES * ev["min_ms"]}
            print(f"alpha {alpha:5g} slowest gradient / fastest eval = {rows['acceptance']['slowest_gradient_over_fastest_eval']:.2f} "
                  f"(with normal {rows['acceptance']['slowest_gradient_normal_over_fastest_eval']:.2f}); bar: < {EVALS_OF_CENTRAL_DIFFERENCES}", flush=True)
            result["alphas"][f"{alpha:g}"] = rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
