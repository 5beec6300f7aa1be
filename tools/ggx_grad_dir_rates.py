"""Rates of mrl_ggx_grad_dir_batch / mrl_ggx_grad_dir_queue on the gold-like metal at alpha 0.05 and 0.3: whole arrays
with both gradients, whole arrays with grad_wo only, material ids over four materials, a dense ascending queue — with mrl_eval_batch on
the same material and inputs in the same process as the baseline: the workaround the calls replace is central differences, at least
8 eval launches (two per tangent direction of wi and of wo).  Device-resident generate_pairs inputs, events around the whole call,
3 warm-up + 10 timed launches, median [min, max].

    python tools/ggx_grad_dir_rates.py [--log2n 24] [--out profiles/ggx_grad_dir_rates.json]
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
EVALS_OF_CENTRAL_DIFFERENCES = 8
# bytes a unit moves: wi, wo, grad_rgb in (36), + 4 with ids, + 4 with a queue; 12 out per gradient.  eval: 24 in, 12 out
BYTES = {"mrl_eval_batch (baseline)": 36, "both gradients": 60, "grad_wo only": 48, "material ids": 64, "queue": 64}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ggx_grad_dir_rates.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    result = {"n": n, "eta": ETA, "k": K, "device": None, "library": host.build_info(), "warmup": 3, "steps": 10,
              "evals_of_central_differences": EVALS_OF_CENTRAL_DIFFERENCES, "bytes_per_unit": BYTES, "alphas": {}}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        g = torch.randn((n, 3), dtype=torch.float32, device="cuda")
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        gwi, gwo = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
        queue = torch.arange(n, dtype=torch.int32, device="cuda")
        count = torch.full((1,), n, dtype=torch.int32, device="cuda")
        for alpha in ALPHAS:
            mids = [gpu.ggx(alpha * s, ETA, K) for s in (1.0, 1.1, 1.2, 1.3)]
            mid = mids[0]
            mat = torch.tensor(mids, dtype=torch.int32, device="cuda")[torch.randint(0, 4, (n,), device="cuda")].contiguous()
            rows = {
                "mrl_eval_batch (baseline)": {"ms": timed(gpu, lambda: gpu.eval(wi, wo, material=mid, out=rgb))},
                "both gradients": {"ms": timed(gpu, lambda: gpu.ggx_grad_dir(wi, wo, g, material=mid, out=(gwi, gwo)))},
                "grad_wo only": {"ms": timed(gpu, lambda: gpu.ggx_grad_dir(wi, wo, g, material=mid, want="wo", out=gwo))},
                "material ids": {"ms": timed(gpu, lambda: gpu.ggx_grad_dir(wi, wo, g, mat=mat, out=(gwi, gwo)))},
                "queue": {"ms": timed(gpu, lambda: gpu.ggx_grad_dir_queue(wi, wo, g, queue, count, material=mid, out=(gwi, gwo)))},
            }
            for m in mids:
                gpu.release_material(m)
            for label, row in rows.items():
                med = statistics.median(row["ms"])
                row.update({"median_ms": med, "min_ms": min(row["ms"]), "max_ms": max(row["ms"]), "units_per_s": n / (med * 1e-3),
                            "GB_per_s": BYTES[label] * n / (med * 1e-3) / 1e9})
                print(f"alpha {alpha:5g} {label:26s} median {med:8.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  "
                      f"{row['units_per_s'] / 1e9:.3f} G units/s  {row['GB_per_s']:.0f} GB/s", flush=True)
            fastest_eval = rows["mrl_eval_batch (baseline)"]["min_ms"]
            slowest = max(row["max_ms"] for label, row in rows.items() if label != "mrl_eval_batch (baseline)")
            rows["acceptance"] = {"slowest_gradient_over_fastest_eval": slowest / fastest_eval,
                                  "faster_than_8_evals": slowest < EVALS_OF_CENTRAL_DIFFERENCES * fastest_eval}
            print(f"alpha {alpha:5g} slowest gradient launch / fastest eval launch = {slowest / fastest_eval:.2f}; bar: < "
                  f"{EVALS_OF_CENTRAL_DIFFERENCES}", flush=True)
            result["alphas"][f"{alpha:g}"] = rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not all(rows["acceptance"]["faster_than_8_evals"] for rows in result["alphas"].values()):
        sys.exit("a gradient launch took longer than 8 eval launches")


if __name__ == "__main__":
    main()
