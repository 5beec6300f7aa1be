"""Rates of mrl_rgl_grad_dir_batch on two synthetic RGL files of the database's shapes — isotropic (n_theta = 8,
res 32) and anisotropic (n_phi = 8, n_theta = 8, res 32) —, 16.8 M device-resident generate_pairs units: whole arrays with both
gradients, grad_wo only, material ids and a dense ascending queue, with mrl_eval_batch on the same file and inputs in the same
process as the baseline: the workaround the call replaces is central differences, 8 eval launches (two per tangent direction of wi
and of wo).  Events around the whole call, 3 warm-up + 10 timed launches, median [min, max].  No ratio is a bar: what is measured is
recorded.

    python tools/rgl_dir_grad_rates.py [--log2n 24] [--out profiles/rgl_dir_grad_rates.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EVALS_OF_CENTRAL_DIFFERENCES = 8
BASELINE = "mrl_eval_batch (baseline)"
FILES = {"isotropic": dict(seed=11, n_phi=1, n_theta=8, res=32, res_ndf=128, res_sigma=32),
         "anisotropic": dict(seed=12, n_phi=8, n_theta=8, res=32, res_ndf=128, res_sigma=32)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgl_dir_grad_rates.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    result = {"n": n, "device": None, "library": host.build_info(), "warmup": 3, "steps": 10,
              "evals_of_central_differences": EVALS_OF_CENTRAL_DIFFERENCES, "files": {}}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        g = torch.randn((n, 3), dtype=torch.float32, device="cuda")
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        gwi, gwo = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
        queue = torch.arange(n, dtype=torch.int32, device="cuda")
        count = torch.full((1,), n, dtype=torch.int32, device="cuda")
        for name, shape in FILES.items():
            mid = gpu.upload_rgl(synth.make_rgl_fields(**shape))
            mat = torch.full((n,), mid, dtype=torch.int32, device="cuda")
            rows = {
                BASELINE: {"ms": timed(gpu, lambda: gpu.eval(wi, wo, material=mid, out=rgb))},
                "both gradients": {"ms": timed(gpu, lambda: gpu.rgl_grad_dir(wi, wo, g, material=mid, out=(gwi, gwo)))},
                "grad_wo only": {"ms": timed(gpu, lambda: gpu.rgl_grad_dir(wi, wo, g, material=mid, want="wo", out=gwo))},
                "material ids": {"ms": timed(gpu, lambda: gpu.rgl_grad_dir(wi, wo, g, mat=mat, out=(gwi, gwo)))},
                "queue": {"ms": timed(gpu, lambda: gpu.rgl_grad_dir_queue(wi, wo, g, queue, count, material=mid, out=(gwi, gwo)))},
            }
            for label, row in rows.items():
                med = statistics.median(row["ms"])
                row.update({"median_ms": med, "min_ms": min(row["ms"]), "max_ms": max(row["ms"]), "units_per_s": n / (med * 1e-3),
                            "eval_launches": med / statistics.median(rows[BASELINE]["ms"])})
                print(f"{name:12s} {label:26s} median {med:8.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  "
                      f"{row['units_per_s'] / 1e9:.3f} G units/s  = {row['eval_launches']:.2f} eval launches "
                      f"(central differences: {EVALS_OF_CENTRAL_DIFFERENCES})", flush=True)
            result["files"][name] = {"shape": shape, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
