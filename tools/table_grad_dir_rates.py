"""Rates of mrl_table_grad_dir_batch / mrl_table_grad_dir_queue on a 'ggx_tab' table at MERL dims: whole arrays with
both gradients, whole arrays with grad_wo only, material ids over four tables, a dense ascending queue — with mrl_eval_batch on the same
material and inputs in the same process as the baseline: the workaround the calls replace is central differences, at least 8 eval
launches (two per tangent direction of wi and of wo).  Two input sets: device-resident generate_pairs units (every lookup another
128-B line) and synth.coherent_pairs (a 2-degree cone around one mirror direction).  Events around the whole call, 3 warm-up + 10 timed
launches, median [min, max].

    python tools/table_grad_dir_rates.py [--log2n 24] [--out profiles/table_grad_dir_rates.json]
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
# bytes a unit moves in streams: wi, wo, grad_rgb in (36), + 4 with ids, + 4 with a queue; 12 out per gradient.  eval: 24 in, 12 out.
# Every unit also reads one neighbourhood of the table: a 128-B line of the brick layout when the lookups are incoherent.
STREAM_BYTES = {BASELINE: 36, "both gradients": 60, "grad_wo only": 48, "material ids": 64, "queue": 64}
LINE_BYTES = 128


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_grad_dir_rates.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    result = {"n": n, "table": "synth.ggx_tab_table(seed) at 90 x 90 x 180, brick layout", "device": None, "library": host.build_info(),
              "warmup": 3, "steps": 10, "evals_of_central_differences": EVALS_OF_CENTRAL_DIFFERENCES, "stream_bytes_per_unit": STREAM_BYTES,
              "table_bytes_per_incoherent_unit": LINE_BYTES, "inputs": {}}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        mids = [gpu.upload_merl(synth.ggx_tab_table(seed)) for seed in range(4)]
        mid = mids[0]
        g = torch.randn((n, 3), dtype=torch.float32, device="cuda")
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        gwi, gwo = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
        queue = torch.arange(n, dtype=torch.int32, device="cuda")
        count = torch.full((1,), n, dtype=torch.int32, device="cuda")
        mat = torch.tensor(mids, dtype=torch.int32, device="cuda")[torch.randint(0, 4, (n,), device="cuda")].contiguous()
        for name in ("generate_pairs", "coherent_pairs"):
            if name == "generate_pairs":
                wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
            else:
                wi, wo = (torch.from_numpy(x).cuda() for x in synth.coherent_pairs(n))
            rows = {
                BASELINE: {"ms": timed(gpu, lambda: gpu.eval(wi, wo, material=mid, out=rgb))},
                "both gradients": {"ms": timed(gpu, lambda: gpu.table_grad_dir(wi, wo, g, material=mid, out=(gwi, gwo)))},
                "grad_wo only": {"ms": timed(gpu, lambda: gpu.table_grad_dir(wi, wo, g, material=mid, want="wo", out=gwo))},
                "material ids": {"ms": timed(gpu, lambda: gpu.table_grad_dir(wi, wo, g, mat=mat, out=(gwi, gwo)))},
                "queue": {"ms": timed(gpu, lambda: gpu.table_grad_dir_queue(wi, wo, g, queue, count, material=mid, out=(gwi, gwo)))},
            }
            for label, row in rows.items():
                med = statistics.median(row["ms"])
                row.update({"median_ms": med, "min_ms": min(row["ms"]), "max_ms": max(row["ms"]), "units_per_s": n / (med * 1e-3),
                            "stream_TB_per_s": STREAM_BYTES[label] * n / (med * 1e-3) / 1e12,
                            "stream_plus_line_TB_per_s": (STREAM_BYTES[label] + LINE_BYTES) * n / (med * 1e-3) / 1e12})
                print(f"{name:15s} {label:26s} median {med:8.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  "
                      f"{row['units_per_s'] / 1e9:.3f} G units/s  streams {row['stream_TB_per_s']:.2f} TB/s  "
                      f"with a line per unit {row['stream_plus_line_TB_per_s']:.2f} TB/s", flush=True)
            fastest_eval = rows[BASELINE]["min_ms"]
            slowest = max(row["max_ms"] for label, row in rows.items() if label != BASELINE)
            rows["acceptance"] = {"slowest_gradient_over_fastest_eval": slowest / fastest_eval,
                                  "faster_than_8_evals": slowest <= EVALS_OF_CENTRAL_DIFFERENCES * fastest_eval}
            print(f"{name:15s} slowest gradient launch / fastest eval launch = {slowest / fastest_eval:.2f}; bar: <= "
                  f"{EVALS_OF_CENTRAL_DIFFERENCES}", flush=True)
            result["inputs"][name] = rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not all(rows["acceptance"]["faster_than_8_evals"] for rows in result["inputs"].values()):
        sys.exit("a gradient launch took longer than 8 eval launches")


if __name__ == "__main__":
    main()
