"""Rates of mrl_table_grad_batch_nch beside what a user had before it: ceil(n_ch / 3) calls of mrl_table_grad_batch on
channel triplets, the column gather included (the last triplet padded with zeros).  n_ch in {4, 16, 32} on random pairs, on a
coherent set and on one repeated pair.  The method of tools/table_grad_rates.py: MERL dims, trilinear, device-resident arrays, events
around the whole call, 3 warm-up + 10 timed launches, median [min, max].  A row counts as different only when the slowest launch of
one side beats the fastest of the other.

    python tools/table_grad_nch_rates.py [--log2n 24] [--out profiles/table_grad_nch_rates.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from table_grad_rates import ATOMIC_CEILING_TBS, timed             # noqa: E402

WIDTHS = (4, 16, 32)


def main():
    import torch
    from mitsuba_customization_amd import host, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_grad_nch_rates.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    dims = (90, 90, 180)
    result = {"n": n, "dims": dims, "lookup": "trilinear", "device": None, "library": host.build_info(), "warmup": 3, "steps": 10,
              "atomic_ceiling_TBs": ATOMIC_CEILING_TBS, "widths": {}}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        wi_r, wo_r, _ = gpu.generate_pairs(0x5EED, 0, n)
        wi_c, wo_c = [torch.from_numpy(a).cuda() for a in synth.coherent_pairs(n)]
        wi_1, wo_1 = wi_c[:1].expand(n, 3).contiguous(), wo_c[:1].expand(n, 3).contiguous()
        sets = {"random_pairs": (wi_r, wo_r), "coherent_2deg_cone": (wi_c, wo_c), "one_cell": (wi_1, wo_1)}
        rgb = gpu.upload_table(np.ones((3,) + dims), (1.0, 1.0, 1.0))
        for n_ch in WIDTHS:
            triplets = -(-n_ch // 3)
            mid = gpu.upload_table_nch(np.ones((n_ch,) + dims))
            g = torch.randn((n, n_ch), dtype=torch.float32, device="cuda")
            G = torch.zeros(n_ch * dims[0] * dims[1] * dims[2], dtype=torch.float64, device="cuda")
            G3 = torch.zeros((triplets, 3) + dims, dtype=torch.float64, device="cuda")
            cols = torch.zeros((n, 3), dtype=torch.float32, device="cuda")

            def one_call():
                gpu.table_grad_nch(wi, wo, g, n_ch, [mid], material=mid, out=G)

            def triplet_calls():
                for t in range(triplets):
                    width = min(3, n_ch - 3 * t)
                    if width < 3:
                        cols.zero_()
                    cols[:, :width] = g[:, 3 * t:3 * t + width]
                    gpu.table_grad(wi, wo, cols, material=rgb, out=G3[t])
            rows = {}
            for name, (wi, wo) in sets.items():
                one, today = timed(gpu, one_call), timed(gpu, triplet_calls)
                row = {"one_call_ms": one, "triplet_calls_ms": today, "triplet_calls": triplets,
                       "added_bytes_per_unit": {"one_call": 64 * n_ch, "triplet_calls": 192 * triplets}}
                for side, ms, added in (("one_call", one, 64 * n_ch), ("triplet_calls", today, 192 * triplets)):
                    med = statistics.median(ms)
                    row[side] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "units_per_s": n / (med * 1e-3),
                                 "added_TBs": n * added / (med * 1e-3) / 1e12}
                a, b = row["one_call"], row["triplet_calls"]
                row["verdict"] = "one call faster" if a["max_ms"] < b["min_ms"] else ("triplet calls faster" if b["max_ms"] < a["min_ms"] else "no difference")
                row["speedup_median"] = b["median_ms"] / a["median_ms"]
                rows[name] = row
                print(f"n_ch {n_ch:2d} {name:20s} one call {a['median_ms']:9.3f} ms [{a['min_ms']:.3f}, {a['max_ms']:.3f}] {a['added_TBs']:.2f} TB/s | "
                      f"{triplets} triplet calls {b['median_ms']:9.3f} ms [{b['min_ms']:.3f}, {b['max_ms']:.3f}] {b['added_TBs']:.2f} TB/s | {row['verdict']}", flush=True)
            result["widths"][str(n_ch)] = rows
            gpu.release_material(mid)
            del g, G, G3, cols
        # the RGB call on the same inputs: its unit is untouched by the n-channel kernels
        g3 = torch.randn((n, 3), dtype=torch.float32, device="cuda")
        G3 = torch.zeros((3,) + dims, dtype=torch.float64, device="cuda")
        ms = timed(gpu, lambda: gpu.table_grad(wi_r, wo_r, g3, material=rgb, out=G3))
        result["mrl_table_grad_batch_random_pairs"] = {"ms": ms, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
        print(f"mrl_table_grad_batch, random pairs: median {statistics.median(ms):.3f} ms [{min(ms):.3f}, {max(ms):.3f}]", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
