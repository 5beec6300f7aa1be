"""Rates of mrl_rgl_values_grad_batch and mrl_material_update_rgl_values: the plain planar-atomic kernel against the
gradient-brick kernel (wave-uniform merge choice, never merged, always merged) on random pairs, on a 2-degree cone and on one repeated
pair, for an isotropic 8 x 32 x 32 and an anisotropic 16 x 8 x 32 x 32 file, with mrl_eval_batch on the same inputs as the transform
floor; and the update in place against what there was before it, release + upload_rgl of the same values.  Device-resident arrays,
events around the whole call, 3 warm-up + 10 timed launches, median [min, max].

    python tools/rgl_values_grad_rates.py [--log2n 24] [--out profiles/rgl_values_grad_rates.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.table_grad_rates import ATOMIC_CEILING_TBS, VARIANTS, timed       # noqa: E402

FILES = {"isotropic 8 x 32 x 32": dict(seed=71, n_phi=1, n_theta=8, res=32), "anisotropic 16 x 8 x 32 x 32": dict(seed=72, n_phi=16, n_theta=8, res=32)}


def main():
    import torch
    from mitsuba_customization_amd import host, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgl_values_grad_rates.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    result = {"n": n, "device": None, "library": host.build_info(), "warmup": 3, "steps": 10, "atomic_ceiling_TBs": ATOMIC_CEILING_TBS,
              "note": "the ceiling is the guide's rate for contiguous global float atomics; units/s at the ceiling = ceiling / added bytes per unit: derived, not measured",
              "files": {}}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        g = torch.randn((n, 3), dtype=torch.float32, device="cuda")
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        wi_r, wo_r, _ = gpu.generate_pairs(0x5EED, 0, n)
        wi_c, wo_c = [torch.from_numpy(a).cuda() for a in synth.coherent_pairs(n)]
        wi_1, wo_1 = wi_c[:1].expand(n, 3).contiguous(), wo_c[:1].expand(n, 3).contiguous()
        sets = {"random_pairs": (wi_r, wo_r), "cone_2deg": (wi_c, wo_c), "one_pair": (wi_1, wo_1)}
        for file_name, kw in FILES.items():
            fields = synth.make_rgl_fields(**kw)
            mid = gpu.upload_rgl(fields)
            shape = gpu.rgl_values_shape(mid)
            slices = (2 if shape[0] > 1 else 1) * (2 if shape[1] > 1 else 1)
            added = 12 * slices * 8
            G = torch.zeros(int(np.prod(shape)), dtype=torch.float64, device="cuda")
            entry = {"shape": shape, "added_bytes_per_unit": added, "units_per_s_at_ceiling": ATOMIC_CEILING_TBS * 1e12 / added, "sets": {}}
            for name, (wi, wo) in sets.items():
                rows = {"mrl_eval_batch (floor)": {"ms": timed(gpu, lambda: gpu.eval(wi, wo, material=mid, out=rgb))}}
                for label, variant in VARIANTS.items():
                    gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
                    rows[label] = {"ms": timed(gpu, lambda: gpu.rgl_values_grad(wi, wo, g, [mid], material=mid, out=G))}
                gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)
                for label, row in rows.items():
                    med = statistics.median(row["ms"])
                    row.update({"median_ms": med, "min_ms": min(row["ms"]), "max_ms": max(row["ms"]), "units_per_s": n / (med * 1e-3)})
                    if "floor" not in label:
                        row["added_TBs"] = n * added / (med * 1e-3) / 1e12
                        row["fraction_of_atomic_ceiling"] = row["added_TBs"] / ATOMIC_CEILING_TBS
                    print(f"{file_name:30s} {name:14s} {label:26s} median {med:9.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  "
                          f"{row['units_per_s'] / 1e9:.3f} G units/s", flush=True)
                naive, ship = rows["naive_planar_atomics"], rows["bricks_auto (shipped)"]
                never, always = rows["bricks_never_merged"], rows["bricks_always_merged"]
                spread = ship["max_ms"] - ship["min_ms"]
                rows["acceptance"] = {"shipped_faster_than_naive": ship["max_ms"] < naive["min_ms"], "speedup_median": naive["median_ms"] / ship["median_ms"],
                                      "auto_not_slower_than_both_fixed_by_more_than_its_spread":
                                          ship["median_ms"] <= max(never["median_ms"], always["median_ms"]) + spread}
                entry["sets"][name] = rows
            # the update in place (from a device tensor: launches only; from a host array: staged) against release + upload
            new = np.ascontiguousarray(fields["rgb"], np.float32)
            dnew = torch.from_numpy(new).cuda()
            upd = {"update_rgl_values (device pointer)": {"ms": timed(gpu, lambda: gpu.update_rgl_values(mid, dnew))}}
            wall = []
            for _ in range(5):
                gpu.synchronize(); t0 = time.perf_counter(); gpu.update_rgl_values(mid, new); gpu.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
            upd["update_rgl_values (host array, wall clock)"] = {"ms": wall}
            wall = []
            for _ in range(5):
                gpu.synchronize(); t0 = time.perf_counter(); gpu.release_material(mid); mid = gpu.upload_rgl(fields); gpu.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            upd["release + upload_rgl (wall clock)"] = {"ms": wall}
            for label, row in upd.items():
                row.update({"median_ms": statistics.median(row["ms"]), "min_ms": min(row["ms"]), "max_ms": max(row["ms"])})
                print(f"{file_name:30s} {label:44s} median {row['median_ms']:9.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]", flush=True)
            entry["update"] = upd
            result["files"][file_name] = entry
            gpu.release_material(mid)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
