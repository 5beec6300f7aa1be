"""Rates of mrl_rgl_spectral_values_grad_batch and mrl_material_update_rgl_spectral_values: the plain planar-atomic
kernel (the baseline) against the gradient-brick kernel (wave-uniform merge choice, never merged, always merged) on random pairs, on a
2-degree cone and on one repeated pair, at W = 4 and 16 hero wavelengths per unit, for an isotropic 8 x 32 x 32 and an anisotropic
16 x 8 x 32 x 32 file of 32 wavelength nodes each, with mrl_eval_spectral_batch on the same inputs as the transform floor; and the
update in place against what there was before it, release + upload_rgl of the same spectra.  Device-resident arrays, events around the
whole call, 3 warm-up + 10 timed launches, median [min, max].  Every (file, W) step runs as a process of its own under `timeout`; a
step that fails ends the run.

    python tools/rgl_spectral_values_grad_rates.py [--log2n 21] [--out profiles/rgl_spectral_values_grad_rates.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.table_grad_rates import VARIANTS, timed       # noqa: E402

NODES = 32
FILES = {"isotropic 8 x 32 x 32": dict(seed=71, n_phi=1, n_theta=8, res=32, n_wavelengths=NODES),
         "anisotropic 16 x 8 x 32 x 32": dict(seed=72, n_phi=16, n_theta=8, res=32, n_wavelengths=NODES)}
WS = (4, 16)
STEP_SECONDS = 300


def step(file_name, W, log2n):
    import torch
    from mitsuba_customization_amd import host, synth
    n = 1 << log2n
    out = {"sets": {}}
    with host.MerlHip(0) as gpu:
        out["device"], out["library"] = gpu.device_name, host.build_info()
        fields = synth.make_rgl_fields(**FILES[file_name])
        mid = gpu.upload_rgl(fields)
        shape = gpu.rgl_spectral_values_shape(mid)
        slices = (2 if shape[0] > 1 else 1) * (2 if shape[1] > 1 else 1)
        out["shape"] = shape
        out["added_bytes_per_unit"] = W * 2 * 4 * slices * 8       # two nodes per wavelength, 4 S doubles each
        out["workspace_bytes"] = max(shape[0] - 1, 1) * max(shape[1] - 1, 1) * (shape[3] - 1) * (shape[4] - 1) * shape[2] * slices * 32
        nodes = np.asarray(fields["wavelengths"], np.float32)
        g = torch.randn((n, W), dtype=torch.float32, device="cuda")
        wl = (torch.rand((n, W), dtype=torch.float32, device="cuda") * float(nodes[-1] - nodes[0]) + float(nodes[0])).contiguous()
        values = torch.empty((n, W), dtype=torch.float32, device="cuda")
        wi_r, wo_r, _ = gpu.generate_pairs(0x5EED, 0, n)
        wi_c, wo_c = [torch.from_numpy(a).cuda() for a in synth.coherent_pairs(n)]
        wi_1, wo_1 = wi_c[:1].expand(n, 3).contiguous(), wo_c[:1].expand(n, 3).contiguous()
        G = torch.zeros(int(np.prod(shape)), dtype=torch.float64, device="cuda")
        for name, (wi, wo) in {"random_pairs": (wi_r, wo_r), "cone_2deg": (wi_c, wo_c), "one_pair": (wi_1, wo_1)}.items():
            rows = {"mrl_eval_spectral_batch (floor)": {"ms": timed(gpu, lambda: gpu.eval_spectral(wi, wo, wl, material=mid, out=values))}}
            for label, variant in VARIANTS.items():
                gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
                rows[label] = {"ms": timed(gpu, lambda: gpu.rgl_spectral_values_grad(wi, wo, wl, g, [mid], material=mid, out=G))}
            gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)
            for label, row in rows.items():
                med = statistics.median(row["ms"])
                row.update({"median_ms": med, "min_ms": min(row["ms"]), "max_ms": max(row["ms"]), "units_per_s": n / (med * 1e-3)})
                print(f"{file_name:30s} W {W:2d} {name:14s} {label:32s} median {med:9.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  "
                      f"{row['units_per_s'] / 1e9:.3f} G units/s", flush=True)
            naive, ship = rows["naive_planar_atomics"], rows["bricks_auto (shipped)"]
            rows["comparison"] = {"shipped_faster_than_plain": ship["max_ms"] < naive["min_ms"], "plain_over_shipped_median": naive["median_ms"] / ship["median_ms"]}
            out["sets"][name] = rows
        if W == WS[0]:
            # the update in place (from a device tensor: launches only; from a host array: staged) against release + upload
            new = np.ascontiguousarray(fields["spectra"], np.float32)
            dnew = torch.from_numpy(new).cuda()
            upd = {"update_rgl_spectral_values (device pointer)": {"ms": timed(gpu, lambda: gpu.update_rgl_spectral_values(mid, dnew))}}
            wall = []
            for _ in range(5):
                gpu.synchronize(); t0 = time.perf_counter(); gpu.update_rgl_spectral_values(mid, new); gpu.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
            upd["update_rgl_spectral_values (host array, wall clock)"] = {"ms": wall}
            wall = []
            for _ in range(5):
                gpu.synchronize(); t0 = time.perf_counter(); gpu.release_material(mid); mid = gpu.upload_rgl(fields); gpu.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            upd["release + upload_rgl (wall clock)"] = {"ms": wall}
            for label, row in upd.items():
                row.update({"median_ms": statistics.median(row["ms"]), "min_ms": min(row["ms"]), "max_ms": max(row["ms"])})
                print(f"{file_name:30s} {label:52s} median {row['median_ms']:9.3f} ms  [{row['min_ms']:.3f}, {row['max_ms']:.3f}]", flush=True)
            out["update"] = upd
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgl_spectral_values_grad_rates.json"))
    ap.add_argument("--step", nargs=2, metavar=("FILE", "W"), help="one (file, W) step, written to --out (what the run starts under timeout)")
    args = ap.parse_args()
    if args.step:
        with open(args.out, "w") as f:
            json.dump(step(args.step[0], int(args.step[1]), args.log2n), f)
        return 0
    result = {"n": 1 << args.log2n, "device": None, "library": None, "warmup": 3, "steps": 10, "nodes": NODES, "files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for file_name in FILES:
            entry = {"W": {}}
            for W in WS:
                part = os.path.join(tmp, "step.json")
                rc = subprocess.call(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--log2n", str(args.log2n),
                                      "--out", part, "--step", file_name, str(W)])
                if rc != 0:                                        # nothing more is started on the device after a failed step
                    print(f"step ({file_name}, W = {W}) ended with status {rc}: stopping", flush=True)
                    return rc
                with open(part) as f:
                    one = json.load(f)
                result["device"], result["library"] = one.pop("device"), one.pop("library")
                for k in ("shape", "workspace_bytes"):
                    entry[k] = one.pop(k)
                if "update" in one:
                    entry["update"] = one.pop("update")
                entry["W"][str(W)] = one
            result["files"][file_name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
