"""What it costs to make a fit's iterate resident: MerlHip.update_table — from a device tensor with and without the
sampling rebuilds, from a host array — beside what fit.py did before it, release_material + upload_table of a device-tensor iterate
(the D2H copy of the iterate included); and one CGLS iteration of fit_table on 2^24 pairs both ways.  MERL dims, an RGB table and an
n-channel table of 16 channels.  Every figure is host wall time around work that ends in a stream synchronise — the old path's cost is
host work (copies, allocations, the marginal's loop), which device events do not see — 3 warm-up + 10 timed runs in this one fresh
process, median [min, max].  A pair of rows counts as different only when the slowest run of one side beats the fastest of the other.

    python tools/update_rates.py [--log2n 24] [--out profiles/update_rates.json]
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

WARMUP, STEPS = 3, 10
DIMS = (90, 90, 180)


def timed(gpu, fn):
    import torch
    ms = []
    for k in range(WARMUP + STEPS):
        torch.cuda.synchronize(); gpu.synchronize()
        t0 = time.perf_counter()
        fn()
        gpu.synchronize(); torch.cuda.synchronize()
        if k >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def row(ms, **more):
    return dict(ms=ms, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), **more)


def verdict(new, old):
    return "update faster" if new["max_ms"] < old["min_ms"] else ("upload path faster" if old["max_ms"] < new["min_ms"] else "no difference")


def table_rows(gpu, n_ch):
    """the ways to make one iterate resident, for a table of n_ch channels (3: the RGB path)"""
    import torch
    cells = DIMS[0] * DIMS[1] * DIMS[2]
    scale = (1.0, 1.0, 1.0) if n_ch == 3 else None
    upload = (lambda t: gpu.upload_table(t, scale)) if n_ch == 3 else (lambda t: gpu.upload_table_nch(t, scale))
    iterate = torch.randn((n_ch,) + DIMS, dtype=torch.float64, device="cuda")
    on_host = iterate.cpu().numpy()
    work = upload(np.ones((n_ch,) + DIMS))
    held = [upload(np.ones((n_ch,) + DIMS))]

    def parent_path():                                          # what fit.py's A() did, its eval left out
        gpu.release_material(held.pop())
        held.append(upload(iterate.cpu().numpy()))
    image_bytes = gpu.memory_info()["table_bytes"] // 2         # two tables of this shape are resident
    out = {
        "update_device_keep_sampling": row(timed(gpu, lambda: gpu.update_table(work, iterate, keep_sampling=True))),
        "update_device": row(timed(gpu, lambda: gpu.update_table(work, iterate))),
        "update_host_keep_sampling": row(timed(gpu, lambda: gpu.update_table(work, on_host, keep_sampling=True))),
        "update_host": row(timed(gpu, lambda: gpu.update_table(work, on_host))),
        "release_upload_of_device_iterate": row(timed(gpu, parent_path)),
        "upload_from_host_array_alone": row(timed(gpu, lambda: (gpu.release_material(held.pop()), held.append(upload(on_host))))),
    }
    # the floor of a device-source update is its traffic: the planar array read once, the image written once
    traffic = n_ch * cells * 8 + image_bytes
    for name in ("update_device_keep_sampling", "update_device"):
        out[name]["traffic_bytes"] = traffic
        out[name]["traffic_GBs_at_median"] = traffic / (out[name]["median_ms"] * 1e-3) / 1e9
    out["planar_bytes"], out["image_bytes"] = n_ch * cells * 8, image_bytes
    out["verdict_device_keep_vs_release_upload"] = verdict(out["update_device_keep_sampling"], out["release_upload_of_device_iterate"])
    out["verdict_device_vs_release_upload"] = verdict(out["update_device"], out["release_upload_of_device_iterate"])
    out["verdict_host_vs_upload_alone"] = verdict(out["update_host"], out["upload_from_host_array_alone"])
    for name, r in out.items():
        if isinstance(r, dict):
            print(f"n_ch {n_ch:2d} {name:36s} median {r['median_ms']:9.3f} ms [{r['min_ms']:.3f}, {r['max_ms']:.3f}]", flush=True)
    gpu.release_material(work); gpu.release_material(held.pop())
    return out


def cgls_rows(gpu, n):
    """one CGLS iteration of fit_table (fit._cgls's loop body) with the iterate made resident the old way and in place"""
    import torch
    from mitsuba_customization_amd import fit, host
    scale = (1.0, 1.0, 1.0)
    wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
    shape_mid = gpu.upload_table(np.ones((3,) + DIMS), scale)
    work_mid = gpu.upload_table(np.ones((3,) + DIMS), scale)

    def A_in_place(table):
        gpu.update_table(work_mid, table.contiguous(), keep_sampling=True)
        return gpu.eval(wi, wo, material=work_mid).double()

    def A_release_upload(table):                                # fit.py before this section
        mid = gpu.upload_table(table.cpu().numpy(), scale)
        try:
            return gpu.eval(wi, wo, material=mid).double()
        finally:
            gpu.release_material(mid)

    def At(r):
        return gpu.table_grad(wi, wo, r.float().contiguous(), material=shape_mid)

    out = {}
    for name, A in (("in_place", A_in_place), ("release_upload", A_release_upload)):
        x = torch.rand((3,) + DIMS, dtype=torch.float64, device="cuda")
        r = torch.randn((n, 3), dtype=torch.float64, device="cuda")
        s = At(r)
        state = {"x": x, "r": r, "p": s, "gamma": fit._dot(s, s)}

        def iteration():
            q = A(state["p"])
            alpha = state["gamma"] / fit._dot(q, q)
            state["x"] = state["x"] + alpha * state["p"]
            state["r"] = state["r"] - alpha * q
            s = At(state["r"])
            gamma_new = fit._dot(s, s)
            state["p"] = s + (gamma_new / state["gamma"]) * state["p"]
            state["gamma"] = gamma_new
        out[name] = row(timed(gpu, iteration))
        print(f"fit_table CGLS iteration, {name:16s} median {out[name]['median_ms']:9.3f} ms [{out[name]['min_ms']:.3f}, {out[name]['max_ms']:.3f}]", flush=True)
    # the iteration's own kernels, for scale (device events)
    g32 = torch.randn((n, 3), dtype=torch.float32, device="cuda")
    G = torch.zeros((3,) + DIMS, dtype=torch.float64, device="cuda")
    out["eval_alone"] = row(timed(gpu, lambda: gpu.eval(wi, wo, material=work_mid)))
    out["table_grad_alone"] = row(timed(gpu, lambda: gpu.table_grad(wi, wo, g32, material=shape_mid, out=G)))
    out["verdict"] = "in place faster" if out["in_place"]["max_ms"] < out["release_upload"]["min_ms"] else (
        "release + upload faster" if out["release_upload"]["max_ms"] < out["in_place"]["min_ms"] else "no difference")
    return out


def main():
    from mitsuba_customization_amd import host
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_rates.json"))
    args = ap.parse_args()
    result = {"dims": DIMS, "device": None, "library": host.build_info(), "warmup": WARMUP, "steps": STEPS,
              "clock": "host wall time around work that ends in a stream synchronise", "tables": {}}
    with host.MerlHip(0) as gpu:
        gpu.set_option(host.OPT_NEGATIVE, host.NEGATIVE_KEEP)   # what fit_table runs under
        result["device"] = gpu.device_name
        for n_ch in (3, 16):
            result["tables"][str(n_ch)] = table_rows(gpu, n_ch)
        result["fit_table_cgls_iteration"] = dict(n=1 << args.log2n, **cgls_rows(gpu, 1 << args.log2n))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
