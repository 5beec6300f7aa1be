"""Rates of mrl_ggx_pdf_grad_batch / _queue and mrl_ggx_sample_grad_batch / _queue on the gold-like metal at alpha 0.05
and 0.3: every form on 16.8 M units — whole arrays with every output, with the direction gradients only, material ids over four
materials, a dense ascending queue — with the forward mrl_pdf_batch and mrl_sample_batch launches on the same material and inputs in
the same process beside them.  The workaround the calls replace is central differences: 14 pdf launches (two per component of wi,
wo and one pair for alpha), 8 sample launches for (wi, alpha).  No ratio is required of these rates; what is measured is reported.
Device-resident generate_pairs inputs, events around the whole call, 3 warm-up + 10 timed launches, median [min, max].

    python tools/ggx_sample_grad_rates.py [--log2n 24] [--out profiles/ggx_sample_grad_rates.json]
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
FORWARD_LAUNCHES_OF_CENTRAL_DIFFERENCES = {"pdf": 14, "sample": 8}
# bytes a unit moves.  pdf: 24 in, 4 out; its gradient: 28 in, 12 + 12 + 4 out, + 4 with ids, + 4 with a queue.
# sample: 20 in, 28 out; its gradient: 48 in, 12 + 28 out, + 4 with ids, + 4 with a queue.
BYTES = {"mrl_pdf_batch (forward)": 28, "pdf: every output": 56, "pdf: grad_wi and grad_wo": 52, "pdf: material ids": 60, "pdf: queue": 60,
         "mrl_sample_batch (forward)": 48, "sample: both outputs": 88, "sample: grad_wi only": 60, "sample: material ids": 92, "sample: queue": 92}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ggx_sample_grad_rates.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    result = {"n": n, "eta": ETA, "k": K, "device": None, "library": host.build_info(), "warmup": 3, "steps": 10,
              "forward_launches_of_central_differences": FORWARD_LAUNCHES_OF_CENTRAL_DIFFERENCES, "bytes_per_unit": BYTES, "alphas": {}}
    with host.MerlHip(0) as gpu:
        result["device"] = gpu.device_name
        wi, wo, u = gpu.generate_pairs(0x5EED, 0, n)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
        gp, go = torch.randn((n,), dtype=torch.float32, device="cuda"), torch.randn((n, 7), dtype=torch.float32, device="cuda")
        pdf, wo2, pdf2, w2 = f32(n), f32(n, 3), f32(n), f32(n, 3)
        gwi, gwo, gal, gpar = f32(n, 3), f32(n, 3), f32(n), f32(n, 7)
        queue = torch.arange(n, dtype=torch.int32, device="cuda")
        count = torch.full((1,), n, dtype=torch.int32, device="cuda")
        for alpha in ALPHAS:
            mids = [gpu.ggx(alpha * s, ETA, K) for s in (1.0, 1.1, 1.2, 1.3)]
            mid = mids[0]
            mat = torch.tensor(mids, dtype=torch.int32, device="cuda")[torch.randint(0, 4, (n,), device="cuda")].contiguous()
            calls = {
                "mrl_pdf_batch (forward)": lambda: gpu.pdf(wi, wo, material=mid, out=pdf),
                "pdf: every output": lambda: gpu.ggx_pdf_grad(wi, wo, gp, material=mid, out=(gwi, gwo, gal)),
                "pdf: grad_wi and grad_wo": lambda: gpu.ggx_pdf_grad(wi, wo, gp, material=mid, want=("wi", "wo"), out=(gwi, gwo)),
                "pdf: material ids": lambda: gpu.ggx_pdf_grad(wi, wo, gp, mat=mat, out=(gwi, gwo, gal)),
                "pdf: queue": lambda: gpu.ggx_pdf_grad_queue(wi, wo, gp, queue, count, material=mid, out=(gwi, gwo, gal)),
                "mrl_sample_batch (forward)": lambda: gpu.sample(wi, u, material=mid, out=(wo2, pdf2, w2)),
                "sample: both outputs": lambda: gpu.ggx_sample_grad(wi, u, go, material=mid, out=(gwi, gpar)),
                "sample: grad_wi only": lambda: gpu.ggx_sample_grad(wi, u, go, material=mid, want="wi", out=gwi),
                "sample: material ids": lambda: gpu.ggx_sample_grad(wi, u, go, mat=mat, out=(gwi, gpar)),
                "sample: queue": lambda: gpu.ggx_sample_grad_queue(wi, u, go, queue, count, material=mid, out=(gwi, gpar)),
            }
            rows = {}
            for label, call in calls.items():
                ms = timed(gpu, call)
                med = statistics.median(ms)
                rows[label] = {"ms": ms, "median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "units_per_s": n / (med * 1e-3),
                               "GB_per_s": BYTES[label] * n / (med * 1e-3) / 1e9}
                print(f"alpha {alpha:5g} {label:28s} median {med:8.3f} ms  [{min(ms):.3f}, {max(ms):.3f}]  "
                      f"{n / (med * 1e-3) / 1e9:.3f} G units/s  {rows[label]['GB_per_s']:.0f} GB/s", flush=True)
            for m in mids:
                gpu.release_material(m)
            for kind, forward in (("pdf", "mrl_pdf_batch (forward)"), ("sample", "mrl_sample_batch (forward)")):
                slowest = max(row["median_ms"] for label, row in rows.items() if label.startswith(kind + ":"))
                rows[kind + ": slowest gradient launch / forward launch (medians)"] = slowest / rows[forward]["median_ms"]
                print(f"alpha {alpha:5g} {kind}: slowest gradient launch / forward launch = {slowest / rows[forward]['median_ms']:.2f}; central "
                      f"differences: {FORWARD_LAUNCHES_OF_CENTRAL_DIFFERENCES[kind]} forward launches", flush=True)
            result["alphas"][f"{alpha:g}"] = rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
