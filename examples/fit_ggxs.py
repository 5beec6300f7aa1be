"""Several GGX conductors from one capture session: draws (wi, wo, material, rgb) samples of three known conductors — interleaved,
a material index per sample, as a wavefront renderer's hit queue holds them — through the device's own f32 eval, and fits all three
at once with fit.fit_ggx_mat: per Levenberg-Marquardt iteration one eval with material ids and one MerlHip.ggx_grad_mat launch,
whatever the number of materials.  Prints every material's residuals and its true, starting and recovered parameters.

    python examples/fit_ggxs.py [--log2n 18] [--iters 30]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mitsuba_customization_amd import fit, host  # noqa: E402

# (alpha, eta, k) of the truth, and the factors (alpha, eta, k) its fit starts from
CONDUCTORS = (((0.1, (0.143, 0.375, 1.442), (3.983, 2.386, 1.603)), (3.0, 1.5, 0.7)),        # gold-like
              ((0.2, (1.5, 1.45, 1.55), (7.6, 7.5, 7.7)), (1.5, 1.5, 0.7)),                 # aluminium-like
              ((0.1, (0.8, 1.1, 1.3), (0.3, 3.0, 30.0)), (2.0, 1.2, 0.9)))                  # k spread over two decades


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    n = 1 << args.log2n
    truths = [(a, np.array(e), np.array(k)) for (a, e, k), _ in CONDUCTORS]
    starts = [(a * fa, e * fe, k * fk) for (a, e, k), (_, (fa, fe, fk)) in zip(truths, CONDUCTORS)]
    with host.MerlHip(0) as gpu:
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        mat = torch.randint(0, len(CONDUCTORS), (n,), device=wi.device, dtype=torch.int32)
        ids = [gpu.ggx(a, e, k) for a, e, k in truths]
        rgb = gpu.eval(wi, wo, mat=fit._unit_ids(mat, ids))   # the "measurement": every sample through its own material
        for mid in ids:
            gpu.release_material(mid)
        fits = fit.fit_ggx_mat(gpu, wi, wo, mat, rgb, starts, args.iters)
    fmt = lambda v: " ".join(f"{x:8.5f}" for x in v)
    for j, ((a, e, k), start, (fa, fe, fk, residuals)) in enumerate(zip(truths, starts, fits)):
        print(f"material {j}: |eval - y| {residuals[0]:.4e} -> {residuals[-1]:.4e} in {args.iters} iterations")
        print(f"            alpha      eta (r g b)                  k (r g b)")
        print(f"true     {a:8.5f}   {fmt(e)}   {fmt(k)}")
        print(f"start    {start[0]:8.5f}   {fmt(start[1])}   {fmt(start[2])}")
        print(f"fitted   {fa:8.5f}   {fmt(fe)}   {fmt(fk)}")


if __name__ == "__main__":
    main()
