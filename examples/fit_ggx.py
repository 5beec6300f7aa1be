"""From samples to a GGX conductor: draws (wi, wo, rgb) samples of a known GGX material through eval, adds 1 % noise, fits
alpha, eta and k from a distant start (Levenberg-Marquardt with MerlHip.eval and MerlHip.ggx_grad: fit.fit_ggx) and prints the true
and the recovered parameters.

    python examples/fit_ggx.py [--log2n 18] [--iters 30] [--alpha 0.1]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mitsuba_customization_amd import fit, host  # noqa: E402

ETA, K = (0.143, 0.375, 1.442), (3.983, 2.386, 1.603)           # gold-like


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--noise", type=float, default=0.01)
    args = ap.parse_args()
    n = 1 << args.log2n
    eta, k = np.array(ETA), np.array(K)
    with host.MerlHip(0) as gpu:
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        mid = gpu.ggx(args.alpha, eta, k)
        rgb = gpu.eval(wi, wo, material=mid)                  # the "measurement" ...
        gpu.release_material(mid)
        torch.manual_seed(1)
        rgb = (rgb * (1.0 + args.noise * torch.randn_like(rgb))).contiguous()      # ... with multiplicative noise
        start = (3.0 * args.alpha, eta * 1.5, k * 0.7)
        a, e, kk, residuals = fit.fit_ggx(gpu, wi, wo, rgb, start, args.iters)
    for i, r in enumerate(residuals):
        print(f"iteration {i:3d}   |eval - y| = {r:.6e}")
    fmt = lambda v: " ".join(f"{x:8.5f}" for x in v)
    print(f"            alpha      eta (r g b)                  k (r g b)")
    print(f"true     {args.alpha:8.5f}   {fmt(eta)}   {fmt(k)}")
    print(f"start    {start[0]:8.5f}   {fmt(start[1])}   {fmt(start[2])}")
    print(f"fitted   {a:8.5f}   {fmt(e)}   {fmt(kk)}")


if __name__ == "__main__":
    main()
