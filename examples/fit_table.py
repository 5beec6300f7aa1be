"""From samples to a table: draws (wi, wo, rgb) samples of a synthetic GGX-shaped table through eval, fits a fresh table to
them (normalised splat, then CGLS with MerlHip.eval as A and MerlHip.table_grad as A^T), prints the residuals and writes the
result as a MERL-layout .binary.

    python examples/fit_table.py [--log2n 20] [--iters 20] [--out fitted.binary]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mitsuba_customization_amd import fit, host, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dims", type=int, nargs=3, default=(24, 24, 48))
    ap.add_argument("--out", default="fitted.binary")
    args = ap.parse_args()
    dims, n = tuple(args.dims), 1 << args.log2n
    truth = synth.make_table("ggx_tab", 0, dims)
    with host.MerlHip(0) as gpu:
        gpu.set_option(host.OPT_NEGATIVE, 1)                  # keep: eval stays linear in the iterates (fit.py)
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        mid = gpu.upload_table(truth)
        rgb = gpu.eval(wi, wo, material=mid)                  # the "measurement"
        gpu.release_material(mid)
        table, residuals = fit.fit_table(gpu, dims, wi, wo, rgb, args.iters)
        norm = float((rgb.double() ** 2).sum()) ** 0.5
    for k, r in enumerate(residuals):
        print(f"iteration {k:3d}   |A T - y| = {r:.6e}   relative {r / norm:.3e}")
    synth.write_merl_binary(args.out, table.cpu().numpy())
    print(f"wrote {args.out}: dims {dims}, {n} samples")


if __name__ == "__main__":
    main()
