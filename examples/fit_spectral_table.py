"""From spectral samples to a table: draws (wi, wo, 16 values) samples of a synthetic 16-channel GGX-shaped table through eval_nch,
fits a fresh 16-channel table to them (normalised splat, then CGLS with MerlHip.eval_nch as A and MerlHip.table_grad_nch as A^T —
one launch serves all channels), prints the residuals and writes the result as a customized_measurement file of 16 planes.

    python examples/fit_spectral_table.py [--log2n 20] [--iters 20] [--channels 16] [--out fitted_spectral.binary]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mitsuba_customization_amd import fit, host, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--dims", type=int, nargs=3, default=(24, 24, 48))
    ap.add_argument("--out", default="fitted_spectral.binary")
    args = ap.parse_args()
    dims, n, n_ch = tuple(args.dims), 1 << args.log2n, args.channels
    truth = synth.make_table_nch("spectral", n_ch, 0, dims)
    with host.MerlHip(0) as gpu:
        gpu.set_option(host.OPT_NEGATIVE, 1)                  # keep: eval stays linear in the iterates (fit.py)
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        mid = gpu.upload_table_nch(truth)
        values = gpu.eval_nch(wi, wo, n_ch, material=mid)     # the "measurement"
        gpu.release_material(mid)
        table, residuals = fit.fit_table_nch(gpu, dims, wi, wo, values, args.iters)
        norm = float((values.double() ** 2).sum()) ** 0.5
    for k, r in enumerate(residuals):
        print(f"iteration {k:3d}   |A T - y| = {r:.6e}   relative {r / norm:.3e}")
    synth.write_table_nch(args.out, table.cpu().numpy())
    print(f"wrote {args.out}: {n_ch} channels, dims {dims}, {n} samples")


if __name__ == "__main__":
    main()
