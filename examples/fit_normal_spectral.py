"""From measurements to a shading normal THROUGH A MEASURED SPECTRAL BRDF: the Gauss-Newton fit of examples/fit_normal.py with a
16-channel table behind it.  The surface is synth's 'spectral' table at MERL dims (90 x 90 x 180, half / difference angles, 16
wavelength-like channels); the local directions R(p) wi, R(p) wo go through diff.table_eval_nch, whose backward pass
(MerlHip.table_grad_dir_nch, one call) hands d eval / d direction back to torch — one backward pass per channel for the Jacobian of
the residuals.  The objective is piecewise smooth, as in examples/fit_normal_table.py: the line search of fit_normal.fit is what
guarantees a loss that does not rise; no convergence rate is promised.

    python examples/fit_normal_spectral.py [--log2n 16] [--iters 8] [--seed 0] [--channels 16]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fit_normal import TRUTH, fit, rotation            # noqa: E402


def fit_spectral(gpu, material, n_channels, wi, wo, iters=8):
    """wi, wo: local direction pairs [n, 3] on the device, as the TRUE frame sees them.  Returns fit_normal.fit's (angles, loss
    history, angle-error history) for the n-channel table `material` of the context `gpu`."""
    from mitsuba_customization_amd import diff
    r = rotation(torch.tensor(TRUTH, dtype=torch.float64)).to(wi.device)
    wi_w, wo_w = wi.to(torch.float64) @ r, wo.to(torch.float64) @ r
    return fit(lambda a, b: diff.table_eval_nch(gpu, a, b, n_channels, material=material), wi_w, wo_w, iters=iters)


def main():
    from mitsuba_customization_amd import host, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=16)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--channels", type=int, default=16)
    args = ap.parse_args()
    with host.MerlHip(0) as gpu:
        mid = gpu.upload_table_nch(synth.make_table_nch("spectral", args.channels, args.seed))
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, 1 << args.log2n)
        angles, history, errors = fit_spectral(gpu, mid, args.channels, wi, wo, iters=args.iters)
    for i, (loss, err) in enumerate(zip(history, errors)):
        print(f"iteration {i:3d}   loss {loss:.6e}   normal off by {err:.3e} rad")
    print(f"true angles   {TRUTH[0]:9.6f} {TRUTH[1]:9.6f}\nfitted angles {angles[0]:9.6f} {angles[1]:9.6f}")


if __name__ == "__main__":
    main()
