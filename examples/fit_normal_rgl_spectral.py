"""From measurements to a shading normal THROUGH A SPECTRAL RGL MATERIAL: the twin of examples/fit_normal_rgl.py on a spectral file
(what upstream Mitsuba 3's `measured` evaluates in its spectral variants) with per-unit hero wavelengths, as a hero-wavelength
renderer carries them per ray.  The surface is a synthetic spectral RGL file (synth.make_rgl_fields, isotropic, the database's shape,
32 wavelength nodes); every unit has its own four wavelengths, drawn once; the local directions R(p) wi, R(p) wo go through
diff.rgl_spectral_eval, whose backward pass (MerlHip.rgl_grad_dir_spectral, one call) hands d eval / d direction back to torch.  The
objective is piecewise smooth, so the line search of fit_normal.fit is what guarantees a loss that does not rise; no convergence
rate is promised.

    python examples/fit_normal_rgl_spectral.py [--log2n 16] [--iters 8] [--seed 0] [--wavelengths 4]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fit_normal import TRUTH, fit, rotation            # noqa: E402


def fit_rgl_spectral(gpu, material, wi, wo, wavelengths, iters=8):
    """wi, wo: local direction pairs [n, 3] on the device, as the TRUE frame sees them; wavelengths: [n, W] float32 on the device.
    Returns fit_normal.fit's (angles, loss history, angle-error history) for the spectral RGL material `material` of `gpu`."""
    from mitsuba_customization_amd import diff
    r = rotation(torch.tensor(TRUTH, dtype=torch.float64)).to(wi.device)
    wi_w, wo_w = wi.to(torch.float64) @ r, wo.to(torch.float64) @ r
    return fit(lambda a, b: diff.rgl_spectral_eval(gpu, a, b, wavelengths, material=material), wi_w, wo_w, iters=iters)


def main():
    from mitsuba_customization_amd import host, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=16)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--wavelengths", type=int, default=4)
    args = ap.parse_args()
    n = 1 << args.log2n
    with host.MerlHip(0) as gpu:
        mid = gpu.upload_rgl(synth.make_rgl_fields(seed=args.seed, n_phi=1, n_theta=8, res=32, res_ndf=128, res_sigma=32, n_wavelengths=32))
        nodes = gpu.wavelengths(mid)
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        draw = torch.rand((n, args.wavelengths), generator=torch.Generator().manual_seed(args.seed), dtype=torch.float32)
        wavelengths = (float(nodes[0]) + draw * float(nodes[-1] - nodes[0])).cuda()
        angles, history, errors = fit_rgl_spectral(gpu, mid, wi, wo, wavelengths, iters=args.iters)
    for i, (loss, err) in enumerate(zip(history, errors)):
        print(f"iteration {i:3d}   loss {loss:.6e}   normal off by {err:.3e} rad")
    print(f"true angles   {TRUTH[0]:9.6f} {TRUTH[1]:9.6f}\nfitted angles {angles[0]:9.6f} {angles[1]:9.6f}")
    print(f"final angular error {errors[-1]:.3e} rad after {len(history) - 1} iterations")


if __name__ == "__main__":
    main()
