"""From sampled directions to a shading normal and a roughness: a GGX surface scatters world-space directions wi with known random
numbers u, the sampled directions wo are observed, and both the tilt of the shading frame and alpha are recovered.  The gradient has to
flow THROUGH THE SAMPLER: the local wi = R(p) wi_w goes into diff.ggx_sample, whose backward pass (MerlHip.ggx_sample_grad, one call)
hands d wo' / d wi and d wo' / d alpha back to torch, which carries them on to the two angles and to log alpha.  The fit is BFGS on
(p0, p1, log alpha) with a backtracking line search, so the loss never rises.

    python examples/fit_sampled_lobe.py [--log2n 14] [--iters 40] [--alpha 0.3]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fit_normal import angle_between_normals, rotation  # noqa: E402  (examples/ is on the path when this runs as a script or a test imports it)

ETA, K = (0.143, 0.375, 1.442), (3.983, 2.386, 1.603)           # gold-like
TRUTH = (0.06, -0.08, 0.3)                                      # two angles and alpha
START = (0.0, 0.0, 0.2)


def _params(alpha, dtype=torch.float64):
    return torch.cat([alpha.reshape(1).to(dtype), torch.tensor(ETA + K, dtype=dtype)])


def sampled_world(sample_fn, wi_w, u, x, dtype):
    """the sampled directions in world space for x = (p0, p1, log alpha): R(p)^T sample_fn(R(p) wi_w, u, params).  Rejected samples
    (a zero direction) stay zero."""
    r = rotation(x[:2]).to(wi_w.device)
    wo_l = sample_fn((wi_w @ r.T).to(dtype), u, _params(torch.exp(x[2])))
    return wo_l.to(torch.float64) @ r


def fit(sample_fn, wi_w, u, wo_obs=None, start=START, iters=40, dtype=torch.float32, truth=TRUTH):
    """BFGS on x = (p0, p1, log alpha) for sum |R(p)^T wo'(R(p) wi_w, u; alpha) - wo_obs|^2 over the units accepted on both sides.
    sample_fn(wi_local, u, params): the sampled local direction [n, 3] of `dtype`, differentiable in wi_local and in the f64 [7]
    parameter tensor (diff.ggx_sample bound to a context and a material, its first result); wi_w: float64 world directions on
    sample_fn's device; wo_obs: the observations (None: sample_fn at `truth`).
    Returns (x, loss history, normal-angle error history, |alpha - truth| history)."""
    as_x = lambda t: torch.tensor([t[0], t[1], math.log(t[2])], dtype=torch.float64)
    with torch.no_grad():
        if wo_obs is None:
            wo_obs = sampled_world(sample_fn, wi_w, u, as_x(truth), dtype)
    seen = (wo_obs * wo_obs).sum(-1) > 0

    def loss_of(x):
        wo = sampled_world(sample_fn, wi_w, u, x, dtype)
        both = seen & ((wo.detach() * wo.detach()).sum(-1) > 0)
        return (((wo - wo_obs) ** 2).sum(-1) * both).sum()

    def loss_and_gradient(x):
        q = x.clone().requires_grad_(True)
        loss = loss_of(q)
        loss.backward()
        return float(loss.detach()), q.grad.detach().clone()

    x = as_x(start)
    loss, g = loss_and_gradient(x)
    H = torch.eye(3, dtype=torch.float64) / max(float(g.norm()), 1e-30) * 0.05        # first step: 0.05 in parameter space
    history, errors, alphas = [loss], [angle_between_normals(x[:2], truth[:2])], [abs(math.exp(float(x[2])) - truth[2])]
    for _ in range(iters):
        step = -(H @ g)
        accepted = False
        with torch.no_grad():
            for _ in range(16):
                trial = float(loss_of(x + step))
                if trial <= loss:
                    accepted = True
                    break
                step = 0.5 * step
        if accepted and float(step.norm()) > 0:
            x_new = x + step
            loss, g_new = loss_and_gradient(x_new)
            s, yv = x_new - x, g_new - g
            sy = float(s @ yv)
            if sy > 1e-300:                                     # the BFGS update of the inverse Hessian
                rho = 1.0 / sy
                eye = torch.eye(3, dtype=torch.float64)
                H = (eye - rho * torch.outer(s, yv)) @ H @ (eye - rho * torch.outer(yv, s)) + rho * torch.outer(s, s)
            x, g = x_new, g_new
        history.append(loss); errors.append(angle_between_normals(x[:2], truth[:2])); alphas.append(abs(math.exp(float(x[2])) - truth[2]))
    return x, history, errors, alphas


def main():
    from mitsuba_customization_amd import diff, host
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=14)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--alpha", type=float, default=TRUTH[2])
    args = ap.parse_args()
    truth = (TRUTH[0], TRUTH[1], args.alpha)
    with host.MerlHip(0) as gpu:
        mid = gpu.ggx(START[2], ETA, K)
        wi, _, u = gpu.generate_pairs(0x5EED, 0, 1 << args.log2n)
        r = rotation(torch.tensor(truth[:2], dtype=torch.float64)).to(wi.device)
        wi_w = wi.to(torch.float64) @ r
        sample_fn = lambda a, uu, p: diff.ggx_sample(gpu, a, uu, material=mid, params=p)[0]
        x, history, errors, alphas = fit(sample_fn, wi_w, u, iters=args.iters, truth=truth)
    for i, (loss, err, da) in enumerate(zip(history, errors, alphas)):
        print(f"iteration {i:3d}   loss {loss:.6e}   normal off by {err:.3e} rad   alpha off by {da:.3e}")
    print(f"truth  {truth[0]:9.6f} {truth[1]:9.6f} alpha {truth[2]:.6f}\nfitted {float(x[0]):9.6f} {float(x[1]):9.6f} alpha {math.exp(float(x[2])):.6f}")


if __name__ == "__main__":
    main()
