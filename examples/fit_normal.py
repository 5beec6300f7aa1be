"""From measurements to a shading normal: a GGX surface is seen under world-space direction pairs, its shading frame is tilted by an
unknown rotation, and the tilt is recovered by Gauss-Newton.  The rotation R(p) = Rx(p0) Ry(p1) is written in torch; the local
directions R wi, R wo go through diff.ggx_eval, whose backward pass (MerlHip.ggx_grad_dir, one call) hands d eval / d direction back
to torch, which carries it on to the two angles.  Three backward passes with one-hot channel weights give the Jacobian of every
residual — units are independent, so the gradient of sum_u eval_uc in wi_u IS d eval_uc / d wi_u — and loss.backward() the
gradient of the loss in the angles.

    python examples/fit_normal.py [--log2n 16] [--iters 8] [--alpha 0.3]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ETA, K = (0.143, 0.375, 1.442), (3.983, 2.386, 1.603)           # gold-like
TRUTH = (0.16, -math.acos(math.cos(0.2) / math.cos(0.16)))      # the true normal is 0.2 rad from the start p = (0, 0)


def rotation(p):
    """world -> local, [3, 3], differentiable in the two angles p"""
    ca, sa, cb, sb = torch.cos(p[0]), torch.sin(p[0]), torch.cos(p[1]), torch.sin(p[1])
    one, zero = torch.ones_like(ca), torch.zeros_like(ca)
    rx = torch.stack([torch.stack([one, zero, zero]), torch.stack([zero, ca, -sa]), torch.stack([zero, sa, ca])])
    ry = torch.stack([torch.stack([cb, zero, sb]), torch.stack([zero, one, zero]), torch.stack([-sb, zero, cb])])
    return rx @ ry


def angle_between_normals(p, q):
    """between the shading normals R(p)^T e_z and R(q)^T e_z, rad"""
    a, b = rotation(torch.as_tensor(p, dtype=torch.float64))[2], rotation(torch.as_tensor(q, dtype=torch.float64))[2]
    return float(torch.atan2(torch.linalg.cross(a, b).norm(), a @ b))


def world_pairs(wi_local, wo_local, truth):
    """local direction pairs [n, 3] (numpy) as the world sees them when the frame is R(truth)"""
    r = rotation(torch.as_tensor(truth, dtype=torch.float64)).numpy()
    return np.asarray(wi_local, np.float64) @ r, np.asarray(wo_local, np.float64) @ r


def fit(eval_fn, wi_w, wo_w, y=None, start=(0.0, 0.0), iters=8, dtype=torch.float32, truth=TRUTH):
    """Gauss-Newton on p for sum |eval_fn(R(p) wi_w, R(p) wo_w) - y|^2; a step is halved until the loss does not rise.  eval_fn: a
    differentiable eval of [n, 3] local directions of `dtype` (diff.ggx_eval bound to a context and a material); wi_w, wo_w: float64
    tensors on eval_fn's device; y: the measurements (None: eval_fn at `truth`).  Returns (angles, loss history, angle-error history)."""
    def local(p):
        r = rotation(p).to(wi_w.device)
        return (wi_w @ r.T).to(dtype), (wo_w @ r.T).to(dtype)

    def residual(p):
        return (eval_fn(*local(p)) - y).to(torch.float64)

    with torch.no_grad():
        if y is None:
            y = eval_fn(*local(torch.tensor(truth, dtype=torch.float64)))
    p = torch.tensor(start, dtype=torch.float64)
    with torch.no_grad():
        loss = float((residual(p) ** 2).sum())
    history, errors = [loss], [angle_between_normals(p, truth)]
    for _ in range(iters):
        q = p.clone().requires_grad_(True)
        wi_l, wo_l = local(q)
        rgb = eval_fn(wi_l, wo_l)
        r = (rgb - y).to(torch.float64)
        # d local direction / d p_j = world direction @ (dR / dp_j)^T
        dr = torch.autograd.functional.jacobian(rotation, q.detach()).to(wi_w.device)        # [3, 3, 2]
        dwi, dwo = torch.einsum("uk,ikj->uij", wi_w, dr), torch.einsum("uk,ikj->uij", wo_w, dr)
        jac = []
        for c in range(r.shape[1]):                             # one-hot channel weights: the wrapper's backward, once per channel
            ji, jo = torch.autograd.grad(rgb[:, c].sum(), (wi_l, wo_l), retain_graph=True)
            jac.append(torch.einsum("ui,uij->uj", ji.to(torch.float64), dwi) + torch.einsum("ui,uij->uj", jo.to(torch.float64), dwo))
        jac = torch.stack(jac, 1)                               # [n, channels, 2]
        (r ** 2).sum().backward()                               # ... and once more, all the way to the angles: q.grad = 2 J^T r
        jtr = 0.5 * q.grad
        jtj = torch.einsum("uci,ucj->ij", jac, jac).cpu()
        step = -torch.linalg.solve(jtj + 1e-12 * torch.trace(jtj) * torch.eye(2, dtype=torch.float64), jtr)
        with torch.no_grad():
            for _ in range(12):
                trial = float((residual(p + step) ** 2).sum())
                if trial <= loss:
                    p, loss = p + step, trial
                    break
                step = 0.5 * step
        history.append(loss); errors.append(angle_between_normals(p, truth))
    return (float(p[0]), float(p[1])), history, errors


def main():
    from mitsuba_customization_amd import diff, host
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=16)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=0.3)
    args = ap.parse_args()
    with host.MerlHip(0) as gpu:
        mid = gpu.ggx(args.alpha, ETA, K)
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, 1 << args.log2n)
        r = rotation(torch.tensor(TRUTH, dtype=torch.float64)).to(wi.device)
        wi_w, wo_w = wi.to(torch.float64) @ r, wo.to(torch.float64) @ r
        angles, history, errors = fit(lambda a, b: diff.ggx_eval(gpu, a, b, material=mid), wi_w, wo_w, iters=args.iters)
    for i, (loss, err) in enumerate(zip(history, errors)):
        print(f"iteration {i:3d}   loss {loss:.6e}   normal off by {err:.3e} rad")
    print(f"true angles   {TRUTH[0]:9.6f} {TRUTH[1]:9.6f}\nfitted angles {angles[0]:9.6f} {angles[1]:9.6f}")


if __name__ == "__main__":
    main()
