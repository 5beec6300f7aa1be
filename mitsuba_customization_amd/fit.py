"""From measurements (wi, wo, rgb) to a table: the normalised splat and CGLS on |A T - y|^2, built on MerlHip.eval (A) and
MerlHip.table_grad (A^T).  numpy arrays in -> numpy out, device tensors in -> device tensors out.

The context's lookup / node / cosine options define A.  fit_table uploads iterates that have negative entries, so A is linear
only with host.OPT_NEGATIVE at keep (1), set before the context's first table is uploaded."""
from __future__ import annotations

import numpy as np

from . import host


def _f64(x):
    return x.double() if host._is_tensor(x) else x.astype(np.float64)


def _f32(x):
    return x.float().contiguous() if host._is_tensor(x) else np.ascontiguousarray(x, np.float32)


def _dot(a, b) -> float:
    return float((a * b).sum())


def _upload(ctx, table, param, scale) -> int:
    t = table.cpu().numpy() if host._is_tensor(table) else table
    return ctx.upload_table(t, scale) if param is None else ctx.upload_table_param(t, param, scale)


def splat(ctx, dims, wi, wo, rgb, param=None, scale=(1.0, 1.0, 1.0)):
    """sum_u a_u y_u / sum_u a_u^2 per cell and channel: the exact least-squares table of a nearest lookup.  The numerator is
    A^T y, the denominator A^T (A 1).  Returns (table f64 [3, *dims], mask of the cells some unit reached); the rest is 0."""
    mid = _upload(ctx, np.ones((3,) + tuple(dims)), param, scale)
    try:
        num = ctx.table_grad(wi, wo, _f32(rgb), material=mid)
        den = ctx.table_grad(wi, wo, ctx.eval(wi, wo, material=mid), material=mid)
    finally:
        ctx.release_material(mid)
    mask = den > 0
    return num / (den + ~mask) * mask, mask


def fit_table(ctx, dims, wi, wo, rgb, iters, param=None, scale=(1.0, 1.0, 1.0)):
    """CGLS on |A T - y|^2 started from the splat.  Returns (table f64 [3, *dims], [|A T_k - y| for k = 0 .. iters])."""
    if ctx.get_option(host.OPT_NEGATIVE) != 1:
        raise ValueError("fit_table needs OPT_NEGATIVE = 1 (keep): the iterates have negative entries and a clamped upload is not linear")
    y = _f64(rgb)
    x, _ = splat(ctx, dims, wi, wo, rgb, param, scale)
    shape_mid = _upload(ctx, np.ones((3,) + tuple(dims)), param, scale)      # what table_grad takes dims, parameterisation and scale from

    def A(table):
        mid = _upload(ctx, table, param, scale)
        try:
            return _f64(ctx.eval(wi, wo, material=mid))
        finally:
            ctx.release_material(mid)

    def At(r):
        return ctx.table_grad(wi, wo, _f32(r), material=shape_mid)

    try:
        r = y - A(x)
        s = At(r)
        p, gamma = s, _dot(s, s)
        residuals = [_dot(r, r) ** 0.5]
        for _ in range(iters):
            q = A(p)
            qq = _dot(q, q)
            if gamma == 0.0 or qq == 0.0:
                residuals.append(residuals[-1])
                continue
            alpha = gamma / qq
            x = x + alpha * p
            r = r - alpha * q
            s = At(r)
            gamma_new = _dot(s, s)
            p = s + (gamma_new / gamma) * p
            gamma = gamma_new
            residuals.append(_dot(r, r) ** 0.5)
    finally:
        ctx.release_material(shape_mid)
    return x, residuals
