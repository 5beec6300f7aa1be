"""numpy f64 restatement of A^T, the adjoint of eval on an RGB table (include/merl_hip.h, mrl_table_grad_batch).

Row u of A holds guard x (cos(theta_o) or 1) x scale[c] x the eight corner weights of the trilinear lookup (a single 1 for the
nearest lookup).  The coordinates come from tests/np_restatement.py (half_diff / coords) and its split rules; the weights are
formed in f64 the way corner_weights() does and rounded once to f32, the cosine is the Float wo.z.  Pinned to the CPU oracle by
tests/test_table_grad_cpu.py, never to the code under test."""
import numpy as np

from tests import np_restatement as npr

HALF_DIFF, STANDARD, STANDARD_FULL = 0, 1, 2


def guard(wi, wo):
    """The units eval does not mask: both cosines positive, every component finite."""
    wi = np.asarray(wi, np.float32); wo = np.asarray(wo, np.float32)
    with np.errstate(invalid="ignore"):
        return (wi[:, 2] > 0) & (wo[:, 2] > 0) & np.isfinite(wi).all(1) & np.isfinite(wo).all(1)


def table_coords(wi, wo, dims, param=HALF_DIFF):
    """Continuous table coordinates (x0, x1, x2) of the guarded units (the others get a harmless direction)."""
    ok = guard(wi, wo)
    up = np.array([0.0, 0.0, 1.0])
    a = np.where(ok[:, None], np.asarray(wi, np.float32).astype(np.float64), up)
    b = np.where(ok[:, None], np.asarray(wo, np.float32).astype(np.float64), up)
    if param == HALF_DIFF:
        return npr.coords(*npr.half_diff(a, b), dims) + (ok,)
    a, b = npr.unit(a), npr.unit(b)
    n0, n1, n2 = dims
    ti = np.arctan2(np.hypot(a[:, 0], a[:, 1]), a[:, 2])
    to = np.arctan2(np.hypot(b[:, 0], b[:, 1]), b[:, 2])
    cr = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    dt = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
    dp = np.where((cr == 0) & (dt == 0), 0.0, np.arctan2(cr, dt))
    x0, x1 = ti / (np.pi / 2) * n0, to / (np.pi / 2) * n1
    if param == STANDARD:
        x2 = np.abs(dp) / np.pi * n2
    else:
        x2 = np.where(dp < 0, dp + 2 * np.pi, dp) / (2 * np.pi) * n2
    return x0, x1, x2, ok


def near_cell_boundary(wi, wo, dims, param=HALF_DIFF, eps=1e-9):
    """Units whose coordinate on some axis is within eps of an integer: a nearest lookup may bin them either way."""
    x0, x1, x2, ok = table_coords(wi, wo, dims, param)
    near = np.zeros(len(ok), bool)
    for x in (x0, x1, x2):
        near |= np.abs(x - np.round(x)) <= eps
    return near & ok


def _split_clamped(x, n):
    i = np.clip(np.floor(x).astype(np.int64), 0, n - 1)
    return i, np.minimum(i + 1, n - 1), np.clip(x - i, 0.0, 1.0)


def _split_periodic(x, n):
    fl = np.floor(x)
    i = np.mod(fl.astype(np.int64), n)
    return i, np.mod(i + 1, n), x - fl


def adjoint(wi, wo, g, dims, param=HALF_DIFF, trilinear=True, center=False, cosine=True, scale=(1.0, 1.0, 1.0)):
    """Returns (R, S): R = A^T g as f64 [3, n0, n1, n2] and S = sum_u |a_u g_u| per cell and channel (the error scale)."""
    n0, n1, n2 = dims
    wo32 = np.asarray(wo, np.float32)
    g64 = np.asarray(g, np.float32).astype(np.float64)
    x0, x1, x2, ok = table_coords(wi, wo, dims, param)
    factor = wo32[:, 2].astype(np.float64) if cosine else np.ones(len(ok))
    with np.errstate(invalid="ignore"):
        s = np.asarray(scale, np.float64)[None, :] * factor[:, None] * g64                   # [n, 3]
    keep = np.nonzero(ok)[0]
    s = s[keep]
    if trilinear:
        sh = 0.5 if center else 0.0
        h0, h1, fh = _split_clamped(x0[keep] - sh, n0)
        d0, d1, fd = _split_clamped(x1[keep] - sh, n1)
        p0, p1, fp = _split_clamped(x2[keep] - sh, n2) if param == STANDARD else _split_periodic(x2[keep] - sh, n2)
        gh, gd, gp = 1.0 - fh, 1.0 - fd, 1.0 - fp
        corners = [(h0, d0, p0, (gh * gd) * gp), (h0, d0, p1, (gh * gd) * fp), (h0, d1, p0, (gh * fd) * gp), (h0, d1, p1, (gh * fd) * fp),
                   (h1, d0, p0, (fh * gd) * gp), (h1, d0, p1, (fh * gd) * fp), (h1, d1, p0, (fh * fd) * gp), (h1, d1, p1, (fh * fd) * fp)]
    else:
        ih = np.clip(np.trunc(x0[keep]).astype(np.int64), 0, n0 - 1)
        id_ = np.clip(np.trunc(x1[keep]).astype(np.int64), 0, n1 - 1)
        ip = np.clip(np.trunc(x2[keep]).astype(np.int64), 0, n2 - 1)
        corners = [(ih, id_, ip, np.ones(len(keep)))]
    plane = n0 * n1 * n2
    R = np.zeros(3 * plane); S = np.zeros(3 * plane)
    for hi, di, pi, w in corners:
        w = w.astype(np.float32).astype(np.float64)                  # rounded once to Float, like corner_weights()
        cell = (hi * n1 + di) * n2 + pi
        for c in range(3):
            v = w * s[:, c]
            np.add.at(R, c * plane + cell, v)
            np.add.at(S, c * plane + cell, np.abs(v))
    return R.reshape(3, n0, n1, n2), S.reshape(3, n0, n1, n2)

