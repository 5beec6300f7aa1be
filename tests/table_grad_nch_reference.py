"""numpy f64 restatement of A^T, the adjoint of eval on an n-channel table (include/merl_hip_fit_nch.h, mrl_table_grad_batch_nch).

Row u of A holds, per channel c, guard x (cos(theta_o) or 1) x scale[c] x the eight corner weights of the trilinear lookup (a single
1 for the nearest lookup).  Coordinates and split rules are those of tests/table_grad_reference.py (ref.table_coords and the split
rules of ref.adjoint); unlike there the weights stay in f64 — the n-channel blend does not round them to Float — and the cosine is
the Float wo.z.  Pinned to the CPU oracle by tests/test_table_grad_nch_cpu.py, never to the code under test."""
import numpy as np

from tests import table_grad_reference as ref


def scales(n_ch, k=0):
    """Non-unit channel scales of target k: between 0.4 and 2.5, no two channels alike."""
    return 0.4 + 2.1 * ((np.arange(n_ch) * 0.61803398875 + 0.37 * k + 0.11) % 1.0)


def gradients(wi, wo, n_ch, seed, stray=None):
    """g [n, n_ch] f32: random, NaN / inf (alternating) in the rows of the units the guard removes and of the units `stray` marks."""
    g = ref.poisoned(np.random.default_rng(seed).standard_normal((len(wi), n_ch)), wi, wo)
    if stray is not None:
        at = np.nonzero(stray)[0]
        g[at[0::2]] = np.nan; g[at[1::2]] = np.inf
    return g


def reference(wi, wo, g, role, specs, lookup, node, cosine=True):
    """[(R_k, S_k)]: adjoint_nch per target of specs ((dims, param), ..) on the units whose role is k, with scales(n_ch, k)."""
    out = []
    for k, (dims, param) in enumerate(specs):
        at = np.asarray(role) == k
        out.append(adjoint_nch(wi[at], wo[at], g[at], dims, param=param, trilinear=bool(lookup), center=bool(node), cosine=cosine,
                               scale=scales(g.shape[1], k)))
    return out


def adjoint_nch(wi, wo, g, dims, param=ref.HALF_DIFF, trilinear=True, center=False, cosine=True, scale=None):
    """Returns (R, S): R = A^T g as f64 [n_ch, n0, n1, n2] and S = sum_u |a_u g_u| per texel and channel (the error scale).
    g: [n, n_ch]; scale: n_ch values, None = ones."""
    n0, n1, n2 = dims
    g64 = np.asarray(g, np.float32).astype(np.float64)
    n_ch = g64.shape[1]
    scale = np.ones(n_ch) if scale is None else np.asarray(scale, np.float64)
    assert scale.shape == (n_ch,)
    wo32 = np.asarray(wo, np.float32)
    x0, x1, x2, ok = ref.table_coords(wi, wo, dims, param)
    factor = wo32[:, 2].astype(np.float64) if cosine else np.ones(len(ok))
    with np.errstate(invalid="ignore"):
        s = scale[None, :] * factor[:, None] * g64                                         # [n, n_ch]
    keep = np.nonzero(ok)[0]
    s = s[keep]
    if trilinear:
        sh = 0.5 if center else 0.0
        h0, h1, fh = ref._split_clamped(x0[keep] - sh, n0)
        d0, d1, fd = ref._split_clamped(x1[keep] - sh, n1)
        p0, p1, fp = ref._split_clamped(x2[keep] - sh, n2) if param == ref.STANDARD else ref._split_periodic(x2[keep] - sh, n2)
        gh, gd, gp = 1.0 - fh, 1.0 - fd, 1.0 - fp
        corners = [(h0, d0, p0, (gh * gd) * gp), (h0, d0, p1, (gh * gd) * fp), (h0, d1, p0, (gh * fd) * gp), (h0, d1, p1, (gh * fd) * fp),
                   (h1, d0, p0, (fh * gd) * gp), (h1, d0, p1, (fh * gd) * fp), (h1, d1, p0, (fh * fd) * gp), (h1, d1, p1, (fh * fd) * fp)]
    else:
        ih = np.clip(np.trunc(x0[keep]).astype(np.int64), 0, n0 - 1)
        id_ = np.clip(np.trunc(x1[keep]).astype(np.int64), 0, n1 - 1)
        ip = np.clip(np.trunc(x2[keep]).astype(np.int64), 0, n2 - 1)
        corners = [(ih, id_, ip, np.ones(len(keep)))]
    plane = n0 * n1 * n2
    R = np.zeros((n_ch, plane)); S = np.zeros((n_ch, plane))
    for hi, di, pi, w in corners:                                    # the f64 products as they are: no rounding to Float
        cell = (hi * n1 + di) * n2 + pi
        v = w[:, None] * s                                           # [units, n_ch]
        for c in range(n_ch):
            R[c] += np.bincount(cell, weights=v[:, c], minlength=plane)
            S[c] += np.bincount(cell, weights=np.abs(v[:, c]), minlength=plane)
    return R.reshape(n_ch, n0, n1, n2), S.reshape(n_ch, n0, n1, n2)
