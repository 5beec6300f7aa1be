"""From measurements (wi, wo, rgb) to a material.
A table: the normalised splat and CGLS on |A T - y|^2, built on MerlHip.eval (A) and MerlHip.table_grad (A^T).  numpy arrays in ->
numpy out, device tensors in -> device tensors out.  splat_mat / fit_tables do the same for several tables at once from one
interleaved measurement set with a table index per unit, on MerlHip.table_grad_mat: one launch serves all tables.  splat_nch /
fit_table_nch are the twins for an n-channel table (1..32 channels, spectral measurements), on MerlHip.eval_nch and
MerlHip.table_grad_nch: one launch serves all channels.
A GGX conductor (alpha, eta[3], k[3]): Levenberg-Marquardt on sum w (eval - y)^2, built on MerlHip.eval and MerlHip.ggx_grad
(fit_ggx; the loop itself, lm_ggx, takes eval and gradient as callables).  fit_ggx_mat / lm_ggx_mat fit several conductors at once
from one interleaved set with a material index per unit, on MerlHip.ggx_grad_mat: one eval and one gradient launch per iteration.
The measured values of an RGB RGL file (fit_rgl_values): CGLS over R >= 0 on MerlHip.eval and MerlHip.rgl_values_grad, the other
fields of the file fixed; every iterate is written into the resident material with MerlHip.update_rgl_values.  The spectra of a
spectral RGL file from samples at per-unit wavelengths (fit_rgl_spectral_values): the same loop on MerlHip.eval_spectral,
MerlHip.rgl_spectral_values_grad and MerlHip.update_rgl_spectral_values.

The context's lookup / node / cosine options define A.  fit_table makes iterates resident that have negative entries, so A is linear
only with host.OPT_NEGATIVE at keep (1), set before the context's first table is uploaded.
An iterate becomes resident in place (MerlHip.update_table / update_ggx): every loop keeps one working material per
table or conductor and writes each iterate into it — a device tensor from device memory, without visiting the host."""
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


def _resident(ctx, mid, table):
    """the working material `mid` holds `table` (texels only: the fitting loops evaluate, they never sample)"""
    t = table.contiguous() if host._is_tensor(table) else np.ascontiguousarray(table, np.float64)
    ctx.update_table(mid, t, keep_sampling=True)
    return mid


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


def _cgls(A, At, y, x, iters):
    """CGLS on |A x - y|^2 from the start x.  Returns (x, [|A x_k - y| for k = 0 .. iters])."""
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
    return x, residuals


def fit_table(ctx, dims, wi, wo, rgb, iters, param=None, scale=(1.0, 1.0, 1.0)):
    """CGLS on |A T - y|^2 started from the splat.  Returns (table f64 [3, *dims], [|A T_k - y| for k = 0 .. iters])."""
    if ctx.get_option(host.OPT_NEGATIVE) != 1:
        raise ValueError("fit_table needs OPT_NEGATIVE = 1 (keep): the iterates have negative entries and a clamped upload is not linear")
    y = _f64(rgb)
    x, _ = splat(ctx, dims, wi, wo, rgb, param, scale)
    shape_mid = _upload(ctx, np.ones((3,) + tuple(dims)), param, scale)      # what table_grad takes dims, parameterisation and scale from
    work_mid = _upload(ctx, np.ones((3,) + tuple(dims)), param, scale)       # what every iterate is written into

    def A(table):
        return _f64(ctx.eval(wi, wo, material=_resident(ctx, work_mid, table)))

    def At(r):
        return ctx.table_grad(wi, wo, _f32(r), material=shape_mid)

    try:
        return _cgls(A, At, y, x, iters)
    finally:
        ctx.release_material(work_mid)
        ctx.release_material(shape_mid)


def _cgls_nonneg(zeros, shape, A, At, y, start, iters, name):
    """the loop of fit_rgl_values / fit_rgl_spectral_values: CGLS inside the face of x >= 0 the iterate lies in.  Returns (x, residuals)"""
    if start is None:
        one = zeros() + 1.0
        a1 = A(one)
        x = one * max(_dot(a1, y) / max(_dot(a1, a1), 1e-300), 0.0)
    else:
        x = _f64(start).reshape(shape) + zeros()
        if float(x.min()) < 0.0:
            raise ValueError(f"{name}: the start must lie in R >= 0")
    r = y - A(x)
    residuals = [_dot(r, r) ** 0.5]
    p, gamma, free = None, 0.0, None
    for _ in range(iters):
        s = At(r)
        now_free = (x > 0) | (s > 0)
        s = s * now_free
        g_new = _dot(s, s)
        restart = p is None or gamma == 0.0 or not bool((now_free == free).all())
        p = s if restart else s + (g_new / gamma) * p
        gamma, free = g_new, now_free
        q = A(p)
        qq = _dot(q, q)
        if g_new == 0.0 or qq == 0.0:
            residuals.append(residuals[-1])
            continue
        alpha = _dot(r, q) / qq                                     # the minimiser along p (CGLS: gamma / qq while p is conjugate)
        shrinking = p < 0
        if bool(shrinking.any()):                                   # the longest step that stays in R >= 0
            room = float((x[shrinking] / -p[shrinking]).min())
            if room < alpha:
                alpha, p_next = room, None
            else:
                p_next = p
        else:
            p_next = p
        x = x + alpha * p
        x = x * (x > 0)                                             # (a value that reaches 0 is 0, not a rounding below it)
        r = r - alpha * q
        p = p_next
        residuals.append(_dot(r, r) ** 0.5)
    return x, residuals


# ---- the measured values of an RGB RGL material (MerlHip.eval is A, MerlHip.rgl_values_grad is A^T) ----
def fit_rgl_values(ctx, mid, wi, wo, rgb, iters, start=None):
    """min |eval(R) - y|^2 over R >= 0 in the measured values R of the resident RGB RGL material `mid`, its other fields (vndf, ndf,
    sigma, luminance, the grids) fixed.  Built on MerlHip.eval (A), MerlHip.rgl_values_grad (A^T) and MerlHip.update_rgl_values:
    every array the loop evaluates is written into `mid` in place, and `mid` holds the result when the call returns.
    start: values [n_phi, n_theta, 3, ny, nx] >= 0, or None for the constant file that fits best (one eval of the all-ones file).
    The loop is CGLS inside the face of R >= 0 the iterate lies in: a step is cut where it would leave R >= 0 (the residual falls along
    the whole step, so it never rises), and the search restarts from the projected gradient whenever the set of free values changes
    — a value at 0 is free when its gradient points inwards.  On R >= 0 nothing is clamped and eval is linear; a direction p with
    negative entries is evaluated as eval(max(p, 0)) - eval(max(-p, 0)), two resident arrays without a negative value.
    Returns (R f64 like the file's rgb, [|eval(R_k) - y| for k = 0 .. iters])."""
    shape = ctx.rgl_values_shape(mid)
    tensor = host._is_tensor(wi)
    y = _f64(rgb)

    def zeros():
        if tensor:
            import torch
            return torch.zeros(shape, dtype=torch.float64, device=wi.device)
        return np.zeros(shape, np.float64)

    def A(v):                                                       # linear for every sign of v
        pos, neg = v * (v > 0), -v * (v < 0)
        ctx.update_rgl_values(mid, _f32(pos))
        out = _f64(ctx.eval(wi, wo, material=mid))
        if float(neg.max()) > 0.0:
            ctx.update_rgl_values(mid, _f32(neg))
            out = out - _f64(ctx.eval(wi, wo, material=mid))
        return out

    def At(r):
        return ctx.rgl_values_grad(wi, wo, _f32(r), [mid], material=mid)[0]

    x, residuals = _cgls_nonneg(zeros, shape, A, At, y, start, iters, "fit_rgl_values")
    ctx.update_rgl_values(mid, _f32(x))
    return x, residuals


# ---- the spectra of a spectral RGL material (MerlHip.eval_spectral is A, MerlHip.rgl_spectral_values_grad is A^T) ----
def fit_rgl_spectral_values(ctx, mid, wi, wo, wavelengths, values, iters, start=None):
    """min |eval_spectral(R) - y|^2 over R >= 0 in the spectra R of the resident spectral RGL material `mid`, its other fields (vndf,
    ndf, sigma, luminance, the grids, the wavelength nodes) fixed: fit_rgl_values on MerlHip.eval_spectral (A),
    MerlHip.rgl_spectral_values_grad (A^T) and MerlHip.update_rgl_spectral_values.  wavelengths: [n, W] per-unit wavelengths (hero
    wavelengths), values: the measurements y [n, W].  Every array the loop evaluates is written into `mid` in place, and `mid` holds
    the result when the call returns.  start: spectra [n_phi, n_theta, n_wl, ny, nx] >= 0, or None for the constant file that fits
    best.  Returns (R f64 like the file's spectra, [|eval_spectral(R_k) - y| for k = 0 .. iters])."""
    shape = ctx.rgl_spectral_values_shape(mid)
    tensor = host._is_tensor(wi)
    y = _f64(values)

    def zeros():
        if tensor:
            import torch
            return torch.zeros(shape, dtype=torch.float64, device=wi.device)
        return np.zeros(shape, np.float64)

    def A(v):                                                       # linear for every sign of v
        pos, neg = v * (v > 0), -v * (v < 0)
        ctx.update_rgl_spectral_values(mid, _f32(pos))
        out = _f64(ctx.eval_spectral(wi, wo, wavelengths, mid))
        if float(neg.max()) > 0.0:
            ctx.update_rgl_spectral_values(mid, _f32(neg))
            out = out - _f64(ctx.eval_spectral(wi, wo, wavelengths, mid))
        return out

    def At(r):
        return ctx.rgl_spectral_values_grad(wi, wo, wavelengths, _f32(r), [mid], material=mid)[0]

    x, residuals = _cgls_nonneg(zeros, shape, A, At, y, start, iters, "fit_rgl_spectral_values")
    ctx.update_rgl_spectral_values(mid, _f32(x))
    return x, residuals


# ---- n-channel tables (1..32 channels: MerlHip.eval_nch is A, MerlHip.table_grad_nch is A^T; one launch serves all channels) ----
def _upload_nch(ctx, table, param, scale) -> int:
    t = table.cpu().numpy() if host._is_tensor(table) else table
    return ctx.upload_table_nch(t, scale) if param is None else ctx.upload_table_param(t, param, scale)


def splat_nch(ctx, dims, wi, wo, values, param=None, scale=None):
    """splat() for an n-channel table: values is [n, n_channels], the channel count is its second dim.  Returns (table f64
    [n_channels, *dims], mask of the cells some unit reached); the rest is 0."""
    n_ch = int(values.shape[1])
    mid = _upload_nch(ctx, np.ones((n_ch,) + tuple(dims)), param, scale)
    try:
        (num,) = ctx.table_grad_nch(wi, wo, _f32(values), n_ch, [mid], material=mid)
        (den,) = ctx.table_grad_nch(wi, wo, ctx.eval_nch(wi, wo, n_ch, material=mid), n_ch, [mid], material=mid)
    finally:
        ctx.release_material(mid)
    mask = den > 0
    return num / (den + ~mask) * mask, mask


def fit_table_nch(ctx, dims, wi, wo, values, iters, param=None, scale=None):
    """fit_table() for an n-channel table: CGLS on |A T - y|^2 started from splat_nch.  Returns (table f64 [n_channels, *dims],
    [|A T_k - y| for k = 0 .. iters])."""
    if ctx.get_option(host.OPT_NEGATIVE) != 1:
        raise ValueError("fit_table_nch needs OPT_NEGATIVE = 1 (keep): the iterates have negative entries and a clamped upload is not linear")
    n_ch = int(values.shape[1])
    y = _f64(values)
    x, _ = splat_nch(ctx, dims, wi, wo, values, param, scale)
    shape_mid = _upload_nch(ctx, np.ones((n_ch,) + tuple(dims)), param, scale)   # what table_grad_nch takes dims, parameterisation and scales from
    work_mid = _upload_nch(ctx, np.ones((n_ch,) + tuple(dims)), param, scale)    # what every iterate is written into

    def A(table):
        return _f64(ctx.eval_nch(wi, wo, n_ch, material=_resident(ctx, work_mid, table)))

    def At(r):
        return ctx.table_grad_nch(wi, wo, _f32(r), n_ch, [shape_mid], material=shape_mid)[0]

    try:
        return _cgls(A, At, y, x, iters)
    finally:
        ctx.release_material(work_mid)
        ctx.release_material(shape_mid)


# ---- several tables from one interleaved measurement set (MerlHip.table_grad_mat: one launch for all tables) ----
def _per_table(value, count, default):
    return [default] * count if value is None else list(value)


def _unit_ids(mat, ids):
    """The material id of every unit: ids[mat[i]], or -1 (no material) where mat[i] is not an index into ids.  int32, like mat."""
    k = len(ids)
    if host._is_tensor(mat):
        import torch
        table = torch.tensor(list(ids) + [-1], dtype=torch.int32, device=mat.device)
        return table[torch.where((mat >= 0) & (mat < k), mat, torch.full_like(mat, k)).long()].contiguous()
    table = np.array(list(ids) + [-1], np.int32)
    return np.ascontiguousarray(table[np.where((mat >= 0) & (mat < k), mat, k)])


def _upload_all(ctx, tables, params, scales):
    ids = []
    try:
        for t, p, s in zip(tables, params, scales):
            ids.append(_upload(ctx, t, p, s))
    except Exception:
        for mid in ids:
            ctx.release_material(mid)
        raise
    return ids


def splat_mat(ctx, dims_list, wi, wo, mat, rgb, params=None, scales=None):
    """splat() for K tables at once: unit i belongs to table mat[i] (int32, an index into dims_list; any other value: to none).
    Two launches of table_grad_mat serve all tables.  Returns (tables, masks), tuples of K arrays like splat()'s."""
    k = len(dims_list)
    params, scales = _per_table(params, k, None), _per_table(scales, k, (1.0, 1.0, 1.0))
    ids = _upload_all(ctx, [np.ones((3,) + tuple(d)) for d in dims_list], params, scales)
    try:
        unit = _unit_ids(mat, ids)
        num = ctx.table_grad_mat(wi, wo, _f32(rgb), ids, mat=unit)
        den = ctx.table_grad_mat(wi, wo, ctx.eval(wi, wo, mat=unit), ids, mat=unit)
    finally:
        for mid in ids:
            ctx.release_material(mid)
    masks = tuple(d > 0 for d in den)
    return tuple(n / (d + ~m) * m for n, d, m in zip(num, den, masks)), masks


def fit_tables(ctx, dims_list, wi, wo, mat, rgb, iters, params=None, scales=None):
    """fit_table() for K tables from one interleaved measurement set: K independent CGLS problems driven by shared launches — per
    iteration one eval with material ids and one table_grad_mat, whatever K.  The step lengths, the conjugation factors and the
    residuals are kept per table, from dot products over that table's units.  mat: as in splat_mat(); what a unit of no table
    measured is never read into a sum (it may be NaN).
    Returns (tables, residuals): K arrays f64 [3, *dims_k] and K lists [|A_k T_k - y_k| for iteration 0 .. iters]."""
    if ctx.get_option(host.OPT_NEGATIVE) != 1:
        raise ValueError("fit_tables needs OPT_NEGATIVE = 1 (keep): the iterates have negative entries and a clamped upload is not linear")
    k = len(dims_list)
    params, scales = _per_table(params, k, None), _per_table(scales, k, (1.0, 1.0, 1.0))
    y = _f64(rgb)
    x = list(splat_mat(ctx, dims_list, wi, wo, mat, rgb, params, scales)[0])
    member = [mat == j for j in range(k)]                            # [n] masks: the units of table j
    weight = [_f64(m)[:, None] for m in member]
    shape_ids = _upload_all(ctx, [np.ones((3,) + tuple(d)) for d in dims_list], params, scales)
    shape_unit = _unit_ids(mat, shape_ids)
    work_ids = []

    def A(tables):
        for mid, t in zip(work_ids, tables):
            _resident(ctx, mid, t)
        return _f64(ctx.eval(wi, wo, mat=work_unit))

    def At(r):
        return ctx.table_grad_mat(wi, wo, _f32(r), shape_ids, mat=shape_unit)

    def unit_dots(a):                                               # per table: the dot product of a with itself over its units
        rows = (a * a).sum(1)                                       # (selected, not weighted: a unit of no table may hold NaN)
        return [float(rows[m].sum()) for m in member]

    try:
        work_ids += _upload_all(ctx, [np.ones((3,) + tuple(d)) for d in dims_list], params, scales)   # what every iterate is written into
        work_unit = _unit_ids(mat, work_ids)
        r = y - A(x)
        s = At(r)
        p = list(s)
        gamma = [_dot(sj, sj) for sj in s]
        residuals = [[rr ** 0.5] for rr in unit_dots(r)]
        for _ in range(iters):
            qq = unit_dots(q := A(p))
            alpha = [g / d if g != 0.0 and d != 0.0 else 0.0 for g, d in zip(gamma, qq)]
            for j in range(k):
                x[j] = x[j] + alpha[j] * p[j]
            r = r - sum(a * w for a, w in zip(alpha, weight)) * q
            s = At(r)
            for j in range(k):
                if alpha[j] == 0.0:                                 # a table that has converged (or has no unit) stays as it is
                    continue
                gamma_new = _dot(s[j], s[j])
                p[j] = s[j] + (gamma_new / gamma[j]) * p[j]
                gamma[j] = gamma_new
            for j, rr in enumerate(unit_dots(r)):
                residuals[j].append(rr ** 0.5 if alpha[j] != 0.0 else residuals[j][-1])
    finally:
        for mid in work_ids + shape_ids:
            ctx.release_material(mid)
    return tuple(x), residuals


# ---- GGX conductor: Levenberg-Marquardt in q = (ln alpha, ln eta[3], k[3]) ----
def _ggx_params(q):
    """p = (alpha, eta[3], k[3]) of q, and dp/dq (diagonal)."""
    p = np.concatenate([np.exp(q[:4]), q[4:]])
    return p, np.concatenate([p[:4], np.ones(3)])


def lm_ggx(eval_fn, grad_fn, rgb, start, iters, weights=None):
    """Levenberg-Marquardt on L(p) = sum w (eval(p) - rgb)^2 over p = (alpha, eta[3], k[3]).
    eval_fn(p) -> eval [n, 3] at the 7-vector p;  grad_fn(p, g, h) -> (sum g J [7], sum h J J^T [7, 7]) as numpy f64, h None = 1;
    grad_fn is only called right after eval_fn at the same p.  alpha and eta move in log space (the chain rule is applied to the
    7-vector and the 7 x 7 matrix here), k in linear space, projected onto k >= 0 (a k that starts at 0 stays there; a positive one
    never lands on 0, where its gradient vanishes).  One eval_fn call per iteration: a step that raises L is dropped and the
    damping raised.  Returns (alpha, eta [3], k [3], [sqrt(L) at the start and after each iteration])."""
    alpha, eta, k = start
    y = _f64(rgb)
    w = None if weights is None else _f64(weights)
    if w is not None and w.ndim == 1:
        w = w[:, None]

    def loss_and_model(q):
        p, s = _ggx_params(q)
        r = _f64(eval_fn(p)) - y
        wr = r if w is None else w * r
        return float((wr * r).sum()), p, s, wr

    def model(p, s, wr):
        # g = dL / d eval = 2 w r, h = d2L / d eval2 = 2 w: the factor 2 is applied to the sums
        h = None if w is None else _f32(w.expand(wr.shape) if host._is_tensor(w) else np.broadcast_to(w, wr.shape))
        g, N = grad_fn(p, _f32(wr), h)
        return 2.0 * s * np.asarray(g, np.float64), 2.0 * np.outer(s, s) * np.asarray(N, np.float64)

    q = np.concatenate([np.log(np.asarray([alpha, *eta], np.float64)), np.asarray(k, np.float64)])
    loss, p, s, wr = loss_and_model(q)
    grad, N = model(p, s, wr)
    lam, history = 1e-3, [loss ** 0.5]
    for _ in range(iters):
        d = np.diag(N).copy()
        d[d <= 0.0] = 1.0                                   # a parameter nothing depends on (k of a channel at k = 0) stays put
        try:
            step = np.linalg.solve(N + lam * np.diag(d), -grad)
        except np.linalg.LinAlgError:
            step = -grad / ((1.0 + lam) * d)
        trial = q + step
        # k >= 0.  F depends on k through k^2, so at k = 0 exactly the gradient with respect to k is zero and an iterate that
        # lands there never leaves: a step that would cross zero from k > 0 stops at a tenth of the current value instead
        trial[4:] = np.maximum(trial[4:], 0.1 * q[4:])
        t_loss, t_p, t_s, t_wr = loss_and_model(trial)
        if np.isfinite(t_loss) and t_loss <= loss:
            q, loss = trial, t_loss
            grad, N = model(t_p, t_s, t_wr)
            lam = max(lam / 10.0, 1e-12)
        else:
            lam = min(lam * 10.0, 1e12)
        history.append(loss ** 0.5)
    p, _ = _ggx_params(q)
    return float(p[0]), p[1:4].copy(), p[4:7].copy(), history


def lm_ggx_mat(eval_fn, grad_fn, rgb, unit_ids, starts, iters, weights=None):
    """lm_ggx() for K conductors at once from one interleaved measurement set: unit i belongs to material unit_ids[i] (an index into
    starts; any other value: to none — what such a unit measured is never read into a sum and may be NaN).
    eval_fn(P) -> eval [n, 3] with every unit evaluated at its own material's row of P [K, 7];  grad_fn(P, g, h) -> (sum g J [K, 7],
    sum h J J^T [K, 7, 7]) as numpy f64, each material's sums over its own units, h None = 1; grad_fn is only called right after
    eval_fn at the same P.  One eval_fn and at most one grad_fn call per iteration, whatever K: the normal matrix is block-diagonal,
    so every material has its own damping and accepts or drops its own step on its own share of the loss, with lm_ggx's
    parameterisation and k >= 0 rule.  Returns K tuples (alpha, eta [3], k [3], [sqrt(L_j) at the start and after each iteration])."""
    count = len(starts)
    y = _f64(rgb)
    w = None if weights is None else _f64(weights)
    if w is not None and w.ndim == 1:
        w = w[:, None]
    member = [unit_ids == j for j in range(count)]

    def losses_and_model(Q):
        ps = [_ggx_params(q) for q in Q]
        P, S = np.stack([p for p, _ in ps]), np.stack([s for _, s in ps])
        r = _f64(eval_fn(P)) - y
        wr = r if w is None else w * r
        rows = (wr * r).sum(1)
        return np.array([float(rows[m].sum()) for m in member]), P, S, wr

    def model(P, S, wr):
        h = None if w is None else _f32(w.expand(wr.shape) if host._is_tensor(w) else np.broadcast_to(w, wr.shape))
        g, N = grad_fn(P, _f32(wr), h)
        g, N = np.asarray(g, np.float64), np.asarray(N, np.float64)
        return 2.0 * S * g, 2.0 * S[:, :, None] * S[:, None, :] * N

    Q = np.stack([np.concatenate([np.log(np.asarray([alpha, *eta], np.float64)), np.asarray(k, np.float64)]) for alpha, eta, k in starts])
    loss, P, S, wr = losses_and_model(Q)
    grad, N = model(P, S, wr)
    lam = np.full(count, 1e-3)
    history = [[float(v) ** 0.5] for v in loss]
    for _ in range(iters):
        trial = Q.copy()
        for j in range(count):
            d = np.diag(N[j]).copy()
            d[d <= 0.0] = 1.0
            try:
                step = np.linalg.solve(N[j] + lam[j] * np.diag(d), -grad[j])
            except np.linalg.LinAlgError:
                step = -grad[j] / ((1.0 + lam[j]) * d)
            trial[j] = Q[j] + step
            trial[j, 4:] = np.maximum(trial[j, 4:], 0.1 * Q[j, 4:])
        t_loss, t_P, t_S, t_wr = losses_and_model(trial)
        accept = np.isfinite(t_loss) & (t_loss <= loss)
        if accept.any():
            # the sums at the trial point: a material that dropped its step keeps the ones of the point it stays at, and what its
            # units hold at the trial point (NaN after an overflow) is not handed on
            for j in range(count):
                if not accept[j]:
                    t_wr[member[j]] = 0.0
            t_grad, t_N = model(t_P, t_S, t_wr)
            Q[accept], loss[accept], grad[accept], N[accept] = trial[accept], t_loss[accept], t_grad[accept], t_N[accept]
        lam = np.where(accept, np.maximum(lam / 10.0, 1e-12), np.minimum(lam * 10.0, 1e12))
        for j in range(count):
            history[j].append(float(loss[j]) ** 0.5)
    out = []
    for j in range(count):
        p, _ = _ggx_params(Q[j])
        out.append((float(p[0]), p[1:4].copy(), p[4:7].copy(), history[j]))
    return out


def fit_ggx_mat(ctx, wi, wo, mat, rgb, starts, iters, weights=None):
    """fit_ggx() for K conductors from one interleaved measurement set: mat[i] (int32) is the index into starts of the material unit
    i measured; any other value: none.  K working materials are created once; every iteration writes its parameters into them
    (update_ggx) and runs one eval with material ids and one ggx_grad_mat(..., normal=True) on them.  Returns K tuples (alpha, eta [3], k [3], residual history) — see
    lm_ggx_mat."""
    held = []
    unit = [None]

    def drop():
        while held:
            ctx.release_material(held.pop())

    def eval_fn(P):
        if not held:
            for p in P:
                held.append(ctx.ggx(float(p[0]), [float(x) for x in p[1:4]], [float(x) for x in p[4:7]]))
            unit[0] = _unit_ids(mat, held)
        else:
            for mid, p in zip(held, P):
                ctx.update_ggx(mid, float(p[0]), [float(x) for x in p[1:4]], [float(x) for x in p[4:7]])
        return ctx.eval(wi, wo, mat=unit[0])

    def grad_fn(P, g, h):
        grad, N = ctx.ggx_grad_mat(wi, wo, g, held, mat=unit[0], curvature=h, normal=True)
        if host._is_tensor(grad):
            grad, N = grad.cpu().numpy(), N.cpu().numpy()
        return grad, N

    try:
        return lm_ggx_mat(eval_fn, grad_fn, rgb, mat, starts, iters, weights)
    finally:
        drop()


def fit_ggx(ctx, wi, wo, rgb, start, iters, weights=None):
    """The GGX conductor closest to the measurements: Levenberg-Marquardt on sum w (eval - rgb)^2 from start = (alpha, eta[3], k[3]).
    One working material is created once; every iteration writes its parameters into it (update_ggx) and runs eval and
    ggx_grad(..., normal=True) on it.  weights: [n] or [n, 3], None = 1.
    Returns (alpha, eta [3], k [3], residual history) — see lm_ggx."""
    held = []

    def drop():
        while held:
            ctx.release_material(held.pop())

    def eval_fn(p):
        args = (float(p[0]), [float(x) for x in p[1:4]], [float(x) for x in p[4:7]])
        if held:
            ctx.update_ggx(held[0], *args)
        else:
            held.append(ctx.ggx(*args))
        return ctx.eval(wi, wo, material=held[0])

    def grad_fn(p, g, h):
        grad, N = ctx.ggx_grad(wi, wo, g, held[0], curvature=h, normal=True)
        if host._is_tensor(grad):
            grad, N = grad.cpu().numpy(), N.cpu().numpy()
        return grad, N

    try:
        return lm_ggx(eval_fn, grad_fn, rgb, start, iters, weights)
    finally:
        drop()
