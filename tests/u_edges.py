"""Sample inputs at the points of the unit square where a sampler goes wrong, shared by tests/test_u_edges_cpu.py (which pins this
construction to the oracle), tests/test_gpu_u_edges.py and tests/test_rgl_cpu.py.  Needs no GPU.

generate_pairs draws 24-bit uniform numbers, so none of these points is met by the random batches: u0 on the branch line of the
one-sample mixture (alpha = 1/2 for MRL_OPT_SAMPLING 1, 1/8 for 2), the cosine square's corners, rim, centre and diagonals (where
sincos_quarter_f32 is evaluated at exactly +-pi/4 and the two disk maps break the |a| == |b| tie differently), u0 at 0 and at the
largest Float below 1, u0 on a value of the CDF being searched and on its two Float neighbours, u1 at 0, 1/2 and below 1."""
import numpy as np

F = np.float32
BELOW1 = np.nextafter(F(1), F(0))
EPS24 = F(2.0 ** -24)
U1_EDGES = np.array([0.0, EPS24, 0.25, np.nextafter(F(0.5), F(0)), 0.5, np.nextafter(F(0.5), F(1)), 0.75, BELOW1], F)
DIAGONAL = np.array([0.125, 0.3, 0.5, 0.625, 0.9], F)
N_INCIDENT_BINS = 32                     # incident bins of the conditional table P(theta_h | theta_i)
SPREAD_ABOVE = 64                        # tables with more theta_h bins deal their CDF entries out over the incident directions


def _below(x):
    return np.nextafter(np.asarray(x, F), F(-1))


def _above(x):
    return np.nextafter(np.asarray(x, F), F(2))


def edge_u0(alpha, cdf=None):
    """The u0 values of edge_u, sorted, in [0, 1): u0 = 1 is outside the sampler's contract."""
    a = F(alpha)
    vals = [a * F(x) for x in (0.0, EPS24, 0.25, 0.5, 0.75, BELOW1)]            # scale exactly to the cosine square's edges and centre
    vals += [_below(a), a, _above(a), F(0.75), BELOW1]
    vals = [np.asarray(vals, F)]
    if cdf is not None:
        c = (np.float64(a) + (1.0 - np.float64(a)) * np.asarray(cdf, np.float64)).astype(F)
        vals += [c, _below(c), _above(c)]
    u0 = np.unique(np.concatenate(vals))
    return u0[(u0 >= 0) & (u0 < 1)]


def edge_u(alpha, cdf=None):
    """Float pairs [k, 2]: every u0 of edge_u0 crossed with U1_EDGES, then the two diagonals of the scaled cosine square.
    Cosine sampling (mode 0) uses alpha = 1 and no CDF."""
    a = F(alpha)
    u0 = edge_u0(alpha, cdf)
    grid = np.stack([np.repeat(u0, U1_EDGES.size), np.tile(U1_EDGES, u0.size)], 1)
    diag = np.concatenate([np.stack([DIAGONAL * a, DIAGONAL], 1), np.stack([DIAGONAL * a, F(1) - DIAGONAL], 1)])
    return np.ascontiguousarray(np.concatenate([grid, diag]), F)


def _dir(theta, az):
    return np.array([np.sin(theta) * np.cos(az), np.sin(theta) * np.sin(az), np.cos(theta)])


def incident_directions(bin_centres=True):
    """theta_i from the normal (exactly (0, 0, 1)) to 1e-4 above the horizon at assorted azimuths, then (bin_centres) one direction at
    the centre of incident bins 0, 15 and 31 of the conditional table.  None sits on a bin boundary, where the row index would depend
    on the last bit of normalized()."""
    thetas = (0.0, 1e-4, 0.3, 0.8, 1.2, 1.5, np.pi / 2 - 1e-4)
    azimuths = (0.0, 0.7, -2.1, 2.9, 1.3, -0.4, 4.0)
    d = [_dir(t, p) for t, p in zip(thetas, azimuths)]
    d[0] = np.array([0.0, 0.0, 1.0])
    if bin_centres:
        for i, p in ((0, 0.5), (15, -1.7), (31, 2.3)):
            d.append(_dir(np.arccos((i + 0.5) / N_INCIDENT_BINS), p))
    return np.ascontiguousarray(d, F)


def incident_bin(wi, n_i=N_INCIDENT_BINS):
    """sampling_row's row of the conditional table: floor(cos(theta_i) n_i) of the f64-normalised direction, clamped"""
    w = np.asarray(wi, np.float64)
    z = w[..., 2] / np.linalg.norm(w, axis=-1)
    return np.clip((z * n_i).astype(np.int64), 0, n_i - 1)


def edge_units(wis, alpha, cdf_of=None):
    """(wi [n, 3], u [n, 2], first [len(wis) + 1]): every incident direction with the edge set of its own CDF (cdf_of(k): the n_th + 1
    values direction k searches; None: no CDF).  Units first[k] : first[k + 1] belong to direction k.  A CDF of more than SPREAD_ABOVE
    bins is dealt out: entry j goes to direction j mod len(wis), so that every entry is still drawn on, crossed with every u1, and a
    batch stays below 20,000 units."""
    wi_p, u_p, first = [], [], [0]
    for k, w in enumerate(wis):
        cdf = None if cdf_of is None else np.asarray(cdf_of(k), np.float64)
        if cdf is not None and cdf.size - 1 > SPREAD_ABOVE:
            cdf = cdf[k % len(wis)::len(wis)]
        u = edge_u(alpha, cdf)
        wi_p.append(np.tile(w, (u.shape[0], 1))); u_p.append(u); first.append(first[-1] + u.shape[0])
    return np.ascontiguousarray(np.concatenate(wi_p), F), np.ascontiguousarray(np.concatenate(u_p), F), np.array(first)


def lobe_direction(s, cdf, alpha, wi, u):
    """The f64 restatement of table_sample_dir's lobe branch (u0 >= alpha): theta_h by inverting the row CDF with
    (u0 - alpha) / (1 - alpha) (sin^2 theta_h is uniform inside a bin), phi_h = 2 pi u1, wo = reflect(wi, h).  s, cdf: [n_th + 1];
    wi [n, 3], u [n, 2].  Returns the unrounded direction [n, 3]; its z <= 0 means "rejected"."""
    s = np.asarray(s, np.float64); cdf = np.asarray(cdf, np.float64)
    n = s.size - 1
    a = F(alpha)
    u = np.asarray(u, F)
    t = (u[:, 0] - a).astype(np.float64) * (1.0 / (1.0 - np.float64(a)))          # u0 - alpha is exact in Float
    i = np.clip(np.searchsorted(cdf[:n], t, side="right") - 1, 0, n - 1)          # largest i in [0, n - 1] with cdf[i] <= t
    xi = (t - cdf[i]) / (cdf[i + 1] - cdf[i])
    sin2 = s[i] + xi * (s[i + 1] - s[i])
    ct, st = np.sqrt(np.maximum(1.0 - sin2, 0.0)), np.sqrt(sin2)
    phi = 2.0 * np.pi * u[:, 1].astype(np.float64)
    h = np.stack([st * np.cos(phi), st * np.sin(phi), ct], 1)
    w = np.asarray(wi, np.float64)
    w = w / np.linalg.norm(w, axis=1, keepdims=True)
    c = np.sum(w * h, axis=1, keepdims=True)
    return 2.0 * c * h - w


# ------------------------------------------------------------------ the RGL product: u on the file's own luminance integrals
def rgl_edge_pairs(marg, cond, device=False):
    """u at 0, at the largest Float below 1, at 1, and at the exact Float values of one luminance slice's marginal (marg [ny - 1]) and
    conditional (cond [ny, nx - 1]) integrals.  Conditional plateaus are reached in row 0 (u0 = 0: y = 0, the row total r0 and u1 r0
    exact in f64), by u1 = c / r0 rounded and its two Float neighbours.  device: the pairs with an entry equal to 1 removed (u = 1 is
    outside the kernels' contract)."""
    below1 = np.nextafter(np.float32(1), np.float32(0))
    u0s = np.unique(np.concatenate([[0.0, below1, 1.0], marg, np.nextafter(marg, np.float32(0)), np.nextafter(marg, np.float32(2))])).astype(np.float32)
    u1s = np.unique(np.concatenate([[0.0, below1, 1.0, 0.5]])).astype(np.float32)
    pairs = [(a, b) for a in u0s for b in u1s]
    r0 = float(cond[0, -1])                                        # (node row 0 of the "rows" file has no mass)
    if r0 > 0:
        c_over = (cond[0].astype(np.float64) / r0).astype(np.float32)
        for c in np.concatenate([c_over, np.nextafter(c_over, np.float32(0)), np.nextafter(c_over, np.float32(2))]):
            pairs.append((np.float32(0), np.float32(min(c, 1.0))))
    u = np.array(pairs, np.float32)
    if device:
        u = u[(u < 1).all(axis=1)]
    return u


def rgl_luminance_integrals(orc, slice_index=0):
    """(marg [ny - 1], cond [ny, nx - 1]) of one slice of an OracleRgl's luminance warp"""
    lum = orc.c.luminance
    nx, ny = lum.nx, lum.ny
    marg = np.ctypeslib.as_array(lum.marg, shape=(lum.n_slices, ny - 1))[slice_index].copy()
    cond = np.ctypeslib.as_array(lum.cond, shape=(lum.n_slices, ny, nx - 1))[slice_index].copy()
    return marg, cond


def rgl_edge_units(u, seed=31, k=24):
    """every u against k incident directions from the normal to grazing: (wi, wo, u), direction-major"""
    rng = np.random.default_rng(seed)
    t = np.concatenate([[0.0], rng.uniform(0.0, 1.5, k - 1)]); p = rng.uniform(-np.pi, np.pi, k)
    wis = np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], 1).astype(np.float32)
    wi = np.repeat(wis, u.shape[0], axis=0)
    u = np.tile(u, (k, 1))
    wo = np.ascontiguousarray(np.roll(wi, 7, axis=0) * np.array([1, -1, 1], np.float32))
    return wi, wo, u


# ------------------------------------------------------------------ the table samplers' batches
ALPHA = {0: 1.0, 1: 0.5, 2: 0.125}       # MRL_OPT_SAMPLING -> weight of the cosine lobe (mode 0: all of it)
TABLE_CASES = [("odd_7x5x3", (7, 5, 3), "noise", 5), ("odd_37x11x53", (37, 11, 53), "ggx_tab", 6), ("scan_257x4x6", (257, 4, 6), "noise", 8)]
TABLE_SCALE = (0.5, 2.0, 1.25)


def table_edge_units(mode, cdf=None, rows=None):
    """(wis, wi, u, first) of a sampling mode: 0 cosine (no CDF), 1 the marginal (cdf [n_th + 1]), 2 the conditional table
    (rows [32, 2 n_th + 1] as material_sampling2d / sampling2d_arrays give them: each direction searches the row of its own bin)"""
    wis = incident_directions(bin_centres=(mode == 2))
    if mode == 0:
        cdf_of = None
    elif mode == 1:
        cdf_of = lambda k: cdf
    else:
        n_th = (rows.shape[1] - 1) // 2
        b = incident_bin(wis, rows.shape[0])
        cdf_of = lambda k: rows[b[k], :n_th + 1]
    return (wis,) + edge_units(wis, ALPHA[mode], cdf_of)


def table_lobe_directions(mode, s, wis, wi, u, first, cdf=None, rows=None):
    """(lobe [n] bool, d [n, 3] f64): lobe_direction for the lobe units (u0 >= alpha) of a table_edge_units batch, each direction on
    the CDF it searches; zeros elsewhere"""
    n_th = np.asarray(s).size - 1
    lobe = u[:, 0] >= F(ALPHA[mode])
    d = np.zeros((wi.shape[0], 3))
    b = incident_bin(wis, rows.shape[0]) if mode == 2 else None
    for k in range(len(wis)):
        sel = np.arange(first[k], first[k + 1])
        sel = sel[lobe[sel]]
        d[sel] = lobe_direction(s, cdf if mode == 1 else rows[b[k], :n_th + 1], ALPHA[mode], wi[sel], u[sel])
    return lobe, d
