"""The GGX rough conductor restated in f64 numpy from the published formulas, and the cases the GGX tests run on.

The restatement is independent of oracle/merl_oracle.c and csrc/merl_device.hpp (which mirror each other formula for formula)
and written in a different algebraic form:
  * Fresnel from complex arithmetic: n = eta + ik, cos(theta_t) = sqrt(1 - sin^2(theta) / n^2),
    r_s = (c - n cos_t) / (c + n cos_t), r_p = (n c - cos_t) / (n c + cos_t), F = (|r_s|^2 + |r_p|^2) / 2;
  * D from the angle of the microfacet normal: 1 / (pi a^2 cos^4(theta_m) (1 + tan^2(theta_m) / a^2)^2)   (Walter et al. 2007, eq. 33);
  * Smith G1 from tan(theta_v): 2 / (1 + sqrt(1 + a^2 tan^2(theta_v))), zero where v.m and v.n differ in sign   (ibid., eq. 34);
  * eval = F D G1(i) G1(o) / (4 cos(theta_i))  (the cosine of wo folded in) and, for visible-normal sampling,
    pdf = D G1(i) / (4 cos(theta_i))   (Heitz & d'Eon 2014).
Angles are taken with arctan2 / hypot, never acos of a component.

The cases (ALPHAS x METALS, case_units) are shared by tests/test_ggx_cpu.py, which asserts on the oracle and this file alone
every condition the GPU comparison relies on, and tests/test_gpu_ggx.py.
"""
import numpy as np

ALPHAS = (1e-3, 1e-2, 0.05, 0.3, 1.0, 2.0)
METALS = {                                   # name: (eta, k) per channel
    "gold": ((0.143, 0.375, 1.442), (3.983, 2.386, 1.603)),
    "aluminium": ((1.5, 1.45, 1.55), (7.6, 7.5, 7.7)),
    "dielectric": ((1.5, 1.5, 1.5), (0.0, 0.0, 0.0)),
    "spread_k": ((0.8, 1.1, 1.3), (0.3, 3.0, 30.0)),       # k differs by an order of magnitude from channel to channel
}
CASES = [(a, m) for a in ALPHAS for m in METALS]
N_RANDOM = 1 << 15
SEED = 0x66C7                                # with these windows no random unit lies within 1e-9 of the branch line (test_ggx_cpu.py)
BRANCH_SZ = 0.99999                          # the sampler's normal-incidence branch: stretched s_z >= BRANCH_SZ
BRANCH_TAN = float(np.sqrt(1.0 / BRANCH_SZ ** 2 - 1.0))      # ... i.e. alpha tan(theta_i) < 4.47e-3
F32_BELOW_1 = float(np.nextafter(np.float32(1), np.float32(0)))


def f32_params(alpha, metal):
    """What mrl_material_ggx stores (Float parameters) as Python floats for the oracle: alpha, eta[3], k[3]."""
    eta, k = METALS[metal]
    return float(np.float32(alpha)), [float(np.float32(x)) for x in eta], [float(np.float32(x)) for x in k]


# ------------------------------------------------------------------ the model
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def fresnel(c, eta, k):
    """Unpolarised reflectance of a conductor n = eta + ik at cos(theta) = c > 0, from the complex Fresnel coefficients."""
    c = np.asarray(c, np.float64)
    n = complex(eta, k)
    ct = np.sqrt(1.0 - (1.0 - c * c) / (n * n) + 0j)
    rs = (c - n * ct) / (c + n * ct)
    rp = (n * c - ct) / (n * c + ct)
    return 0.5 * (np.abs(rs) ** 2 + np.abs(rp) ** 2)


def ndf(alpha, m):
    """D(m) for unit m; zero below the macro surface."""
    t2 = (m[..., 0] ** 2 + m[..., 1] ** 2) / np.maximum(m[..., 2], 1e-300) ** 2            # tan^2(theta_m)
    cos4 = 1.0 / (1.0 + t2) ** 2
    d = 1.0 / (np.pi * alpha * alpha * cos4 * (1.0 + t2 / (alpha * alpha)) ** 2)
    return np.where(m[..., 2] > 0.0, d, 0.0)


def smith_g1(alpha, v, m):
    tan_v = np.hypot(v[..., 0], v[..., 1]) / np.abs(v[..., 2])
    g = 2.0 / (1.0 + np.sqrt(1.0 + (alpha * tan_v) ** 2))
    return np.where((v * m).sum(-1) * v[..., 2] > 0.0, g, 0.0)


def _terms(alpha, wi, wo):
    a, b = _unit(wi), _unit(wo)
    m = _unit(a + b)
    up = (np.asarray(wi)[..., 2] > 0) & (np.asarray(wo)[..., 2] > 0)
    return a, b, m, up


def pdf(alpha, wi, wo):
    """Density of the visible-normal sampler in wo (solid angle); f64.  wi, wo: finite, any length; zero below the horizon."""
    with np.errstate(all="ignore"):
        a, b, m, up = _terms(alpha, wi, wo)
        return np.where(up, ndf(alpha, m) * smith_g1(alpha, a, m) / (4.0 * a[..., 2]), 0.0)


def eval(alpha, eta, k, wi, wo):
    """f cos(theta_o) per channel; f64 [n, 3]."""
    with np.errstate(all="ignore"):
        a, b, m, up = _terms(alpha, wi, wo)
        model = ndf(alpha, m) * smith_g1(alpha, a, m) * smith_g1(alpha, b, m) / (4.0 * a[..., 2])
        c = (a * m).sum(-1)
        f = np.stack([fresnel(c, eta[ch], k[ch]) for ch in range(3)], -1)
        return np.where(up[..., None], f * model[..., None], 0.0)


def weight(alpha, eta, k, wi, wo):
    """eval / pdf = F G1(wo), in that closed form (no division of two large numbers)."""
    with np.errstate(all="ignore"):
        a, b, m, up = _terms(alpha, wi, wo)
        c = (a * m).sum(-1)
        f = np.stack([fresnel(c, eta[ch], k[ch]) for ch in range(3)], -1)
        return f * smith_g1(alpha, b, m)[..., None]


def stretched_z(alpha, wi):
    """s_z of the sampler's stretched incident direction (alpha wi.x, alpha wi.y, wi.z) / |.|, which selects its branch."""
    a = _unit(wi)
    return a[..., 2] / np.sqrt((alpha * a[..., 0]) ** 2 + (alpha * a[..., 1]) ** 2 + a[..., 2] ** 2)


# ------------------------------------------------------------------ the conditioning envelope of a sampled direction
def ulp_neighbours(wo):
    """wo [n, 3] Float and the 26 directions one ulp away from it in any subset of its components: [27, n, 3], wo first."""
    wo = np.ascontiguousarray(wo, np.float32)
    steps = (wo, np.nextafter(wo, np.float32(-np.inf)), np.nextafter(wo, np.float32(np.inf)))
    out = [wo]
    for i in range(3):
        for j in range(3):
            for k in range(3):
                if i or j or k:
                    out.append(np.stack([steps[i][:, 0], steps[j][:, 1], steps[k][:, 2]], 1))
    return np.stack(out)


def envelope(pdf_fn, weight_fn, wi, wo2):
    """[min, max] of pdf_fn(wi, wo') and weight_fn(wi, wo') over wo' = the returned Float direction and its ulp neighbours.
    A sampler computes its pdf and weight at the f64 direction and returns that direction rounded to Float; where D changes by
    1 / alpha per unit of direction (small alpha, or a half vector amplified by 1 / |wi + wo| at grazing angles) the rounding
    alone moves the pdf at the returned direction by more than 1e-6.
    The neighbourhood is the whole 3 x 3 x 3 box of one-ulp steps, not only the six axis neighbours: the f64 direction lies
    anywhere in the half-ulp cell around the returned one, and along a diagonal of that cell a pdf that is linear over it moves
    by up to 1.5 times what the largest single axis step gives.  Measured on the oracle's own samples (test_ggx_cpu.py): with
    the six axis neighbours one unit of the 33 115 accepted ones at alpha = 1e-3 lies 3.2e-6 below the range; with the box, none.
    Returns (pdf_lo, pdf_hi, w_lo, w_hi)."""
    nb = ulp_neighbours(wo2)
    p = np.stack([np.asarray(pdf_fn(wi, v), np.float64) for v in nb])
    w = np.stack([np.asarray(weight_fn(wi, v), np.float64) for v in nb])
    return p.min(0), p.max(0), w.min(0), w.max(0)


ENVELOPE_REL = 2e-6


def inside(x, lo, hi, rel=ENVELOPE_REL):
    x = np.asarray(x, np.float64)
    return (x >= lo - rel * np.abs(lo) - 1e-30) & (x <= hi + rel * np.abs(hi) + 1e-30)


# ------------------------------------------------------------------ directions
def _dir(theta, phi):
    return np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


def _tilted_mirror(theta, phi, tilt, out_of_plane):
    """The mirror direction of _dir(theta, phi) rotated by `tilt` rad, in the plane of incidence or about the in-plane tangent."""
    r = _dir(theta, phi + np.pi)
    e1 = _dir(theta + 0.5 * np.pi, phi + np.pi)                   # in the plane of incidence, towards the horizon
    e2 = np.array([-np.sin(phi + np.pi), np.cos(phi + np.pi), 0.0])
    return np.cos(tilt) * r + np.sin(tilt) * (e2 if out_of_plane else e1)


THETAS = (0.0, 1e-4, 1e-3, 0.1, 0.5, 1.0, 1.4, 1.55, 0.5 * np.pi - 1e-3, 0.5 * np.pi - 1e-5)
AZIMUTHS = tuple(k * np.pi / 4 for k in range(8)) + (2.0,)       # the axes, the diagonals, one generic
U_EDGES = ((0.0, 0.0), (0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (0.3, float(np.nextafter(np.float32(0.5), np.float32(0)))),
           (0.3, float(np.nextafter(np.float32(0.5), np.float32(1)))), (F32_BELOW_1, 0.3), (0.3, F32_BELOW_1),
           (F32_BELOW_1, F32_BELOW_1), (0.0, F32_BELOW_1), (0.71, 0.13))


def targeted_units(alpha):
    """The hand-built block of a case: (wi, wo, u, special).  `special` marks the units whose inputs are not finite upper-hemisphere
    directions (a side below the horizon, zero length, NaN, inf): both sides must return the oracle's zeros and NaNs there."""
    wi, wo, u = [], [], []
    generic_u = [(0.37, 0.81), (0.93, 0.22), (0.08, 0.64), (0.55, 0.47)]
    j = 0
    for t in THETAS:                                              # exact mirror pairs, every azimuth
        for p in AZIMUTHS:
            wi.append(_dir(t, p)); wo.append(_dir(t, p + np.pi)); u.append(generic_u[j % 4]); j += 1
    for t in THETAS:                                              # off the mirror by alpha / 10, alpha, 10 alpha: where D peaks and falls
        for p in (0.0, np.pi / 4, 2.0):
            for tilt in (0.1 * alpha, alpha, 10.0 * alpha):
                for oop in (False, True):
                    wi.append(_dir(t, p)); wo.append(_tilted_mirror(t, p, tilt, oop)); u.append(generic_u[j % 4]); j += 1
    for side in (1.0 - 1e-3, 1.0 + 1e-3):                         # either side of the sampler's branch line, 1e-3 relative away
        t = np.arctan(BRANCH_TAN * side / alpha)
        for p in (0.0, np.pi / 4, 2.0):
            for uu in generic_u:
                wi.append(_dir(t, p)); wo.append(_dir(t, p + np.pi)); u.append(uu)
    for t in (0.0, 1e-3, 0.5, 1.4, 0.5 * np.pi - 1e-3):           # the corners and edges of u
        for uu in U_EDGES:
            # at normal incidence u0 = 0.5 samples the slope 1, i.e. tan(theta_m) = alpha: at alpha = 1 the reflected direction lies
            # exactly on the horizon, and whether 2 (wi.m) m.z - 1 rounds to 0 or to +-1e-16 decides accept / reject — not under test
            tt = 1e-4 if (t == 0.0 and uu[0] == 0.5 and alpha == 1.0) else t
            wi.append(_dir(tt, 0.3)); wo.append(_dir(tt, 0.3 + np.pi)); u.append(uu)
    for s_i, s_o in ((1e-3, 1.0), (1e3, 1.0), (1.0, 1e-3), (1.0, 1e3), (1e-3, 1e3), (1e3, 1e3)):      # unnormalised
        for t, p in ((0.3, 0.7), (1.2, 4.0)):
            wi.append(s_i * _dir(t, p)); wo.append(s_o * _tilted_mirror(t, p, 0.5 * alpha, True)); u.append(generic_u[j % 4]); j += 1
    n_regular = len(wi)
    a, b = _dir(0.6, 1.0), _dir(0.4, 3.5)
    nan, inf = np.nan, np.inf
    for x, y in (((0, 0, 0), b), (a * [1, 1, -1], b), (a, b * [1, 1, -1]), (a * [1, 1, 0], b), (a, b * [1, 1, 0]),
                 ((nan, 0.1, 0.9), b), ((0.1, nan, 0.9), b), ((0.1, 0.2, nan), b), (a, (nan, 0.1, 0.9)), (a, (0.1, 0.2, nan)),
                 ((inf, 0, 1), b), ((0, 0, inf), b), ((0.1, -inf, 0.5), b), (a, (inf, 0, 1)), (a, (0, 0, inf)), (a, (0, 0, -inf)),
                 ((0, 0, -inf), b)):
        wi.append(np.asarray(x, np.float64)); wo.append(np.asarray(y, np.float64)); u.append(generic_u[j % 4]); j += 1
    special = np.zeros(len(wi), bool); special[n_regular:] = True
    with np.errstate(all="ignore"):
        return np.array(wi).astype(np.float32), np.array(wo).astype(np.float32), np.array(u, np.float32), special


def case_units(oracle, alpha, metal):
    """(wi, wo, u, special) of one case: N_RANDOM generate_pairs units (a window of their own per alpha) and the targeted block."""
    first = ALPHAS.index(alpha) * N_RANDOM
    rwi, rwo, ru = oracle.generate_pairs(SEED, first, N_RANDOM)
    twi, two, tu, special = targeted_units(alpha)
    return (np.concatenate([rwi, twi]), np.concatenate([rwo, two]), np.concatenate([ru, tu]),
            np.concatenate([np.zeros(N_RANDOM, bool), special]))


def case_id(case):
    return f"a{case[0]:g}-{case[1]}"


# ------------------------------------------------------------------ the oracle's view of a case, computed once
_REFERENCE = {}


def case_reference(oracle, alpha, metal):
    """Inputs and the oracle's outputs of a case, with the envelope of every accepted sample; cached (read-only for every test)."""
    key = (alpha, metal)
    if key not in _REFERENCE:
        al, eta, k = f32_params(alpha, metal)
        G = oracle.OracleGgx(al, eta, k)
        wi, wo, u, special = case_units(oracle, alpha, metal)
        with np.errstate(all="ignore"):
            rgb, p = G.eval(wi, wo), G.pdf(wi, wo)
            wo2, pdf2, w = G.sample(wi, u)
            acc = pdf2 > 0

            def ratio(a, b):
                return G.eval(a, b).astype(np.float64) / G.pdf(a, b).astype(np.float64)[:, None]
            env = envelope(G.pdf, ratio, wi[acc], wo2[acc])
        ref = dict(G=G, params=(al, eta, k), wi=wi, wo=wo, u=u, special=special, rgb=rgb, pdf=p, wo2=wo2, pdf2=pdf2, w=w, acc=acc, env=env)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFERENCE[key] = ref
    return _REFERENCE[key]
