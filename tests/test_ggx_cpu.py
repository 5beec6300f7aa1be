"""The oracle's GGX rough conductor against an independent f64 restatement of the published model (tests/ggx_reference.py),
and, on the oracle and the restatement alone, the conditions that tests/test_gpu_ggx.py relies on:
  * no unit of any case lies within 1e-9 of the sampler's branch line s_z = 0.99999 (0 units need dropping);
  * every chosen metal reflects at least 1e-3 at every angle, so a relative bound on eval and weight means something;
  * the oracle's own sample() outputs satisfy the conditioning envelope the device's are held to.
eval and pdf: both sides compute in f64, the oracle rounds its result to Float (6e-8): 1e-6 relative, every unit."""
import numpy as np
import pytest

from tests import ggx_reference as ref

REL = 1e-6
CASE_IDS = [ref.case_id(c) for c in ref.CASES]


def _close(got, want, rel=REL):
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    return np.abs(got - want) <= rel * np.abs(want) + 1e-30


@pytest.mark.parametrize("metal", list(ref.METALS))
def test_every_metal_reflects_at_least_1e_3(oracle, metal):
    """F >= 1e-3 over the whole cosine range, by the restatement and by the oracle (the weight F G1(wo) of its samples over G1(wo))."""
    _, eta, k = ref.f32_params(1.0, metal)
    c = np.concatenate([np.linspace(0.0, 1.0, 20001), 10.0 ** np.linspace(-12, 0, 2001)])
    for ch in range(3):
        assert ref.fresnel(c, eta[ch], k[ch]).min() >= 1e-3
    # the oracle's F: weight / G1(wo) of samples whose wo is known — at alpha = 1, over all of generate_pairs' incident directions
    G = oracle.OracleGgx(1.0, eta, k)
    wi, _, u = oracle.generate_pairs(ref.SEED, 0, 1 << 14)
    wo2, pdf2, w = G.sample(wi, u)
    acc = pdf2 > 0
    m = ref._unit(ref._unit(wi[acc]) + ref._unit(wo2[acc]))
    g1 = ref.smith_g1(1.0, ref._unit(wo2[acc]), m)
    assert (w[acc] / g1[:, None]).min() >= 1e-3


def test_fresnel_restatement_known_answers():
    """Normal incidence: ((eta - 1)^2 + k^2) / ((eta + 1)^2 + k^2); grazing: 1; a dielectric at Brewster's angle: r_p = 0."""
    for eta, k in ((0.143, 3.983), (1.5, 7.6), (1.5, 0.0), (1.3, 30.0)):
        f0 = ((eta - 1) ** 2 + k * k) / ((eta + 1) ** 2 + k * k)
        assert abs(ref.fresnel(1.0, eta, k) - f0) <= 1e-14 * f0                   # f64 rounding of a dozen operations
        assert abs(ref.fresnel(0.0, eta, k) - 1.0) <= 1e-14
    cb = np.cos(np.arctan(1.5))
    ct = np.sqrt(1 - (1 - cb * cb) / 2.25)
    rs = (cb - 1.5 * ct) / (cb + 1.5 * ct)
    assert abs(ref.fresnel(cb, 1.5, 0.0) - 0.5 * rs * rs) <= 1e-14


@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_no_unit_on_the_branch_line(oracle, case):
    """|s_z - 0.99999| >= 1e-9 for every unit: within rounding of the line two correct samplers may branch differently, which no
    test here provokes.  Both branches are populated by the hand-built block at every alpha."""
    alpha, metal = case
    al = ref.f32_params(alpha, metal)[0]
    wi, _, _, special = ref.case_units(oracle, alpha, metal)
    sz = ref.stretched_z(al, wi[~special].astype(np.float64))
    assert np.isfinite(sz).all()
    assert np.abs(sz - ref.BRANCH_SZ).min() >= 1e-9
    twi = wi[ref.N_RANDOM:][~special[ref.N_RANDOM:]].astype(np.float64)
    tsz = ref.stretched_z(al, twi)
    near = np.abs(tsz - ref.BRANCH_SZ) < 1e-7
    assert (tsz[near] > ref.BRANCH_SZ).sum() >= 12 and (tsz[near] < ref.BRANCH_SZ).sum() >= 12


@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_oracle_eval_and_pdf_match_the_restatement(oracle, case):
    alpha, metal = case
    r = ref.case_reference(oracle, alpha, metal)
    al, eta, k = r["params"]
    ok = ~r["special"]
    wi, wo = r["wi"][ok], r["wo"][ok]
    want_pdf = ref.pdf(al, wi, wo)
    want_rgb = ref.eval(al, eta, k, wi, wo)
    assert (want_pdf[(wi[:, 2] > 0) & (wo[:, 2] > 0)] > 0).all()
    assert _close(r["pdf"][ok], want_pdf).all(), np.abs(r["pdf"][ok] / want_pdf - 1)[want_pdf > 0].max()
    assert _close(r["rgb"][ok], want_rgb).all()
    # below the horizon, zero length: exact zeros; NaN in, NaN or zero out — never a finite non-zero value
    sp = r["special"]
    assert not (np.isfinite(r["rgb"][sp]) & (r["rgb"][sp] != 0)).any() and not (np.isfinite(r["pdf"][sp]) & (r["pdf"][sp] != 0)).any()
    assert not r["wo2"][sp & ~r["acc"]].any() and not r["w"][sp & ~r["acc"]].any()


@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_oracle_samples_match_the_restatement_at_the_returned_direction(oracle, case):
    """pdf2 and weight of every accepted sample lie inside the envelope — [min, max] over the returned Float direction and its 26
    one-ulp neighbours, widened by 2e-6 — of the restatement's pdf and F G1(wo), and inside the envelope of the oracle's own
    pdf() and eval() / pdf(), which is what the device's samples are held to."""
    alpha, metal = case
    r = ref.case_reference(oracle, alpha, metal)
    al, eta, k = r["params"]
    acc = r["acc"]
    assert acc.sum() > 0.3 * acc.size
    assert np.abs(np.linalg.norm(r["wo2"][acc].astype(np.float64), axis=1) - 1).max() < 3e-7      # Float rounding of a unit vector
    wi, wo2, pdf2, w = r["wi"][acc], r["wo2"][acc], r["pdf2"][acc], r["w"][acc]
    lo, hi, wlo, whi = ref.envelope(lambda a, b: ref.pdf(al, a, b), lambda a, b: ref.weight(al, eta, k, a, b), wi, wo2)
    bad = ~ref.inside(pdf2, lo, hi)
    assert not bad.any(), (int(bad.sum()), wi[bad][:3], r["u"][acc][bad][:3], pdf2[bad][:3], lo[bad][:3], hi[bad][:3])
    assert ref.inside(w, wlo, whi).all()
    lo, hi, wlo, whi = r["env"]
    assert np.isfinite(lo).all() and np.isfinite(whi).all() and (lo > 0).all()
    assert ref.inside(pdf2, lo, hi).all() and ref.inside(w, wlo, whi).all()


# ------------------------------------------------------------------ the pdf is a density
def _hemisphere_integral(alpha, theta_i, n_t, n_p):
    """Midpoint rule for the integral of ref.pdf(wi, .) over the upper hemisphere, in polar coordinates (theta', phi') about the
    mirror direction: for each phi' the polar angle runs from 0 to where the direction meets the horizon, theta_max(phi') =
    atan2(cos(theta_r), sin(theta_r) cos(phi')), on a sinh-graded grid that puts half its nodes within ~alpha of the mirror."""
    wi = np.array([np.sin(theta_i), 0.0, np.cos(theta_i)])
    r = np.array([-np.sin(theta_i), 0.0, np.cos(theta_i)])
    e1 = np.array([-np.cos(theta_i), 0.0, -np.sin(theta_i)])        # in the plane of incidence, towards the horizon
    e2 = np.array([0.0, 1.0, 0.0])
    t = (np.arange(n_t) + 0.5) / n_t
    ph = (np.arange(n_p) + 0.5) * (2 * np.pi / n_p)
    t_max = np.arctan2(np.cos(theta_i), np.sin(theta_i) * np.cos(ph))[None, :]
    scale = min(alpha, 0.5)
    s = np.arcsinh(t_max / scale)
    th = scale * np.sinh(t[:, None] * s)
    dth = scale * np.cosh(t[:, None] * s) * s
    wo = (np.cos(th)[..., None] * r + np.sin(th)[..., None] * (np.cos(ph)[None, :, None] * e1 + np.sin(ph)[None, :, None] * e2))
    wo[..., 2] = np.maximum(wo[..., 2], 1e-300)                     # the last node of a ray sits a rounding error above the horizon
    p = ref.pdf(alpha, np.broadcast_to(wi, wo.shape), wo)
    return float((p * np.sin(th) * dth).sum() * (1.0 / n_t) * (2 * np.pi / n_p))


@pytest.mark.parametrize("theta_deg", [0.0, 45.0, 85.0])
@pytest.mark.parametrize("alpha", [a for a in ref.ALPHAS if a >= 0.01])
def test_pdf_is_a_density(oracle, alpha, theta_deg):
    """The restatement's pdf integrated over the hemisphere (640 x 512 midpoint grid; 320 x 256 for its own error) plus the
    fraction of 2^18 oracle samples that were rejected equals 1.  The bound is three times the larger of the two grids'
    difference and the binomial error sqrt(p (1 - p) / 2^18) of the rejected fraction.
    Measured (integral + rejected - 1 | grid difference | binomial error), theta_i = 0 / 45 / 85 degrees:
      alpha 0.01: +3.1e-5 | 5.1e-6 | 2.2e-5,  +1.9e-5 | 7.0e-6 | 2.3e-5,  +3.9e-5 | 4.6e-5 | 1.1e-4
      alpha 0.05: -1.7e-5 | 2.7e-6 | 9.7e-5,  -6.8e-5 | 3.7e-6 | 1.1e-4,  +5.5e-4 | 2.2e-5 | 3.4e-4
      alpha 0.3:  +4.4e-4 | 1.5e-6 | 5.4e-4,  +2.2e-4 | 1.7e-6 | 5.5e-4,  -1.2e-4 | 6.0e-6 | 3.2e-4
      alpha 1:    +4.0e-4 | 7.0e-7 | 9.8e-4,  -3.6e-4 | 2.6e-7 | 9.6e-4,  -9.5e-4 | 7.1e-6 | 5.3e-4
      alpha 2:    +5.3e-4 | 1.6e-6 | 7.8e-4,  -2.3e-5 | 3.0e-6 | 8.8e-4,  -3.4e-4 | 1.4e-5 | 7.1e-4
    The binomial error is the larger one in every case.  At normal incidence the integral has the closed form 1 / (1 + alpha^2)
    (the visible normals within 45 degrees of the surface normal): 0.4999998 at alpha = 1 and 0.1999995 at alpha = 2."""
    theta = np.deg2rad(theta_deg)
    fine = _hemisphere_integral(alpha, theta, 640, 512)
    coarse = _hemisphere_integral(alpha, theta, 320, 256)
    n = 1 << 18
    G = oracle.OracleGgx(alpha, *ref.f32_params(alpha, "gold")[1:])
    _, _, u = oracle.generate_pairs(ref.SEED, 1 << 30, n)
    wi = np.tile(np.array([[np.sin(theta), 0.0, np.cos(theta)]], np.float32), (n, 1))
    _, pdf2, _ = G.sample(wi, u)
    rejected = float((pdf2 <= 0).mean())
    mc = float(np.sqrt(rejected * (1 - rejected) / n))
    grid = abs(fine - coarse)
    tol = 3.0 * max(grid, mc)
    print(f"alpha {alpha:g} theta_i {theta_deg:g}: integral {fine:.9f} + rejected {rejected:.9f} - 1 = {fine + rejected - 1:+.3e}; "
          f"grid difference {grid:.3e}, MC error {mc:.3e}, bound {tol:.3e}")
    assert abs(fine + rejected - 1.0) <= tol
