"""The RGL model's one known answer, on the CPU: oracle/rgl_oracle.c evaluates an analytic GGX conductor tabulated in the file format
(tests/rgl_ggx_reference.py) and must return the conductor's closed-form eval, pdf and weights up to the discretisation error of the
tables.  A misreading of the format shared by the oracle and the kernels (a mirrored azimuth, swapped table axes, theta2u on the
wrong angle, the 4 sigma in the wrong place, a wrong sign on the way out of a symmetry-reduced file) passes every parity test and
fails here; tests/test_gpu_rgl_ggx.py holds the device to the same truth at the same bars.

Error: |value - truth| / (truth + 1e-3 max truth), over every value of every unit of a case's fixed direction set (4096 units:
generate_pairs pairs with both polar angles <= 1.2 rad — the horizon cut-off of rgb is a discontinuity bilinear tables cannot hold —
and 63 hand-built rows: normal incidence, theta_i on and between nodes, phi_i on a node, at the seam, in every quadrant, mirror
pairs).  No unit is left out.  "sample pdf" is the pdf a sample reports against the truth at the direction it returns (directions
within 1.2 rad), "weight" the luminance of an accepted sample's weight against the albedo luminance L-bar(wi) (for the spectral
file: every wavelength against colour(wl) L-bar / mean colour).

The bars are discretisation errors, so they are MEASURED on the oracle and held at 1.5 x the measured value (MEASURED below; the
margin covers the 1e-6 by which device and oracle may differ and the choice of statistic).  Measured, median / p99:

  case              file (n_phi x n_theta x res^2, ndf)   eval             pdf              sample pdf       weight
  iso_a0.3          1 x 16 x 32^2, 64^2                   1.54e-3 1.33e-2  1.66e-3 1.74e-2  2.19e-3 2.77e-2  2.96e-3 2.65e-2
  iso_a0.5          1 x 16 x 32^2, 64^2                   5.20e-4 5.60e-3  2.08e-3 1.51e-2  2.14e-3 2.26e-2  2.13e-3 1.80e-2
  iso_a0.5_coarse   1 x  8 x 16^2, 32^2                   2.22e-3 2.49e-2  9.10e-3 6.14e-2  9.46e-3 1.00e-1  9.71e-3 8.64e-2
  iso_a0.5_uneven   1 x 16 x 32^2, 64^2, uneven theta_i   5.65e-4 5.67e-3  2.01e-3 1.48e-2  2.16e-3 2.14e-2  2.15e-3 1.77e-2
  aniso_full        17 x 12 x 32^2, 64^2                  3.29e-3 6.41e-2  8.46e-3 9.10e-2  6.23e-3 5.04e-2  5.85e-3 4.61e-2
  aniso_red2        9 x 12 x 32^2, 64^2, phi_i <= 0       3.37e-3 5.63e-2  8.55e-3 8.66e-2  6.51e-3 5.07e-2  5.97e-3 4.50e-2
  aniso_red4        5 x 12 x 32^2, 64^2, phi_i <= -pi/2   3.15e-3 3.66e-2  8.47e-3 6.45e-2  6.59e-3 5.58e-2  5.78e-3 4.84e-2
  aniso_uneven      17 x 12 x 32^2, 64^2, uneven grids    3.40e-3 5.18e-2  8.84e-3 7.81e-2  6.61e-3 5.52e-2  5.88e-3 4.80e-2
  spectral          1 x 16 x 5 x 32^2, 64^2, W = 4        8.19e-4 8.21e-3  1.55e-3 1.35e-2  1.98e-3 2.37e-2  2.34e-3 2.06e-2

(the ndf table has twice the nodes of the others per axis: D is the steepest table, and at 32^2 it alone sets the median, 1.1e-2 for
the anisotropic files.)  Sampling 4096 times at each of three fixed wi (FIXED_WI), the mean luminance of the weights is within
MEASURED_FIXED[case][0] of L-bar(wi) from a quadrature of its own and its spread (std / mean) is MEASURED_FIXED[case][1].

Teeth (aniso_full, 3.29e-3 median): the same file against the truth of alpha = (0.5, 0.25) has a median error of 0.80; a file whose
slices were built for the incident azimuth -phi_i has 0.14 against the unmirrored truth, the file with x and y of every table
swapped 0.99 — 160 x, 29 x and 200 x the bar.
Convergence (iso_a0.5): the p99 eval error at (16 nodes, 32^2) is 0.23 x that at (8 nodes, 16^2); bilinear tables are second order.
"""
import numpy as np
import pytest

from tests import rgl_ggx_reference as R

MARGIN = 1.5
MEASURED = {   # case: {figure: (median, p99)}, oracle/rgl_oracle.c against the truth
    "iso_a0.3": {"eval": (1.543e-03, 1.335e-02), "pdf": (1.659e-03, 1.740e-02), "sample_pdf": (2.186e-03, 2.770e-02), "weight": (2.957e-03, 2.652e-02)},
    "iso_a0.5": {"eval": (5.200e-04, 5.604e-03), "pdf": (2.082e-03, 1.511e-02), "sample_pdf": (2.137e-03, 2.257e-02), "weight": (2.134e-03, 1.800e-02)},
    "iso_a0.5_coarse": {"eval": (2.221e-03, 2.485e-02), "pdf": (9.105e-03, 6.142e-02), "sample_pdf": (9.459e-03, 1.002e-01), "weight": (9.713e-03, 8.636e-02)},
    "iso_a0.5_uneven": {"eval": (5.649e-04, 5.668e-03), "pdf": (2.009e-03, 1.481e-02), "sample_pdf": (2.155e-03, 2.143e-02), "weight": (2.145e-03, 1.772e-02)},
    "aniso_full": {"eval": (3.287e-03, 6.405e-02), "pdf": (8.458e-03, 9.101e-02), "sample_pdf": (6.231e-03, 5.036e-02), "weight": (5.849e-03, 4.606e-02)},
    "aniso_red2": {"eval": (3.375e-03, 5.629e-02), "pdf": (8.552e-03, 8.659e-02), "sample_pdf": (6.513e-03, 5.072e-02), "weight": (5.971e-03, 4.499e-02)},
    "aniso_red4": {"eval": (3.148e-03, 3.664e-02), "pdf": (8.472e-03, 6.449e-02), "sample_pdf": (6.591e-03, 5.581e-02), "weight": (5.784e-03, 4.840e-02)},
    "aniso_uneven": {"eval": (3.395e-03, 5.181e-02), "pdf": (8.840e-03, 7.807e-02), "sample_pdf": (6.612e-03, 5.522e-02), "weight": (5.882e-03, 4.803e-02)},
    "spectral": {"eval": (8.192e-04, 8.210e-03), "pdf": (1.553e-03, 1.346e-02), "sample_pdf": (1.980e-03, 2.365e-02), "weight": (2.337e-03, 2.059e-02)},
}
MEASURED_FIXED = {   # case: (|mean Y(weight) / L-bar - 1|, std / mean of Y(weight)), the largest over FIXED_WI
    "iso_a0.3": (2.467e-03, 7.911e-03),
    "iso_a0.5": (1.379e-03, 6.893e-03),
    "iso_a0.5_coarse": (5.324e-03, 2.398e-02),
    "iso_a0.5_uneven": (1.044e-03, 6.886e-03),
    "aniso_full": (5.540e-03, 1.491e-02),
    "aniso_red2": (5.540e-03, 1.491e-02),
    "aniso_red4": (5.540e-03, 1.491e-02),
    "aniso_uneven": (5.985e-03, 1.416e-02),
    "spectral": (1.766e-03, 7.310e-03),
}
TESTED = [c for c in MEASURED]
QUADRANTS = ((1, 1), (-1, 1), (-1, -1), (1, -1))


def bars(case):
    """{figure: (median bar, p99 bar)}: 1.5 x what the oracle measures (tests/test_gpu_rgl_ggx.py imports these, it sets none)"""
    return {k: (MARGIN * v[0], MARGIN * v[1]) for k, v in MEASURED[case].items()}


def fixed_bars(case):
    return tuple(MARGIN * v for v in MEASURED_FIXED[case])


def assert_within(got, bar, what):
    """every figure of got within its bar; prints them first (run with -s to read them)"""
    for k in sorted(got):
        print(f"{what} {k}: " + " ".join(f"{g:.3e} (bar {b:.3e})" for g, b in zip(got[k], bar[k])))
    for k in got:
        assert all(g <= b for g, b in zip(got[k], bar[k])), (what, k, got[k], bar[k])


_ORACLE_OUT = {}


def oracle_outputs(oracle, case):
    """(values, pdf, wo2, pdf2, weight, wl) of the oracle on the case's direction set; cached, read-only"""
    if case not in _ORACLE_OUT:
        fields, g = R.case_file(case)
        wi, wo, u = R.case_units(oracle, case)
        orc = oracle.OracleRgl(fields)
        if g.colour is None:
            wl = None
            out = orc.eval_pdf(wi, wo) + orc.sample(wi, u)
        else:
            wl = R.case_wavelengths(case, len(wi))
            out = orc.eval_pdf_spectral(wi, wo, wl) + orc.sample_spectral(wi, u, wl)
        _ORACLE_OUT[case] = out + (wl,)
    return _ORACLE_OUT[case]


# ------------------------------------------------------------------ the reference holds itself
def test_forward_warp_is_the_oracles():
    """the numpy forward warp that places rgb against oracle.binding.OracleWarp.sample, on slices of the anisotropic file"""
    from oracle.binding import OracleWarp
    vndf = R.case_file("aniso_red4")[0]["vndf"]
    slices = vndf.reshape(-1, *vndf.shape[-2:])[[0, 7, 23, 41, 59]]
    rng = np.random.default_rng(5)
    ux, uy = np.concatenate([rng.random(60), [0.0, 1.0, 0.0, 1.0]]), np.concatenate([rng.random(60), [0.0, 0.0, 1.0, 1.0]])
    px, py = R.forward_warp(slices, ux, uy)
    for s, data in enumerate(slices):
        w = OracleWarp(data)
        for k in range(len(ux)):
            (x, y), _ = w.sample((ux[k], uy[k]))
            # the oracle's cdf tables are Float; at the corners ux = 1 the last cell holds next to no mass (D at the horizon) and
            # that rounding moves the point within the cell
            tol = 2e-5 if k < 60 else 1e-3
            assert abs(x - px[s, k]) < tol and abs(y - py[s, k]) < tol, (s, k, x, px[s, k], y, py[s, k])


def test_albedo_quadrature_and_interpolant():
    """L-bar by quadrature against itself at twice the resolution, and the interpolant pdf_truth divides by against direct quadratures"""
    for name in ("iso_a0.3", "aniso_full", "spectral"):
        g = R.case_file(name)[1]
        wi = R.direction(np.array([0.0, 0.13, 0.6, 0.9, 1.2, 1.47]), np.array([0.0, 2.9, 0.3, -1.1, -2.0, 1.0]))
        a, b = g.albedo_luminance(wi), g.albedo_luminance(wi, 128, 768)
        assert float(np.abs(a / b - 1.0).max()) < 1e-7
        assert float(np.abs(g.albedo_luminance_at(wi) / b - 1.0).max()) < 1e-6
        assert 0.3 < float(b.min()) and float(b.max()) < 1.0


def test_truth_is_the_ggx_reference_when_isotropic():
    """the isotropic truth is tests/ggx_reference.py's eval (itself tested against the GGX kernels at 1e-6); the density of visible
    normals integrates to one"""
    from tests import ggx_reference as gref
    from oracle import binding
    wi, wo, _ = R.case_units(binding, "iso_a0.5")
    g = R.case_file("iso_a0.5")[1]
    want = gref.eval(0.5, *R.GOLD, wi, wo)
    assert float(np.abs(g.eval_truth(wi, wo) / want - 1.0).max()) < 1e-12
    a = R.Ggx(0.25, 0.5)
    x, w = np.polynomial.legendre.leggauss(128)
    phi = (np.arange(512) + 0.5) * (2 * np.pi / 512)
    m = R.direction(np.arccos(0.5 * (x + 1))[:, None], phi[None, :])
    for v in R.direction(np.array([0.0, 0.7, 1.3]), np.array([0.0, 0.9, -2.0])):
        d_vis = a.D(m) * np.maximum((m * v).sum(-1), 0.0) / a.sigma(v)
        assert abs(float((d_vis * (0.5 * w)[:, None]).sum() * (2 * np.pi / 512)) - 1.0) < 1e-4


# ------------------------------------------------------------------ the oracle against the truth
@pytest.mark.parametrize("case", TESTED)
def test_oracle_reproduces_the_conductor(oracle, case):
    fields, g = R.case_file(case)
    wi, wo, u = R.case_units(oracle, case)
    values, pdf, wo2, pdf2, weight, wl = oracle_outputs(oracle, case)
    assert_within(R.measure(g, wi, wo, values, pdf, wo2, pdf2, weight, wl), bars(case), case)


@pytest.mark.parametrize("case", TESTED)
def test_weights_at_fixed_wi_carry_the_albedo(oracle, case):
    fields, g = R.case_file(case)
    wi, u = R.fixed_wi_units(oracle)
    orc = oracle.OracleRgl(fields)
    wo2, pdf2, weight = orc.sample(wi, u) if g.colour is None else orc.sample_spectral(wi, u)
    got = R.measure_fixed_wi(g, wi, pdf2, weight)
    assert_within({"fixed_wi": got}, {"fixed_wi": fixed_bars(case)}, case)


def test_spectral_interpolation_is_exact(oracle):
    """the colour factor is linear in the wavelength, so on, between and outside the nodes (clamped to the end node's colour) the
    value is the first column's times colour(wl) / colour(wl_0): Float rounding only"""
    g = R.case_file("spectral")[1]
    values, _, _, pdf2, weight, wl = oracle_outputs(oracle, "spectral")
    for v, keep in ((np.asarray(values, np.float64), slice(None)), (np.asarray(weight, np.float64), pdf2 > 0)):
        v, w = v[keep], wl[keep]
        assert float((v[:, 0] > 0).mean()) == 1.0
        want = g.colour_at(w) / g.colour_at(w[:, :1])
        assert float(np.abs(v / v[:, :1] / want - 1.0).max()) < 1e-6
    outside = (wl[:, 3] < g.wavelengths[0]) | (wl[:, 3] > g.wavelengths[-1])
    assert outside.all() and np.isin(wl[:, 0], g.wavelengths.astype(np.float32)).all()


def test_error_falls_with_resolution(oracle):
    fine = R.measure(R.case_file("iso_a0.5")[1], *R.case_units(oracle, "iso_a0.5")[:2], *oracle_outputs(oracle, "iso_a0.5")[:5])["eval"][1]
    coarse = R.measure(R.case_file("iso_a0.5_coarse")[1], *R.case_units(oracle, "iso_a0.5_coarse")[:2], *oracle_outputs(oracle, "iso_a0.5_coarse")[:5])["eval"][1]
    print(f"p99 eval error: {coarse:.3e} at (8 nodes, 16^2), {fine:.3e} at (16 nodes, 32^2): ratio {fine / coarse:.3f}")
    assert fine <= 0.5 * coarse


def test_teeth_swapped_roughness_and_mirrored_azimuth(oracle):
    """the check can fail: a file of alpha = (0.25, 0.5) against the truth of (0.5, 0.25), and a file whose phi_i nodes were built
    mirrored against the unmirrored truth, miss the case's own bar by more than a factor 10 in the median; so does the file with
    the two axes of every table swapped"""
    fields, g = R.case_file("aniso_full")
    wi, wo, u = R.case_units(oracle, "aniso_full")
    bar = bars("aniso_full")["eval"][0]
    swapped = R.med_p99(oracle_outputs(oracle, "aniso_full")[0], R.Ggx(0.5, 0.25).eval_truth(wi, wo))[0]
    mirrored_file = R.case_file("aniso_mirrored")[0]
    assert np.array_equal(mirrored_file["phi_i"], fields["phi_i"]) and not np.array_equal(mirrored_file["vndf"], fields["vndf"])
    mirrored = R.med_p99(oracle.OracleRgl(mirrored_file).eval_pdf(wi, wo)[0], g.eval_truth(wi, wo))[0]
    transposed_file = {k: (np.ascontiguousarray(np.swapaxes(v, -1, -2)) if v.ndim >= 2 else v) for k, v in fields.items()}      # x and y of every table swapped
    transposed = R.med_p99(oracle.OracleRgl(transposed_file).eval_pdf(wi, wo)[0], g.eval_truth(wi, wo))[0]
    print(f"median eval error: bar {bar:.3e}, swapped roughness {swapped:.3e}, mirrored phi_i {mirrored:.3e}, transposed tables {transposed:.3e}")
    assert swapped >= 10.0 * bar and mirrored >= 10.0 * bar and transposed >= 10.0 * bar


@pytest.mark.parametrize("case", ["aniso_full", "aniso_red2", "aniso_red4"])
def test_reduced_files_describe_the_same_material_in_every_quadrant(oracle, case):
    """an anisotropic GGX has the point symmetry and both mirror planes: the files that store a half / a quarter of the azimuth
    meet the full file's truth in every quadrant of wi — no quadrant's median beyond the bar, none worse than twice the best"""
    g = R.case_file(case)[1]
    wi, wo, u = R.case_units(oracle, case)
    values = oracle_outputs(oracle, case)[0]
    truth = g.eval_truth(wi, wo)
    err = (np.abs(values - truth) / (truth + 1e-3 * truth.max())).reshape(len(wi), -1)
    med = []
    for sx, sy in QUADRANTS:
        q = (np.signbit(wi[:, 0]) == (sx < 0)) & (np.signbit(wi[:, 1]) == (sy < 0))
        assert q.sum() > 500
        med.append(float(np.median(err[q])))
    print(case, "median eval error per quadrant of wi:", " ".join(f"{m:.3e}" for m in med))
    assert max(med) <= bars(case)["eval"][0] and max(med) <= 2.0 * min(med)
    qwi, qu = R.quadrant_units(oracle)
    wo2, pdf2, _ = oracle.OracleRgl(R.case_file(case)[0]).sample(qwi, qu)
    R.assert_lobes_face_wi(qwi, wo2, pdf2)
