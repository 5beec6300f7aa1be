"""The RGL adaptive-parameterisation BSDF (the "*.bsdf tensor format of upstream M3 `measured`") — the
oracle's restatement (oracle/rgl_oracle.c) pinned by self-consistency on the CPU.  PARITY UNPINNED: no measured file, no upstream
plugin and no reference vector exist in the container; what is checked is that the restated model is a consistent
distribution machinery — the piecewise-bilinear warp's sample / invert / eval agree with each other and with closed forms, the
BSDF's pdf is a density, sample() reports it, weight == eval / pdf."""
import numpy as np
import pytest

from mitsuba_customization_amd import synth
from oracle import binding as ob


def test_constant_warp_is_the_identity():
    w = ob.OracleWarp(np.ones((5, 7), np.float32))
    for u in ((0.3, 0.8), (0.0, 0.0), (0.999, 0.001), (0.5, 0.5)):
        pos, pdf = w.sample(u)
        assert np.allclose(pos, u, atol=1e-7) and abs(pdf - 1) < 1e-6
        assert np.allclose(w.invert(u)[0], u, atol=1e-7) and abs(w.eval(u) - 1) < 1e-6


@pytest.mark.parametrize("params", [(), (0.3, 0.6)])
def test_sample_and_invert_are_inverse_and_agree_with_eval(params):
    rng = np.random.default_rng(3)
    grids = [np.array([0.0, 0.5, 1.0], np.float32), np.array([0.0, 0.2, 0.7, 1.0], np.float32)][:len(params)]
    shape = tuple(len(g) for g in grids) + (9, 13)
    w = ob.OracleWarp((rng.random(shape) + 0.05).astype(np.float32), grids)
    for u in rng.random((400, 2)):
        pos, pdf = w.sample(u, params)
        back, pdf2 = w.invert(pos, params)
        assert np.allclose(back, u, atol=2e-9), (u, pos, back)
        assert abs(pdf - pdf2) <= 1e-12 * pdf and abs(pdf - w.eval(pos, params)) <= 1e-12 * pdf
        assert 0 <= pos[0] <= 1 and 0 <= pos[1] <= 1
    # the density integrates to one at interpolated parameters: a bilinear patch integrates to the mean of its corners
    ny, nx = 9, 13
    tot = sum(0.25 * (w.eval((x / (nx - 1), y / (ny - 1)), params) + w.eval(((x + 1) / (nx - 1), y / (ny - 1)), params) +
                      w.eval((x / (nx - 1), (y + 1) / (ny - 1)), params) + w.eval(((x + 1) / (nx - 1), (y + 1) / (ny - 1)), params))
              for x in range(nx - 1) for y in range(ny - 1)) / ((nx - 1) * (ny - 1))
    assert abs(tot - 1) < 2e-6


def test_unnormalised_warp_is_bilinear_interpolation_of_the_data():
    rng = np.random.default_rng(9)
    d = rng.random((6, 5)).astype(np.float32)
    w = ob.OracleWarp(d, normalize=False, build_cdf=False)
    for x, y in rng.random((100, 2)):
        px, py = x * 4, y * 5
        i, j = min(int(px), 3), min(int(py), 4)
        fx, fy = px - i, py - j
        want = (1 - fy) * ((1 - fx) * d[j, i] + fx * d[j, i + 1]) + fy * ((1 - fx) * d[j + 1, i] + fx * d[j + 1, i + 1])
        assert abs(w.eval((x, y)) - want) < 1e-12
    # a parameter exactly on a grid node selects that slice (the rgb channel axis works that way)
    s = rng.random((3, 4, 4)).astype(np.float32)
    w3 = ob.OracleWarp(s, [np.array([0, 1, 2], np.float32)], normalize=False, build_cdf=False)
    for c in range(3):
        assert abs(w3.eval((0.0, 0.0), (float(c),)) - s[c, 0, 0]) < 1e-12


@pytest.mark.parametrize("n_phi,reduction", [(1, 1), (5, 1), (4, 2), (3, 4)])
def test_bsdf_pdf_is_a_density_and_sample_reports_it(n_phi, reduction):
    B = ob.OracleRgl(synth.make_rgl_fields(4, n_phi=n_phi, reduction=reduction))
    rng = np.random.default_rng(21)
    for mu, az in ((0.95, 0.3), (0.6, -2.0), (0.25, 1.1)):
        wi1 = np.array([np.sqrt(1 - mu * mu) * np.cos(az), np.sqrt(1 - mu * mu) * np.sin(az), mu], np.float32)
        nz, nphi = 300, 360
        z = (np.arange(nz) + 0.5) / nz
        ph = (np.arange(nphi) + 0.5) / nphi * 2 * np.pi - np.pi
        Z, P = np.meshgrid(z, ph, indexing="ij")
        r = np.sqrt(1 - Z * Z)
        wo = np.stack([r * np.cos(P), r * np.sin(P), Z], -1).reshape(-1, 3).astype(np.float32)
        rgb, pdf = B.eval_pdf(np.tile(wi1, (wo.shape[0], 1)), wo)
        assert (rgb >= 0).all() and np.isfinite(rgb).all() and (pdf >= 0).all()
        u = rng.random((200000, 2)).astype(np.float32)
        s_wo, s_pdf, s_w = B.sample(np.tile(wi1, (u.shape[0], 1)), u)
        live = s_pdf > 0
        # The pdf over directions has an integrable singularity at the mirror direction (the map u_m -> wo has Jacobian
        # 2 pi^2 u sin(theta_m) 4 wi.m -> 0), which a quadrature over directions under-integrates; in the domain of the warp the
        # same integral is smooth: the mass of u_m whose reflected direction is above the horizon == the accepted fraction.
        import ctypes as C
        L = ob._rgl_lib()
        wi_d = wi1.astype(np.float64) / np.linalg.norm(wi1.astype(np.float64))
        if reduction >= 2:                                          # into the stored part of the azimuth (the mass is the same there)
            sy = 1.0 if np.signbit(wi_d[1]) else -1.0
            sx = (1.0 if np.signbit(wi_d[0]) else -1.0) if reduction == 4 else sy
            wi_d = wi_d * np.array([sx, sy, 1.0])
        theta_i = 2 * np.arcsin(min(1.0, 0.5 * np.linalg.norm(wi_d - np.array([0, 0, 1.0]))))
        phi_i = np.arctan2(wi_d[1], wi_d[0])
        par = (C.c_double * 3)(phi_i, theta_i, 0.0)
        G = 160
        mass = 0.0
        for a in range(G):
            for b in range(G):
                um = ((a + 0.5) / G, (b + 0.5) / G)
                theta_m = um[0] ** 2 * np.pi / 2
                phi_m = (2 * um[1] - 1) * np.pi + (phi_i if n_phi <= 2 else 0.0)
                m = np.array([np.cos(phi_m) * np.sin(theta_m), np.sin(phi_m) * np.sin(theta_m), np.cos(theta_m)])
                c = float(wi_d @ m)
                if c <= 0 or (2 * c * m - wi_d)[2] <= 0:
                    continue
                smp = (C.c_double * 2)(); vp = C.c_double()
                L.rgl_warp_invert(C.byref(B.c.vndf), (C.c_double * 2)(*um), par, smp, C.byref(vp))
                mass += vp.value * L.rgl_warp_eval(C.byref(B.c.luminance), smp, par)
        mass /= G * G
        assert abs(mass - live.mean()) < 0.01, (mu, mass, live.mean())
        # sample() reports pdf(wi, wo') and weight == eval / pdf, exactly
        e_rgb, e_pdf = B.eval_pdf(np.tile(wi1, (int(live.sum()), 1)), s_wo[live])
        assert np.array_equal(e_pdf, s_pdf[live]) and np.array_equal(s_w[live], (e_rgb / e_pdf[:, None]).astype(np.float32))
        # the estimator's mean equals the quadrature of eval (f cos) over the hemisphere
        albedo_q = rgb.astype(np.float64).mean(axis=0) * 2 * np.pi
        albedo_s = s_w.astype(np.float64).mean(axis=0)
        assert np.allclose(albedo_q, albedo_s, rtol=0.03), (albedo_q, albedo_s)


def test_guards():
    B = ob.OracleRgl(synth.make_rgl_fields(1))
    wi = np.array([[0, 0, -1], [0.3, 0.1, 0.9]], np.float32)
    wo = np.array([[0.1, 0.2, 0.9], [0.1, 0.2, -0.9]], np.float32)
    rgb, pdf = B.eval_pdf(wi, wo)
    assert not rgb.any() and not pdf.any()
    s_wo, s_pdf, s_w = B.sample(wi[:1], np.array([[0.3, 0.4]], np.float32))
    assert not s_wo.any() and not s_pdf.any() and not s_w.any()


# ------------------------------------------------------------------ the product's per-unit functions compiled for the host
def _host_harness(tmp_path_factory):
    """tests/rgl_host_harness.hip built once per session"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = tmp_path_factory.getbasetemp() / "rgl_host_harness"
    if not build.exists():
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-mavx2", "-mfma", "-w", "-o", str(build),
                               os.path.join(root, "tests", "rgl_host_harness.hip")])
    return build


def _write_fields(path, f):
    """the harness's fields.bin: n_phi n_theta, then (nx, ny) of vndf / ndf / sigma read off the arrays' shapes, jacobian[, n_wavelengths]"""
    spectral = "spectra" in f
    vn = f["vndf"].shape
    head = [vn[0], vn[1], vn[3], vn[2], f["ndf"].shape[1], f["ndf"].shape[0], f["sigma"].shape[1], f["sigma"].shape[0], 1]
    names = ("phi_i", "theta_i", "ndf", "sigma", "vndf", "luminance") + (("spectra", "wavelengths") if spectral else ("rgb",))
    with open(path, "wb") as o:
        np.array(head + ([f["wavelengths"].shape[0]] if spectral else []), np.int32).tofile(o)
        for k in names:
            np.ascontiguousarray(f[k], np.float32).tofile(o)


def _run_host(build, tmp, f, wi, wo, u):
    """the harness's n x 11 floats (rgb pdf | wo' pdf' weight') for an RGB file"""
    import subprocess
    _write_fields(tmp / "f.bin", f)
    n = wi.shape[0]
    with open(tmp / "p.bin", "wb") as o:
        np.array([n], np.uint64).tofile(o); wi.tofile(o); wo.tofile(o); u.tofile(o)
    r = subprocess.run([str(build), str(tmp / "f.bin"), str(tmp / "p.bin"), str(tmp / "o.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(tmp / "o.bin", np.float32).reshape(n, 11)


def _host_close(a, b, what):
    b = np.asarray(b, np.float64)
    err = np.abs(a.astype(np.float64) - b) / (np.abs(b) + 0.1 * max(float(np.abs(b).max()), 1e-30))
    assert float(err.max()) < 1e-6, (what, float(err.max()), int(err.argmax()))


def _host_matches_oracle(out, orc, wi, wo, u, min_live=0.5, faint=0.0):
    """The host tolerances: eval / pdf to 1e-6 (of the value, or of a tenth of the batch's largest); the sampled direction to 5e-7
    absolute, its pdf and weight against the oracle evaluated AT the product's direction; at most two units sampled live on one side only.
    faint > 0: a sample whose pdf is below faint x the batch's largest (one drawn onto the edge of a region without mass, where the density
    is the difference of two O(1) positions) has its weight held as weight x pdf == eval — the weight itself is 1 / (that difference)."""
    rgb, pdf = orc.eval_pdf(wi, wo)
    _host_close(out[:, 0:3], rgb, "eval"); _host_close(out[:, 3], pdf, "pdf")
    o_wo, o_pdf, _ = orc.sample(wi, u)
    live = out[:, 7] > 0
    assert live.mean() >= min_live and np.count_nonzero(live != (o_pdf > 0)) <= 2, (live.mean(), np.count_nonzero(live != (o_pdf > 0)))
    both = live & (o_pdf > 0)
    if both.any():
        assert float(np.abs(out[both, 4:7] - o_wo[both]).max()) < 5e-7, float(np.abs(out[both, 4:7] - o_wo[both]).max())
    if live.any():
        c_rgb, c_pdf = orc.eval_pdf(wi[live], out[live, 4:7])
        _host_close(out[live, 7], c_pdf, "sample pdf")
        sharp = c_pdf >= faint * float(c_pdf.max())
        _host_close(out[live, 8:11][sharp], c_rgb[sharp] / c_pdf[sharp, None], "sample weight")
        if not sharp.all():
            _host_close(out[live, 8:11][~sharp] * out[live, 7][~sharp, None].astype(np.float64), c_rgb[~sharp], "faint sample weight x pdf")
    return live


@pytest.mark.skipif(__import__("shutil").which("hipcc") is None, reason="hipcc missing")
@pytest.mark.parametrize("case", [dict(seed=1, n_phi=1, n_theta=6, res=12, res_ndf=16, res_sigma=8),
                                  dict(seed=2, n_phi=5, n_theta=4, res=9, res_ndf=8, res_sigma=6),
                                  dict(seed=3, n_phi=1, n_theta=1, res=2, res_ndf=2, res_sigma=2),
                                  dict(seed=4, n_phi=4, n_theta=3, res=7, res_ndf=8, res_sigma=6, reduction=2),
                                  dict(seed=5, n_phi=3, n_theta=3, res=6, res_ndf=6, res_sigma=4, reduction=4),
                                  dict(seed=6, n_phi=5, n_theta=1, res=8, res_ndf=8, res_sigma=6)],      # one elevation node: a bracket of two phi slices
                         ids=lambda c: f"phi{c['n_phi']}_theta{c['n_theta']}_res{c['res']}_red{c.get('reduction', 1)}")
def test_product_per_unit_functions_on_the_host_match_the_oracle(case, tmp_path_factory):
    """The product's RGL code — image builder (cell bricks, running integrals) and per-unit eval / pdf / sample, the SAME
    functions the kernel runs (__host__ __device__) — compiled for the host (tests/rgl_host_harness.hip) against the
    independent restatement in oracle/rgl_oracle.c.  The product uses reciprocal / rsqrt-seeded Newton steps, an atan
    polynomial and Taylor sin / cos where the oracle calls libm: 1e-6 relative."""
    from oracle.binding import OracleRgl, generate_pairs
    build = _host_harness(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("rgl_host")
    f = synth.make_rgl_fields(**case)
    n = 30000
    wi, wo, u = generate_pairs(7 + case["seed"], 0, n)
    wi[:50] = wi[50:100]; wo[:50] = wi[:50] * np.array([-1, -1, 1], np.float32)          # exact mirror pairs: m == n
    wo[100:150] = wi[100:150] * np.array([-1, -1, 1], np.float32) * np.float32(1 + 3e-7)   # ... and pairs a few ulps off
    out = _run_host(build, tmp, f, wi, wo, u)
    _host_matches_oracle(out, OracleRgl(f), wi, wo, u)


def _near_normal(wi, k, rng):
    """the first k incident directions replaced by ones within 0.07 rad of the normal (below an uneven grid's first elevation node)"""
    t = rng.uniform(0.0, 0.07, k); p = rng.uniform(-np.pi, np.pi, k)
    wi[:k] = np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], 1).astype(np.float32)
    return wi


# Files no fixed case built before: the database's shapes, rows of more than 16 cells (the column search past its four halvings from
# the row-header blocks), non-square tables (an x / y swap anywhere shows), uneven parameter grids with a first elevation node above 0,
# and distributions with regions without mass (flat running integrals: ties in the searches, zero slopes, samples of pdf 0).
HOST_SHAPES = [
    ("iso_database", dict(seed=11, n_phi=1, n_theta=8, res=32, res_ndf=128, res_sigma=32), 0.5),
    ("aniso_res20", dict(seed=12, n_phi=5, n_theta=4, res=20, res_ndf=12, res_sigma=8), 0.5),
    ("iso_33x9", dict(seed=13, n_phi=1, n_theta=5, res=(33, 9), res_ndf=(12, 7), res_sigma=(5, 9)), 0.5),
    ("iso_9x33", dict(seed=14, n_phi=1, n_theta=5, res=(9, 33), res_ndf=(7, 12), res_sigma=(9, 5)), 0.5),
    ("aniso_33x9", dict(seed=15, n_phi=4, n_theta=3, res=(33, 9), res_ndf=(6, 11), res_sigma=(10, 4)), 0.5),
    ("aniso_9x33_red2", dict(seed=16, n_phi=4, n_theta=3, res=(9, 33), res_ndf=(11, 6), res_sigma=(4, 10), reduction=2), 0.5),
    ("iso_uneven", dict(seed=17, n_phi=1, n_theta=7, res=(19, 13), grid="uneven"), 0.5),
    ("aniso_uneven", dict(seed=18, n_phi=6, n_theta=5, res=(13, 19), grid="uneven"), 0.5),
    ("iso_rows", dict(seed=19, n_phi=1, n_theta=5, res=(21, 12), sparse="rows"), 0.3),
    ("iso_cols", dict(seed=20, n_phi=1, n_theta=5, res=(21, 12), sparse="cols"), 0.3),
    ("iso_slice", dict(seed=21, n_phi=1, n_theta=5, res=(21, 12), sparse="slice"), 0.3),
    ("iso_delta_luminance", dict(seed=22, n_phi=1, n_theta=5, res=(21, 12), sparse="delta", sparse_in=("luminance",)), 0.0),
    ("iso_delta_vndf", dict(seed=23, n_phi=1, n_theta=5, res=(21, 12), sparse="delta", sparse_in=("vndf",)), 0.0),
    ("aniso_rows_uneven", dict(seed=24, n_phi=5, n_theta=4, res=(12, 21), sparse="rows", grid="uneven"), 0.3),
    ("aniso_cols", dict(seed=25, n_phi=5, n_theta=4, res=(21, 12), sparse="cols"), 0.3),
    ("aniso_slice", dict(seed=26, n_phi=5, n_theta=4, res=(21, 12), sparse="slice"), 0.3),
    ("aniso_delta", dict(seed=27, n_phi=4, n_theta=3, res=(21, 12), sparse="delta", reduction=4), 0.0),
]


@pytest.mark.skipif(__import__("shutil").which("hipcc") is None, reason="hipcc missing")
@pytest.mark.parametrize("name,case,min_live", HOST_SHAPES, ids=[c[0] for c in HOST_SHAPES])
def test_product_on_the_host_at_new_shapes(name, case, min_live, tmp_path_factory):
    """The host-compiled product against the oracle on the files of HOST_SHAPES, with the existing host tolerances; a tenth of the
    incident directions lie within 0.07 rad of the normal (below the uneven grids' first elevation node)."""
    from oracle.binding import OracleRgl, generate_pairs
    build = _host_harness(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("rgl_host_shapes")
    f = synth.make_rgl_fields(**case)
    n = 20000
    wi, wo, u = generate_pairs(0xA11 + case["seed"], 0, n)
    wi = _near_normal(wi, n // 10, np.random.default_rng(case["seed"]))
    out = _run_host(build, tmp, f, wi, wo, u)
    _host_matches_oracle(out, OracleRgl(f), wi, wo, u, min_live)


@pytest.mark.skipif(__import__("shutil").which("hipcc") is None, reason="hipcc missing")
@pytest.mark.parametrize("sparse", ["rows", "cols"])
def test_product_on_the_host_at_the_edges_of_u(sparse, tmp_path_factory):
    """A single-slice file (one node per parameter: every blend is the slice's own Float) with node rows / columns without mass: u at
    0, at the largest Float below 1, at 1, and at the exact Float values of luminance's marginal and conditional integrals — plateaus
    among them.  Both sides compare the same Float integrals in f64, so a tie is a tie on both and every search decision must agree.
    Conditional plateaus are reached in row 0 (u0 = 0: y = 0, the row total r0 and u1 r0 exact in f64), by u1 = c / r0 rounded and
    its two Float neighbours."""
    from oracle.binding import OracleRgl
    from tests import u_edges
    build = _host_harness(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("rgl_host_edges")
    f = synth.make_rgl_fields(seed=31, n_phi=1, n_theta=1, res=(19, 11), res_ndf=8, res_sigma=6, sparse=sparse)
    orc = OracleRgl(f)
    marg, cond = u_edges.rgl_luminance_integrals(orc)
    assert (np.diff(marg) == 0).any() if sparse == "rows" else (np.diff(cond[0]) == 0).any()      # plateaus to tie on
    assert (float(cond[0, -1]) > 0) == (sparse == "cols")          # (node row 0 of the "rows" file has no mass)
    u = u_edges.rgl_edge_pairs(marg, cond)
    assert (u == 1).any()
    wi, wo, u = u_edges.rgl_edge_units(u)                          # every u against incident directions from the normal to grazing
    out = _run_host(build, tmp, f, wi, wo, u)
    live = _host_matches_oracle(out, orc, wi, wo, u, 0.2, faint=1e-6)
    # and the oracle's own pdf-0 samples are the product's: a draw from a zero-mass region comes back empty on both sides
    o_wo, o_pdf, _ = orc.sample(wi, u)
    assert np.count_nonzero(live != (o_pdf > 0)) == 0


@pytest.mark.parametrize("reduction", [2, 4])
def test_symmetry_reduced_files_are_equivariant(reduction):
    """A file that stores phi_i in [-pi, 0] (reduction 2: point symmetry) or [-pi, -pi/2] (reduction 4: two mirror planes) answers for
    the whole azimuth: eval / pdf are invariant under the sample's symmetry operations and sample() is equivariant (the direction
    drawn for S wi is S applied to the direction drawn for wi) — which is what pins the map back out of the stored part."""
    B = ob.OracleRgl(synth.make_rgl_fields(6, n_phi=4, n_theta=4, res=8, reduction=reduction))
    assert B.c.reduction == reduction
    wi, wo, u = ob.generate_pairs(77, 0, 4000)
    ops = [np.array([-1, -1, 1], np.float32)] + ([np.array([-1, 1, 1], np.float32), np.array([1, -1, 1], np.float32)] if reduction == 4 else [])
    rgb, pdf = B.eval_pdf(wi, wo)
    s_wo, s_pdf, s_w = B.sample(wi, u)
    assert (pdf > 0).mean() > 0.9 and (s_pdf > 0).mean() > 0.5
    for S in ops:
        r2, p2 = B.eval_pdf(wi * S, wo * S)
        assert np.array_equal(r2, rgb) and np.array_equal(p2, pdf)
        w2, q2, v2 = B.sample(wi * S, u)
        assert np.array_equal(w2, s_wo * S) and np.array_equal(q2, s_pdf) and np.array_equal(v2, s_w)
    # and the stored part is really what is read: wi inside it is not touched
    inside = (wi[:, 1] < 0) & ((wi[:, 0] < 0) | (reduction == 2))
    B1 = ob.OracleRgl(dict(synth.make_rgl_fields(6, n_phi=4, n_theta=4, res=8, reduction=reduction)))
    assert inside.any() and np.array_equal(B1.eval_pdf(wi[inside], wo[inside])[0], rgb[inside])
    # a span that is no integer fraction of the circle is refused
    bad = synth.make_rgl_fields(6, n_phi=4, n_theta=4, res=8, reduction=2)
    bad["phi_i"] = np.linspace(-np.pi, -1.0, 4).astype(np.float32)
    with pytest.raises(AssertionError):
        ob.OracleRgl(bad)


# ------------------------------------------------------------------ spectral files ("spectra" + "wavelengths" instead of "rgb")
def test_spectral_files_interpolate_the_wavelength_as_a_third_parameter():
    """What pins the spectral restatement (no spectral file or upstream source exists offline: PARITY UNPINNED):
    at the file's own nodes the values are the per-node tables' (a spectral file whose three "wavelengths" are 0, 1, 2 IS the RGB file,
    bit for bit); between two nodes the value is their linear blend; outside the grid it is the end node's; pdf and sampled direction do
    not depend on the wavelength and equal the RGB file's; weight == value / pdf."""
    from mitsuba_customization_amd import synth
    from oracle import binding as ob
    rgbf = synth.make_rgl_fields(seed=31, n_phi=1, n_theta=4, res=7, res_ndf=6, res_sigma=5)
    spec = {k: v for k, v in rgbf.items() if k != "rgb"}
    spec["spectra"] = rgbf["rgb"].copy(); spec["wavelengths"] = np.array([0.0, 1.0, 2.0], np.float32)
    A, B = ob.OracleRgl(rgbf), ob.OracleRgl(spec)
    wi, wo, u = ob.generate_pairs(0x5EED, 31, 4000)
    rgb, pdf = A.eval_pdf(wi, wo)
    val, pdf_s = B.eval_pdf_spectral(wi, wo)                     # at the nodes
    assert np.array_equal(val, rgb) and np.array_equal(pdf_s, pdf)
    wo2, pdf2, w = A.sample(wi, u)
    s_wo2, s_pdf2, s_w = B.sample_spectral(wi, u)
    assert np.array_equal(s_wo2, wo2) and np.array_equal(s_pdf2, pdf2) and np.array_equal(s_w, w)
    # per-unit wavelengths: midpoints blend, outside clamps
    n = wi.shape[0]
    wl = np.tile(np.array([0.5, 1.25, -3.0, 7.0, 2.0], np.float32), (n, 1))
    v, p = B.eval_pdf_spectral(wi, wo, wl)
    r64 = rgb.astype(np.float64)
    assert np.array_equal(p, pdf)
    assert np.allclose(v[:, 0], 0.5 * (r64[:, 0] + r64[:, 1]), rtol=3e-7, atol=1e-30)
    assert np.allclose(v[:, 1], 0.75 * r64[:, 1] + 0.25 * r64[:, 2], rtol=3e-7, atol=1e-30)
    assert np.array_equal(v[:, 2], rgb[:, 0]) and np.array_equal(v[:, 3], rgb[:, 2]) and np.array_equal(v[:, 4], rgb[:, 2])
    s2_wo, s2_pdf, s2_w = B.sample_spectral(wi, u, wl)
    assert np.array_equal(s2_wo, wo2) and np.array_equal(s2_pdf, pdf2)
    live = s2_pdf > 0
    c_val, c_pdf = B.eval_pdf_spectral(wi[live], s2_wo[live], wl[live])
    assert np.array_equal(c_pdf, s2_pdf[live]) and np.array_equal(s2_w[live], c_val / c_pdf[:, None])


@pytest.mark.skipif(__import__("shutil").which("hipcc") is None, reason="hipcc missing")
def test_product_spectral_functions_on_the_host_match_the_oracle(tmp_path_factory):
    """The product's spectral per-unit functions and image builder compiled for the HOST (tests/rgl_host_harness.hip --spectral)
    against the oracle: values / weights to 1e-6, pdf to 1e-6, directions to an ulp."""
    import os, subprocess
    from mitsuba_customization_amd import synth
    from oracle import binding as ob
    build = _host_harness(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("spectral")
    for case in (dict(seed=41, n_phi=1, n_theta=5, res=9, res_ndf=8, res_sigma=6, n_wavelengths=7),
                 dict(seed=42, n_phi=4, n_theta=3, res=6, res_ndf=6, res_sigma=4, n_wavelengths=1),
                 dict(seed=43, n_phi=5, n_theta=2, res=5, res_ndf=6, res_sigma=4, n_wavelengths=12),
                 dict(seed=44, n_phi=1, n_theta=6, res=(23, 7), res_ndf=(9, 5), res_sigma=(4, 7), n_wavelengths=64, grid="uneven"),
                 dict(seed=45, n_phi=4, n_theta=3, res=(7, 19), res_ndf=(5, 9), res_sigma=(7, 4), n_wavelengths=66, sparse="cols")):
        f = synth.make_rgl_fields(**case)
        B = ob.OracleRgl(f)
        n, W = 3000, 4
        wi, wo, u = ob.generate_pairs(0x5EED, case["seed"], n)
        rng = np.random.default_rng(case["seed"])
        wl = rng.uniform(300.0, 1060.0, (n, W)).astype(np.float32)            # some outside the grid
        _write_fields(tmp / "fields.bin", f)
        with open(tmp / "pairs.bin", "wb") as fh:
            np.array([n], np.uint64).tofile(fh); np.array([W], np.int32).tofile(fh)
            wi.tofile(fh); wo.tofile(fh); u.tofile(fh); wl.tofile(fh)
        subprocess.check_call([str(build), "--spectral", str(tmp / "fields.bin"), str(tmp / "pairs.bin"), str(tmp / "out.bin")])
        out = np.fromfile(tmp / "out.bin", np.float32).reshape(n, 2 * W + 5)
        val, pdf, wo2, pdf2, w = out[:, :W], out[:, W], out[:, W + 1:W + 4], out[:, W + 4], out[:, W + 5:]
        o_val, o_pdf = B.eval_pdf_spectral(wi, wo, wl)
        close = lambda a, b: bool((np.abs(a.astype(np.float64) - b) <= 1e-6 * np.abs(b) + 1e-30).all())
        assert close(val, o_val) and close(pdf, o_pdf), case
        o_wo2, o_pdf2, _ = B.sample_spectral(wi, u, wl)
        live = (pdf2 > 0) & (o_pdf2 > 0)
        assert np.count_nonzero((pdf2 > 0) != (o_pdf2 > 0)) <= 1 and float(np.abs(wo2[live] - o_wo2[live]).max()) < 5e-7
        c_val, c_pdf = B.eval_pdf_spectral(wi[live], wo2[live], wl[live])
        assert close(pdf2[live], c_pdf) and close(w[live], c_val / c_pdf[:, None]), case
