"""The RGL kernels against the model's one known answer: the files of tests/rgl_ggx_reference.py — an analytic GGX conductor tabulated
in the RGL file format, isotropic, anisotropic over the whole, a half and a quarter of the azimuth, on uneven parameter grids, and
spectral — uploaded with upload_rgl and held against the conductor's closed-form eval, pdf and weights on the same fixed direction
sets and at the SAME bars as the oracle in tests/test_rgl_ggx_cpu.py (1.5 x the discretisation error measured there on the CPU
oracle; imported, not re-measured here: the code under test sets no bar of its own).  No unit is left out.

On the alpha = 0.5 isotropic file the truth is also met through the other routes to the same kernels' code: 2^15 units (route_rgl
copies the search tables to LDS from 2^15 units on: k_rgl_lds), OPT_RGL_SEARCH = 1 (the tables read from memory), the file's id in a
batch that also carries a GGX material and a MERL table, and eval_sample_queue; and its eval agrees with the device's own analytic
ctx.ggx(0.5, eta, k) material — two kernels of this library that describe one material — within the same bar.  Bit-identity between
these routes is tested in test_gpu_rgl.py and not repeated.

Measured on the device (MI355X), median / p99 of |value - truth| / (truth + 1e-3 max truth); every figure equals the oracle's in
tests/test_rgl_ggx_cpu.py to the four digits printed (device and oracle differ by 1e-6, the discretisation error is 1e-3):

  case              eval                 pdf                  sample pdf           weight               fixed wi: mean, spread
  iso_a0.3          1.543e-3 1.335e-2    1.659e-3 1.740e-2    2.186e-3 2.770e-2    2.957e-3 2.652e-2    2.467e-3 7.911e-3
  iso_a0.5          5.200e-4 5.604e-3    2.082e-3 1.511e-2    2.137e-3 2.257e-2    2.134e-3 1.800e-2    1.379e-3 6.893e-3
  iso_a0.5_coarse   2.221e-3 2.485e-2    9.105e-3 6.142e-2    9.459e-3 1.002e-1    9.713e-3 8.636e-2    5.324e-3 2.398e-2
  iso_a0.5_uneven   5.649e-4 5.668e-3    2.009e-3 1.481e-2    2.155e-3 2.143e-2    2.145e-3 1.772e-2    1.044e-3 6.886e-3
  aniso_full        3.287e-3 6.405e-2    8.458e-3 9.101e-2    6.231e-3 5.036e-2    5.849e-3 4.606e-2    5.540e-3 1.491e-2
  aniso_red2        3.375e-3 5.629e-2    8.552e-3 8.659e-2    6.513e-3 5.072e-2    5.971e-3 4.499e-2    5.540e-3 1.491e-2
  aniso_red4        3.148e-3 3.664e-2    8.472e-3 6.449e-2    6.591e-3 5.581e-2    5.784e-3 4.840e-2    5.540e-3 1.491e-2
  aniso_uneven      3.395e-3 5.181e-2    8.840e-3 7.807e-2    6.612e-3 5.522e-2    5.882e-3 4.803e-2    5.985e-3 1.416e-2
  spectral          8.192e-4 8.210e-3    1.553e-3 1.346e-2    1.980e-3 2.365e-2    2.337e-3 2.059e-2    1.766e-3 7.310e-3

iso_a0.5 against the analytic material: 5.200e-4 / 5.604e-3; through k_rgl_lds (the set tiled 8 x to 2^15 units) 5.200e-4 / 5.614e-3,
with OPT_RGL_SEARCH = 1, in the mixed batch and through the queue 5.200e-4 / 5.604e-3.  Median eval error per quadrant of wi
(+ +, - +, - -, + -): full 3.36e-3 3.05e-3 3.12e-3 3.67e-3, reduction 2 3.29e-3 3.47e-3 3.12e-3 3.67e-3, reduction 4 3.29e-3 3.05e-3
3.12e-3 3.14e-3.
"""
import numpy as np
import pytest

from tests import rgl_ggx_reference as R
from tests import test_rgl_ggx_cpu as cpu

pytestmark = pytest.mark.gpu

RGB_CASES = [c for c in cpu.TESTED if c != "spectral"]


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]          # a copy: the case's arrays are read-only


def _np(tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("case", RGB_CASES)
def test_kernels_reproduce_the_conductor(oracle, case):
    """eval, pdf, eval_pdf and sample of every RGB file against the truth, and the weights at three fixed wi against the albedo"""
    from mitsuba_customization_amd import host
    fields, g = R.case_file(case)
    wi, wo, u = R.case_units(oracle, case)
    fwi, fu = R.fixed_wi_units(oracle)
    with host.MerlHip(0) as gpu:
        mid = gpu.upload_rgl(fields)
        wi_t, wo_t, u_t, fwi_t, fu_t = _cuda(wi, wo, u, fwi, fu)
        rgb, = _np([gpu.eval(wi_t, wo_t, material=mid)])
        pdf, = _np([gpu.pdf(wi_t, wo_t, material=mid)])
        wo2, pdf2, weight = _np(gpu.sample(wi_t, u_t, material=mid))
        fused = _np(gpu.eval_pdf(wi_t, wo_t, material=mid))
        _, f_pdf2, f_weight = _np(gpu.sample(fwi_t, fu_t, material=mid))
    cpu.assert_within(R.measure(g, wi, wo, rgb, pdf, wo2, pdf2, weight), cpu.bars(case), case)
    cpu.assert_within(R.measure(g, wi, wo, fused[0], fused[1], wo2, pdf2, weight), cpu.bars(case), case + " eval_pdf")
    cpu.assert_within({"fixed_wi": R.measure_fixed_wi(g, fwi, f_pdf2, f_weight)}, {"fixed_wi": cpu.fixed_bars(case)}, case)


@pytest.mark.parametrize("case", ["aniso_full", "aniso_red2", "aniso_red4"])
def test_reduced_files_in_every_quadrant(oracle, case):
    """the sign flips into and out of the stored part of the azimuth: every quadrant of wi meets the full file's truth"""
    from mitsuba_customization_amd import host
    fields, g = R.case_file(case)
    wi, wo, u = R.case_units(oracle, case)
    qwi, qu = R.quadrant_units(oracle)
    with host.MerlHip(0) as gpu:
        mid = gpu.upload_rgl(fields)
        wi_t, wo_t, qwi_t, qu_t = _cuda(wi, wo, qwi, qu)
        rgb, = _np([gpu.eval(wi_t, wo_t, material=mid)])
        wo2, pdf2, _ = _np(gpu.sample(qwi_t, qu_t, material=mid))
    truth = g.eval_truth(wi, wo)
    err = (np.abs(rgb - truth) / (truth + 1e-3 * truth.max())).reshape(len(wi), -1)
    med = []
    for sx, sy in cpu.QUADRANTS:
        q = (np.signbit(wi[:, 0]) == (sx < 0)) & (np.signbit(wi[:, 1]) == (sy < 0))
        med.append(float(np.median(err[q])))
    print(case, "median eval error per quadrant of wi:", " ".join(f"{m:.3e}" for m in med))
    assert max(med) <= cpu.bars(case)["eval"][0] and max(med) <= 2.0 * min(med)
    R.assert_lobes_face_wi(qwi, wo2, pdf2)


def test_the_analytic_ggx_material_and_every_route(oracle, tables):
    """the alpha = 0.5 isotropic file: against the device's analytic GGX material, then the truth through k_rgl_lds (2^15 units),
    OPT_RGL_SEARCH = 1, a mixed batch with the GGX material and a MERL table, and a wavefront queue"""
    import torch
    from mitsuba_customization_amd import host
    case = "iso_a0.5"
    fields, g = R.case_file(case)
    wi, wo, u = R.case_units(oracle, case)
    n = len(wi)
    bar = cpu.bars(case)
    with host.MerlHip(0) as gpu:
        mid = gpu.upload_rgl(fields)
        ggx = gpu.ggx(0.5, *R.GOLD)
        merl = gpu.upload_merl(tables("ggx_tab", 0))
        wi_t, wo_t, u_t = _cuda(wi, wo, u)
        # two kernels, one material (the analytic material samples visible normals without the luminance warp: its pdf and weights
        # are another sampler's, only eval is common)
        rgb, = _np([gpu.eval(wi_t, wo_t, material=mid)])
        analytic, = _np([gpu.eval(wi_t, wo_t, material=ggx)])
        assert float(np.abs(analytic / g.eval_truth(wi, wo) - 1.0).max()) < 2e-6
        cpu.assert_within({"eval": R.med_p99(rgb, analytic)}, bar, "rgl against the analytic material")
        # 2^15 units: the search tables in LDS
        assert n * 8 == 1 << 15
        big = [t.repeat(8, 1) for t in (wi_t, wo_t, u_t)]
        out = _np(gpu.eval_sample(*big, material=mid))
        cpu.assert_within(R.measure(g, np.tile(wi, (8, 1)), np.tile(wo, (8, 1)), *out), bar, "2^15 units")
        # the search tables from memory
        gpu.set_option(host.OPT_RGL_SEARCH, 1)
        out = _np(gpu.eval_sample(wi_t, wo_t, u_t, material=mid))
        gpu.set_option(host.OPT_RGL_SEARCH, 0)
        cpu.assert_within(R.measure(g, wi, wo, *out), bar, "OPT_RGL_SEARCH = 1")
        # the file's id on every unit of the set, the GGX material and the MERL table on 512 more
        extra = 512
        mat = torch.cat([torch.full((n,), mid, dtype=torch.int32), torch.tensor([ggx, merl], dtype=torch.int32).repeat(extra // 2)]).cuda()
        mixed = [torch.cat([t, t[:extra]]) for t in (wi_t, wo_t, u_t)]
        out = _np(gpu.eval_sample(*mixed, mat=mat))
        cpu.assert_within(R.measure(g, wi, wo, *[o[:n] for o in out]), bar, "mixed batch")
        on_ggx = np.arange(n, n + extra, 2)
        assert float(np.abs(out[0][on_ggx] / g.eval_truth(wi[0:extra:2], wo[0:extra:2]) - 1.0).max()) < 2e-6
        assert float(out[0][on_ggx + 1].max()) > 0.0
        # a wavefront queue over every unit
        queue = torch.arange(n, device="cuda", dtype=torch.int32)
        count = torch.tensor([n], device="cuda", dtype=torch.int32)
        out = _np(gpu.eval_sample_queue(wi_t, wo_t, u_t, queue, count, material=mid))
        cpu.assert_within(R.measure(g, wi, wo, *out), bar, "queue")


def test_spectral_file(oracle):
    """eval_spectral / sample_spectral at W = 4 per-unit wavelengths: on nodes, between them and outside the grid"""
    from mitsuba_customization_amd import host
    case = "spectral"
    fields, g = R.case_file(case)
    wi, wo, u = R.case_units(oracle, case)
    wl = R.case_wavelengths(case, len(wi))
    fwi, fu = R.fixed_wi_units(oracle)
    with host.MerlHip(0) as gpu:
        mid = gpu.upload_rgl(fields)
        wi_t, wo_t, u_t, wl_t, fwi_t, fu_t = _cuda(wi, wo, u, wl, fwi, fu)
        values, pdf = _np(gpu.eval_spectral(wi_t, wo_t, wl_t, mid, with_pdf=True))
        alone, = _np([gpu.eval_spectral(wi_t, wo_t, wl_t, mid)])
        wo2, pdf2, weight = _np(gpu.sample_spectral(wi_t, u_t, wl_t, mid))
        _, f_pdf2, f_weight = _np(gpu.sample_spectral(fwi_t, fu_t, None, mid, n_wavelengths=len(g.wavelengths)))
    cpu.assert_within(R.measure(g, wi, wo, values, pdf, wo2, pdf2, weight, wl), cpu.bars(case), case)
    cpu.assert_within({"eval": R.med_p99(alone, g.eval_truth(wi, wo, wl))}, cpu.bars(case), case + " eval alone")
    cpu.assert_within({"fixed_wi": R.measure_fixed_wi(g, fwi, f_pdf2, f_weight)}, {"fixed_wi": cpu.fixed_bars(case)}, case)
    # linear in the wavelength and clamped outside the grid: exact up to Float rounding
    for v, keep in ((values.astype(np.float64), slice(None)), (weight.astype(np.float64), pdf2 > 0)):
        v, w = v[keep], wl[keep]
        assert float((v[:, 0] > 0).mean()) == 1.0
        assert float(np.abs(v / v[:, :1] / (g.colour_at(w) / g.colour_at(w[:, :1])) - 1.0).max()) < 1e-6
