"""The RGL kernels at the database's shapes and on files the other RGL tests never build: non-square tables, uneven parameter grids,
distributions with regions without mass, an isotropic file on either side of the LDS fit boundary, 2^24-unit batches.  Every case
goes against oracle/rgl_oracle.c (4,096 strided units and the batch's last 257) and holds the bit-identity invariants between entry
points and kernels.  Which kernels a case reaches is route_rgl (csrc/merl_kernels.hpp, exported as mrl_rgl_route); its rules are
restated and checked without a device in tests/test_rgl_route_cpu.py, on these shapes among others."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_rgl import _close

pytestmark = pytest.mark.gpu

SMALL = 1 << 15          # the smallest batch that takes the LDS kernels
BIG = 1 << 24            # tools/rgl_rates.py's batch


def lds_limit():
    """LDS per workgroup, read the way the library's lds_limit() does: hipDeviceGetAttribute(MaxSharedMemoryPerBlock) on the current
    device, through the HIP runtime torch has loaded"""
    import torch
    torch.cuda.init()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line)
    hip = C.CDLL(path)
    dev, v = C.c_int(), C.c_int()
    assert hip.hipGetDevice(C.byref(dev)) == 0
    assert hip.hipDeviceGetAttribute(C.byref(v), 74, dev) == 0     # hipDeviceAttributeMaxSharedMemoryPerBlock (hip_runtime_api.h)
    assert 64 << 10 <= v.value <= 1 << 20
    return v.value


def lds_bytes_of(n_phi, n_theta, nx, ny, n_wl=0):
    """Python mirror of lds_bytes_of() (csrc/merl_rgl.hip): the parameter grids, then per distribution (vndf, luminance) the slice-major
    conditional integrals (float2 per cell), row totals (float2 per cell row) and marginal (float per cell row), each 16-B aligned"""
    a16 = lambda b: (b + 15) // 16 * 16
    slices, per_c, per_r = n_phi * n_theta, (nx - 1) * (ny - 1), ny - 1
    return a16((n_phi + n_theta + n_wl) * 4) + 2 * (a16(slices * per_c * 8) + a16(slices * per_r * 8) + a16(slices * per_r * 4))


def fit_boundary(limit, n_theta=8, ny=32):
    """(nx that just fits, nx that just does not) for an isotropic n_theta x nx x ny file"""
    nx = 2
    while lds_bytes_of(1, n_theta, nx + 1, ny) <= limit:
        nx += 1
    assert lds_bytes_of(1, n_theta, nx, ny) <= limit < lds_bytes_of(1, n_theta, nx + 1, ny)
    return nx, nx + 1


ISO_DB = dict(seed=9, n_phi=1, n_theta=8, res=32, res_ndf=128, res_sigma=32)
ANISO_DB = dict(seed=10, n_phi=16, n_theta=8, res=32, res_ndf=128, res_sigma=32)

# name, file (res "fit" / "nofit": the nx of fit_boundary x ny 32), kernels reached at n = 2^15 with MRL_OPT_RGL_SEARCH = 0
# (every case also runs at MRL_OPT_RGL_SEARCH = 1 and as a batch of 4,353 units: k_rgl<M, ., false, mask>)
CASES = [
    ("iso_database", ISO_DB, "k_rgl_lds<M, ., false, 5> (1,024 / 768 threads)"),
    ("iso_just_fits", dict(seed=21, n_phi=1, n_theta=8, res="fit", res_ndf=32, res_sigma=16), "k_rgl_lds<M, ., false, 5>"),
    ("iso_just_does_not_fit", dict(seed=22, n_phi=1, n_theta=8, res="nofit", res_ndf=32, res_sigma=16),
     "k_rgl<M, ., false, 5>; sample: k_rgl_lds<2, ., true, 0>; fused: k_rgl<4, ., false, 5> + k_rgl_lds<2, ., true, 0>"),
    ("aniso_database", ANISO_DB, "k_rgl<M, ., false, 15>; sample: k_rgl_lds<2, ., true, 15>; fused: k_rgl<4, ., false, 15> + k_rgl_lds<2, ., true, 15>"),
    ("iso_33x9_uneven_rows", dict(seed=23, n_phi=1, n_theta=5, res=(33, 9), res_ndf=(12, 7), res_sigma=(5, 9), grid="uneven", sparse="rows"),
     "k_rgl_lds<M, ., false, 5>"),
    ("iso_9x33_cols", dict(seed=24, n_phi=1, n_theta=5, res=(9, 33), res_ndf=(7, 12), res_sigma=(9, 5), sparse="cols"), "k_rgl_lds<M, ., false, 5>"),
    ("iso_delta_luminance", dict(seed=25, n_phi=1, n_theta=4, res=(21, 12), sparse="delta", sparse_in=("luminance",)), "k_rgl_lds<M, ., false, 5>"),
    ("aniso_13x19_uneven_slice", dict(seed=26, n_phi=6, n_theta=5, res=(13, 19), grid="uneven", sparse="slice"),
     "k_rgl_lds<M, ., false, 0> (an anisotropic file that fits: the kernel that tests the shape at run time)"),
    ("aniso_21x12_cols_red2", dict(seed=27, n_phi=4, n_theta=3, res=(21, 12), sparse="cols", reduction=2), "k_rgl_lds<M, ., false, 0>"),
    ("phi_only_19x7", dict(seed=28, n_phi=5, n_theta=1, res=(19, 7), grid="uneven"), "k_rgl_lds<M, ., false, 0>"),
    ("iso_database_uneven_rows", dict(seed=29, n_phi=1, n_theta=8, res=32, res_ndf=128, res_sigma=32, grid="uneven", sparse="rows"),
     "k_rgl_lds<M, ., false, 5>"),
    ("iso_database_40x24_cols", dict(seed=30, n_phi=1, n_theta=8, res=(40, 24), res_ndf=(128, 96), res_sigma=(32, 48), sparse="cols"),
     "k_rgl_lds<M, ., false, 5>"),
    ("aniso_database_uneven_rows", dict(ANISO_DB, seed=31, grid="uneven", sparse="rows"),
     "k_rgl<M, ., false, 15>; sample: k_rgl_lds<2, ., true, 15>; fused split"),
]


def _fields(case):
    from mitsuba_customization_amd import synth
    case = dict(case)
    if case.get("res") in ("fit", "nofit"):
        case["res"] = (fit_boundary(lds_limit())[0 if case["res"] == "fit" else 1], 32)
    return synth.make_rgl_fields(**case)


def _oracle_units(n, k=4096, tail=257):
    """k strided units and the batch's last `tail`"""
    return np.unique(np.concatenate([np.arange(k) * (n // k), np.arange(n - tail, n)]))


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.int32)


def _same(got, want, what):
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(x), _bits(y)), (what, k)


def _match_oracle(orc, wi, wo, u, out):
    """eval / pdf within 1e-6 relative (at most 2 near-mirror units excused per quantity); the sampled direction within 5e-7 absolute, its
    pdf and weight against the oracle evaluated AT the device's direction"""
    rgb, pdf, wo2, pdf2, w = out
    o_rgb, o_pdf = orc.eval_pdf(wi, wo)
    assert float(o_pdf.max()) > 0
    _close(rgb, o_rgb, "eval", orc, wi, wo, max_ill=2); _close(pdf, o_pdf, "pdf", orc, wi, wo, max_ill=2)
    o_wo2, o_pdf2, _ = orc.sample(wi, u)
    live = pdf2 > 0
    assert np.count_nonzero(live != (o_pdf2 > 0)) <= 2
    both = live & (o_pdf2 > 0)
    assert both.any() and float(np.abs(wo2[both] - o_wo2[both]).max()) < 5e-7
    c_rgb, c_pdf = orc.eval_pdf(wi[live], wo2[live])
    _close(pdf2[live], c_pdf, "sample pdf", orc, wi[live], wo2[live], max_ill=2)
    _close(w[live], c_rgb / c_pdf[:, None], "weight", orc, wi[live], wo2[live], max_ill=2)


def _check_material(g, orc, mid, n, seed):
    """one material at n units: separate entry points == fused, LDS == memory search, queue == whole array, the oracle's units re-issued
    as one small batch == the same units of the big one; the oracle on those units"""
    import torch
    from mitsuba_customization_amd import host
    wi, wo, u = g.generate_pairs(seed, 0, n)
    fused = [t.clone() for t in g.eval_sample(wi, wo, u, material=mid)]
    _same((g.eval(wi, wo, material=mid), g.pdf(wi, wo, material=mid)), fused[:2], "eval, pdf")
    _same(g.eval_pdf(wi, wo, material=mid), fused[:2], "eval_pdf")
    _same(g.sample(wi, u, material=mid), fused[2:], "sample")
    q = torch.arange(1, n, 3, device=wi.device, dtype=torch.int32)
    cnt = torch.tensor([q.numel()], device=wi.device, dtype=torch.int32)
    ql = q.long()
    _same([t[ql] for t in g.eval_sample_queue(wi, wo, u, q, cnt, material=mid)], [t[ql] for t in fused], "eval_sample queue")
    _same([t[ql] for t in g.sample_queue(wi, u, q, cnt, material=mid)], [t[ql] for t in fused[2:]], "sample queue")
    _same([t[ql] for t in g.eval_pdf_queue(wi, wo, q, cnt, material=mid)], [t[ql] for t in fused[:2]], "eval_pdf queue")
    assert g.get_option(host.OPT_RGL_SEARCH) == 0
    g.set_option(host.OPT_RGL_SEARCH, 1)
    try:
        _same(g.eval_sample(wi, wo, u, material=mid), fused, "memory search: eval_sample")
        _same(g.sample(wi, u, material=mid), fused[2:], "memory search: sample")
        _same(g.eval_pdf(wi, wo, material=mid), fused[:2], "memory search: eval_pdf")
    finally:
        g.set_option(host.OPT_RGL_SEARCH, 0)
    sel = _oracle_units(n)
    st = torch.from_numpy(sel).to(wi.device)
    swi, swo, su = wi[st].contiguous(), wo[st].contiguous(), u[st].contiguous()
    small = g.eval_sample(swi, swo, su, material=mid)              # < 2^15 units: k_rgl
    _same(small, [t[st] for t in fused], "small batch of the same units")
    _match_oracle(orc, swi.cpu().numpy(), swo.cpu().numpy(), su.cpu().numpy(), [t[st].cpu().numpy() for t in fused])



def test_lds_boundary_mirror_matches_the_database_shape():
    """The mirror of lds_bytes_of at the database's isotropic shape (129,008 B: fits) and the anisotropic one (does not); the fit pair
    straddles the device's limit"""
    limit = lds_limit()
    assert lds_bytes_of(1, 8, 32, 32) == 129008 <= limit < lds_bytes_of(16, 8, 32, 32)
    fit, nofit = fit_boundary(limit)
    assert fit < nofit and lds_bytes_of(1, 8, fit, 32) <= limit < lds_bytes_of(1, 8, nofit, 32)


@pytest.mark.parametrize("name,case,kernels", CASES, ids=[c[0] for c in CASES])
def test_rgl_shapes_match_the_oracle_and_agree_between_paths(name, case, kernels):
    from mitsuba_customization_amd import host
    from oracle.binding import OracleRgl
    fields = _fields(case)
    orc = OracleRgl(fields)
    with host.MerlHip(0) as g:
        mid = g.upload_rgl(fields)
        _check_material(g, orc, mid, SMALL, 0x5A0 + case["seed"])


@pytest.mark.parametrize("name,case", [("iso_database", ISO_DB), ("aniso_database", ANISO_DB)], ids=["iso_database", "aniso_database"])
def test_database_files_at_the_rates_batch(name, case):
    """2^24 units (the rates' batch) of the two database-shaped files: the strided units and the tail against the oracle, the same units
    re-issued as one batch below 2^15 (k_rgl) with the same bits, the separate entry points, the queue and the memory search with the fused
    call's bits"""
    from mitsuba_customization_amd import host
    from oracle.binding import OracleRgl
    fields = _fields(case)
    orc = OracleRgl(fields)
    with host.MerlHip(0) as g:
        mid = g.upload_rgl(fields)
        _check_material(g, orc, mid, BIG, 0xB16 + case["seed"])


@pytest.mark.parametrize("W", [1, 16])
def test_spectral_database_shape(W):
    """A spectral file of the isotropic database shape with 64 unevenly spaced wavelength nodes, W wavelengths per unit:
    k_rgl_spectral<M, true, 5> (LDS) and, at MRL_OPT_RGL_SEARCH = 1, k_rgl_spectral<M, false, 5> — the same bits, the separate spectral
    entry points the fused call's bits, the oracle on 4,096 strided units and the tail"""
    import torch
    from mitsuba_customization_amd import host, synth
    from oracle.binding import OracleRgl
    fields = synth.make_rgl_fields(seed=33, n_phi=1, n_theta=8, res=32, res_ndf=128, res_sigma=32, n_wavelengths=64)
    assert lds_bytes_of(1, 8, 32, 32, 64) <= lds_limit()
    orc = OracleRgl(fields)
    n = SMALL
    with host.MerlHip(0) as g:
        mid = g.upload_rgl(fields)
        wi, wo, u = g.generate_pairs(0x5B0 + W, 0, n)
        lo, hi = float(fields["wavelengths"][0]), float(fields["wavelengths"][-1])
        wl = np.random.default_rng(W).uniform(lo - 20.0, hi + 20.0, (n, W)).astype(np.float32)
        wl[:97, 0] = fields["wavelengths"][np.arange(97) % 64]                              # on the nodes
        wl_t = torch.from_numpy(wl).cuda()
        fused = [t.clone() for t in g.eval_sample_spectral(wi, wo, u, wl_t, mid)]
        _same(g.eval_spectral(wi, wo, wl_t, mid, with_pdf=True), fused[:2], "eval_pdf_spectral")
        _same((g.eval_spectral(wi, wo, wl_t, mid),), fused[:1], "eval_spectral")
        _same(g.sample_spectral(wi, u, wl_t, mid), fused[2:], "sample_spectral")
        g.set_option(host.OPT_RGL_SEARCH, 1)
        try:
            _same(g.eval_sample_spectral(wi, wo, u, wl_t, mid), fused, "memory search")
            _same(g.sample_spectral(wi, u, wl_t, mid), fused[2:], "memory search: sample")
        finally:
            g.set_option(host.OPT_RGL_SEARCH, 0)
    sel = _oracle_units(n)
    hwi, hwo, hu, hwl = wi.cpu().numpy()[sel], wo.cpu().numpy()[sel], u.cpu().numpy()[sel], wl[sel]
    val, pdf, wo2, pdf2, w = (t.cpu().numpy()[sel] for t in fused)
    o_val, o_pdf = orc.eval_pdf_spectral(hwi, hwo, hwl)
    _close(val, o_val, "values"); _close(pdf, o_pdf, "pdf")                                 # (random pairs: no exemption, as test_gpu_rgl_spectral.py)
    o_wo2, o_pdf2, _ = orc.sample_spectral(hwi, hu, hwl)
    live = pdf2 > 0
    assert live.mean() > 0.5 and np.count_nonzero(live != (o_pdf2 > 0)) <= 2
    both = live & (o_pdf2 > 0)
    assert float(np.abs(wo2[both] - o_wo2[both]).max()) < 5e-7
    c_val, c_pdf = orc.eval_pdf_spectral(hwi[live], wo2[live], hwl[live])
    _close(pdf2[live], c_pdf, "sample pdf"); _close(w[live], c_val / c_pdf[:, None], "sample weight")


def test_batch_with_ids_of_the_database_files_a_merl_table_and_ggx():
    """A batch with material ids over both database-shaped files, a MERL table and GGX: k_rgl<M, ., true, 0> for the RGL units — every
    mode, every unit the bits of its material's own call (which for these files is k_rgl_lds / k_rgl<M, ., false, 15> / the split)"""
    import torch
    from mitsuba_customization_amd import host, synth
    n = SMALL
    with host.MerlHip(0) as g:
        iso = g.upload_rgl(_fields(ISO_DB))
        aniso = g.upload_rgl(_fields(ANISO_DB))
        tab = g.upload_merl(synth.make_table("ggx_tab", 0))
        ggx = g.ggx(0.2, (1.5, 1.5, 1.5), (3.0, 3.0, 3.0))
        ids = torch.tensor([iso, tab, aniso, ggx], device="cuda", dtype=torch.int32)
        mat = ids[torch.arange(n, device="cuda") % 4]
        wi, wo, u = g.generate_pairs(0x1D5, 0, n)
        for call in (lambda **kw: (g.eval(wi, wo, **kw),), lambda **kw: (g.pdf(wi, wo, **kw),), lambda **kw: g.sample(wi, u, **kw),
                     lambda **kw: g.eval_pdf(wi, wo, **kw), lambda **kw: g.eval_sample(wi, wo, u, **kw)):
            mixed = [t.clone() for t in call(mat=mat)]
            for slot, k in enumerate(ids.tolist()):
                _same([t[slot::4] for t in mixed], [t[slot::4] for t in call(material=int(k))], ("ids", k))
