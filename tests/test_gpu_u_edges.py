"""The device samplers of table, n-channel and RGL materials at the edges of u (tests/u_edges.py; tests/test_u_edges_cpu.py pins that
construction to the oracle on the CPU), with bars that hold on ties: every unit, no fractions.

  * cosine branch (u0 < alpha; all of MRL_OPT_SAMPLING 0): direction, pdf and decision bit-identical to the oracle, both disk maps;
  * lobe branch: direction within 1.2e-7 of the oracle's, decision equal to the oracle's except where the f64 restatement of the
    direction (u_edges.lobe_direction) has |z| < 1e-6 (test_u_edges_cpu.py caps the share of such units at 0.1 %; measured: none);
  * every live unit: pdf to 2e-6 and weight to 3e-6 against the oracle evaluated AT the device's direction (a unit drawn on a CDF
    value returns a half vector on a theta_h bin edge: one ulp of direction moves the pdf by a bin step there, so a comparison with
    the oracle's own draw cannot hold), the device's pdf(wi, wo') equal to sample.pdf bit for bit, rejected units exact zeros;
  * sample, eval_sample, the queue form over all slots and host arrays give the same bits; so does every unit under a permutation
    of the batch (as constructed: neighbouring lanes in different branches; sorted by u0: whole waves in one branch, whole waves
    rejected; a shuffled batch of a multiple of 64 plus 1 units).
The RGL files go against the oracle with the bars of test_rgl_cpu.py::_host_matches_oracle; their batches are tiled to 2^15 units,
the smallest launch that copies the search tables to LDS (route_rgl).  A CDF of more than 64 theta_h bins (257) is dealt out over
the incident directions (u_edges.edge_units), which keeps every batch below 20,000 units.

Measured on the MI355X (worst over every case; each test prints its own as "figures ..."), error of the lobe direction against the
oracle's draw, relative error of pdf and weight against the oracle at the returned direction:
    tables, mode 0    direction 0 (bit-identical)   pdf 0         weight 2.5e-7
    tables, mode 1    direction 8.9e-16             pdf 6.0e-8    weight 3.0e-7
    tables, mode 2    direction 2.8e-14             pdf 0         weight 3.1e-7
    n-channel 1 / 5   direction 2.2e-16             pdf 0         weight 1.7e-7
    RGL (4 files)     direction 1.2e-16             pdf and weight equal to the oracle's Floats (one faint pdf: 8.9e-6 of its value)
(a direction error below 1e-9 is between Floats of equal bits apart from a component like sin(2 pi u1) = 1e-16 against 0).
On the CPU (test_u_edges_cpu.py): restatement against the oracle's Float direction 2.98e-8 = 2^-25, no unit within 1e-6 of the
horizon, 66 - 74 % of the units live, one ulp of wo' moves the pdf beyond 2e-6 on 4.6 % (7x5x3) and 13.7 % (37x11x53) of the live
edge units and on none of 20,000 random ones.

What the set found: an exact mirror pair (wo' = (-x, -y, z) of wi, which the lobe returns for u0 == alpha: theta_h = 0) made the
tuned kernels read phi_d off the rounding residue of their fused sums, and wi == wo' == n gave phi_d = pi/8 where the oracle and the
generic kernel say 0 — weights off by whole texels on the noise tables (59 of 1,198 live units at 7x5x3, mode 1).  Fixed in
merl_table_fast.hpp::coords."""
import functools

import numpy as np
import pytest

from tests import u_edges as ue
from tests.test_gpu_sampling import at_returned_direction, at_returned_direction_2d, frac_close

pytestmark = pytest.mark.gpu

CASES = ue.TABLE_CASES
IDS = [c[0] for c in CASES]
FIGURES = {}                   # family -> [worst direction error, worst relative pdf error, worst relative weight error]


def to_dev(*arrs):
    import torch
    return [torch.from_numpy(np.array(a, copy=True)).cuda() for a in arrs]


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_np(a)).view(np.int32)


def _same(got, want, what):
    got, want = list(got), list(want)
    assert len(got) == len(want), what
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(x), _bits(y)), (what, k, int((_bits(x) != _bits(y)).reshape(_bits(x).shape[0], -1).any(axis=1).sum()))


def _record(family, direction=0.0, pdf=0.0, weight=0.0):
    f = FIGURES.setdefault(family, [0.0, 0.0, 0.0])
    f[0] = max(f[0], float(direction)); f[1] = max(f[1], float(pdf)); f[2] = max(f[2], float(weight))
    print(f"figures {family}: direction {f[0]:.3e} pdf {f[1]:.3e} weight {f[2]:.3e}")


def _rel(got, want):
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max()) if got.size else 0.0


@functools.lru_cache(maxsize=None)
def _table(case):
    from mitsuba_customization_amd import synth
    _, dims, kind, seed = case
    return synth.make_table(kind, seed, dims)


def _orders(u):
    """index arrays: sorted by u0 (whole waves in one branch, whole waves rejected), and a shuffled batch of 64 k + 1 units"""
    n = u.shape[0]
    shuffled = np.random.default_rng(n).permutation(n)[: (n - 1) // 64 * 64 + 1]
    return {"sorted by u0": np.argsort(u[:, 0], kind="stable"), "64 k + 1 shuffled": shuffled}


def _pseudo_wo(wi):
    """outgoing directions for the fused call's eval / pdf half (not under test here)"""
    return np.ascontiguousarray(np.roll(wi, 5, axis=0) * np.array([1, -1, 1], np.float32))


def _check_units(tag, family, mode, u, lobe, d, got, want, at_returned):
    """the bars of the module docstring on one batch: got / want = (wo', pdf, weight) of the device / of the oracle's own draw"""
    s_wo, s_pdf, s_w = got
    c_wo, c_pdf, c_w = want
    assert np.isfinite(s_wo).all() and np.isfinite(s_pdf).all() and np.isfinite(s_w).all(), tag
    live, c_live = s_pdf > 0, c_pdf > 0
    cos = ~lobe
    both = lobe & live & c_live
    err = np.abs(s_wo[both].astype(np.float64) - c_wo[both]).max() if both.any() else 0.0
    at = {}
    if live.any():                                        # measured before anything is asserted
        at = at_returned(None)
        _record(family, err, _rel(s_pdf[live], at["pdf"]), _rel(s_w[live], at["weight"]))
    assert np.array_equal(_bits(s_wo[cos]), _bits(c_wo[cos])), tag + ": cosine branch direction"
    assert np.array_equal(_bits(s_pdf[cos]), _bits(c_pdf[cos])), tag + ": cosine branch pdf"
    assert np.array_equal(live[cos], c_live[cos]), tag + ": cosine branch decision"
    if lobe.any():
        excused = lobe & (np.abs(d[:, 2]) < 1e-6)
        strict = lobe & ~excused
        assert np.array_equal(live[strict], c_live[strict]), (tag + ": lobe decision", int((live[strict] != c_live[strict]).sum()))
        assert np.array_equal(live[strict], d[strict, 2].astype(np.float32) > 0), tag + ": lobe decision against the restatement"
        assert err <= 1.2e-7, (tag + ": lobe direction", err)
    if mode != 0:                                         # (plain cosine sampling keeps the direction of a rim sample of pdf 0, as the oracle)
        assert not s_wo[~live].any(), tag + ": rejected units return zeros"
    assert not s_pdf[~live].any() and not s_w[~live].any(), tag + ": rejected units return zeros"
    at_returned(tag)
    return live


# ------------------------------------------------------------------ RGB tables
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_table_samplers_at_the_edges_of_u(oracle, case, mode):
    import torch
    from mitsuba_customization_amd import host
    name, dims, _, _ = case
    tab = _table(case)
    T = oracle.OracleTable(tab, ue.TABLE_SCALE)
    s, cdf, _ = T.sampling_arrays()
    family = f"table mode {mode}"
    for layout in (host.LAYOUT_ROWS, host.LAYOUT_BRICK):
        with host.MerlHip(0) as g:
            g.set_option(host.OPT_TABLE_LAYOUT, layout)
            mid = g.upload_table(tab, ue.TABLE_SCALE)
            g.set_option(host.OPT_SAMPLING, mode)
            rows = sp = None
            if mode == 2:                                 # the edge set of the rows the device built; the oracle's sampler runs on them
                rows = g.material_sampling2d(mid)
                sp = T.sampling2d(ue.N_INCIDENT_BINS, flat=rows)
            wis, wi, u, first = ue.table_edge_units(mode, cdf=cdf, rows=rows)
            n = wi.shape[0]
            assert n <= 20000
            lobe, d = ue.table_lobe_directions(mode, s, wis, wi, u, first, cdf=cdf, rows=rows) if mode else (np.zeros(n, bool), None)
            wo = _pseudo_wo(wi)
            dwi, dwo, du = to_dev(wi, wo, u)
            orders = _orders(u)
            by_variant = {}
            for disk in (0, 1):
                opts = oracle.make_opts(disk_map=disk)
                g.set_option(host.OPT_DISK_MAP, disk)
                want = T.sample(wi, u, opts) if mode == 0 else T.sample_table(wi, u, opts) if mode == 1 else T.sample_table2d(sp, wi, u, opts)
                for variant in (0, 1, 3):
                    g.set_option(host.OPT_KERNEL, variant)
                    tag = f"{name} mode {mode} layout {layout} disk {disk} variant {variant}"
                    got = [_np(t) for t in g.sample(dwi, du, material=mid)]
                    by_variant[(disk, variant)] = got

                    def at_returned(t, got=got):
                        s_wo, s_pdf, s_w = got
                        if t is None:                     # the figures alone
                            lv = s_pdf > 0
                            p = (oracle.pdf(wi[lv], s_wo[lv]) if mode == 0 else T.pdf_table(wi[lv], s_wo[lv]) if mode == 1
                                 else T.pdf_table2d(sp, wi[lv], s_wo[lv])).astype(np.float64)
                            return {"pdf": p, "weight": T.eval(wi[lv], s_wo[lv]).astype(np.float64) / p[:, None]}
                        if mode == 1:
                            at_returned_direction(T, wi, s_wo, s_pdf, s_w, t)
                        elif mode == 2:
                            at_returned_direction_2d(T, sp, wi, s_wo, s_pdf, s_w, t)
                        else:
                            lv = s_pdf > 0
                            c_pdf = oracle.pdf(wi[lv], s_wo[lv]).astype(np.float64)
                            assert frac_close(s_pdf[lv], c_pdf, 2e-6) == 1.0, t + ": pdf at the returned direction"
                            assert frac_close(s_w[lv], T.eval(wi[lv], s_wo[lv]).astype(np.float64) / c_pdf[:, None], 3e-6) == 1.0, t + ": weight"

                    live = _check_units(tag, family, mode, u, lobe, d, got, want, at_returned)
                    assert live.mean() > 0.5, tag
                    # the device's own pdf(wi, wo') is what sample() reported
                    back = _np(g.pdf(*to_dev(wi[live], got[0][live]), material=mid))
                    assert np.array_equal(_bits(back), _bits(got[1][live])), tag + ": pdf(wi, wo') == sample.pdf"
                    # entry points
                    fused = g.eval_sample(dwi, dwo, du, material=mid)
                    _same(fused[2:], got, tag + ": eval_sample")
                    _same(g.sample(wi, u, material=mid), got, tag + ": host arrays")
                    _same(g.eval_sample(wi, wo, u, material=mid), fused, tag + ": host arrays, fused")
                    # unit order
                    for what, idx in orders.items():
                        di = torch.from_numpy(idx).cuda()
                        _same(g.sample(dwi[di].contiguous(), du[di].contiguous(), material=mid), [a[idx] for a in got], f"{tag}: {what}")
                # queues do not follow MRL_OPT_KERNEL: bricks (trilinear) take k_table_dma — the bits of variant 3 —, rows the generic kernel
                ref_variant = 3 if layout == host.LAYOUT_BRICK else 0
                g.set_option(host.OPT_KERNEL, 3 - ref_variant)
                queue = torch.from_numpy(np.random.default_rng(7).permutation(n).astype(np.int32)).cuda()
                count = torch.tensor([n], dtype=torch.int32, device="cuda")
                _same(g.sample_queue(dwi, du, queue, count, material=mid), by_variant[(disk, ref_variant)], f"{name} mode {mode} layout {layout} disk {disk}: queue")


@pytest.mark.parametrize("mode", [1, 2])
def test_mixed_batch_of_tables_and_ggx_on_their_own_edge_sets(oracle, mode):
    """Two tables and a GGX conductor in one batch with material ids under MRL_OPT_KERNEL 4 (partitioned by kind first), each unit on
    its own material's edge set, shuffled: the bits of the single-material calls"""
    import torch
    from mitsuba_customization_amd import host
    from tests import ggx_reference as gr
    with host.MerlHip(0) as g:
        g.set_option(host.OPT_KERNEL, 4)
        g.set_option(host.OPT_SAMPLING, mode)
        parts = []
        for case in CASES[:2]:
            tab = _table(case)
            mid = g.upload_table(tab, ue.TABLE_SCALE)
            cdf = oracle.OracleTable(tab, ue.TABLE_SCALE).sampling_arrays()[1]
            rows = g.material_sampling2d(mid) if mode == 2 else None
            _, wi, u, _ = ue.table_edge_units(mode, cdf=cdf, rows=rows)
            parts.append((mid, wi, u))
        ggx = g.ggx(0.2, (1.5, 1.5, 1.5), (3.0, 3.0, 3.0))
        wis = ue.incident_directions()
        ug = np.array(gr.U_EDGES, np.float32)
        parts.append((ggx, np.repeat(wis, ug.shape[0], axis=0), np.tile(ug, (wis.shape[0], 1))))
        wi = np.concatenate([p[1] for p in parts]); u = np.concatenate([p[2] for p in parts])
        mat = np.concatenate([np.full(p[1].shape[0], p[0], np.int32) for p in parts])
        perm = np.random.default_rng(mode).permutation(wi.shape[0])
        wi, u, mat = wi[perm], u[perm], mat[perm]
        wo = _pseudo_wo(wi)
        dwi, dwo, du, dmat = to_dev(wi, wo, u, mat)
        for disk in (0, 1):
            g.set_option(host.OPT_DISK_MAP, disk)
            mixed = [t.clone() for t in g.sample(dwi, du, mat=dmat)]
            fused = [t.clone() for t in g.eval_sample(dwi, dwo, du, mat=dmat)]
            _same(fused[2:], mixed, "fused")
            assert all(bool(torch.isfinite(t).all()) for t in mixed)
            for mid, _, _ in parts:
                sel = torch.from_numpy(np.nonzero(mat == mid)[0]).cuda()
                single = g.sample(dwi[sel].contiguous(), du[sel].contiguous(), material=mid)
                assert float(single[1].max()) > 0
                _same([t[sel] for t in mixed], single, ("mode", mode, "disk", disk, "material", mid))


# ------------------------------------------------------------------ n-channel tables
@pytest.mark.parametrize("n_ch", [1, 5])
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_nch_samplers_at_the_edges_of_u(oracle, case, n_ch):
    """k_table_nch (1 channel) and k_table_nch_wide (5) against eval_sample_nch(..., table_sampling=True); an n-channel table has no
    conditional table: MRL_OPT_SAMPLING 2 answers with the marginal (alpha = 1/2), and is held to the same bars"""
    import torch
    from mitsuba_customization_amd import host, synth
    name, dims, kind, seed = case
    tab = synth.make_table_nch("noise" if kind == "noise" else "spectral", n_ch, seed, dims)
    scale = [0.5 + 0.25 * c for c in range(n_ch)]
    O = oracle.OracleTableNch(tab, scale)
    sp = O.sampling()
    s = np.ctypeslib.as_array(sp.s, (sp.n + 1,)).copy(); cdf = np.ctypeslib.as_array(sp.cdf, (sp.n + 1,)).copy()
    wis, wi, u, first = ue.table_edge_units(1, cdf=cdf)
    lobe, d = ue.table_lobe_directions(1, s, wis, wi, u, first, cdf=cdf)
    n = wi.shape[0]
    wo = _pseudo_wo(wi)
    dwi, dwo, du = to_dev(wi, wo, u)
    orders = _orders(u)
    with host.MerlHip(0) as g:
        mid = g.upload_table_nch(tab, scale)
        for disk in (0, 1):
            opts = oracle.make_opts(disk_map=disk)
            g.set_option(host.OPT_DISK_MAP, disk)
            want = oracle.eval_sample_nch([O], wi, wo, u, None, opts, table_sampling=True)
            for mode in (1, 2):
                g.set_option(host.OPT_SAMPLING, mode)
                tag = f"{name} n_ch {n_ch} disk {disk} mode {mode}"
                got = [_np(t) for t in g.sample_nch(dwi, du, n_ch, material=mid)]

                def at_returned(t, got=got):
                    s_wo, s_pdf, s_w = got
                    lv = s_pdf > 0
                    back = oracle.eval_sample_nch([O], wi[lv], s_wo[lv], u[lv], None, opts, table_sampling=True)
                    c_pdf = back[1].astype(np.float64)
                    c_w = back[0].astype(np.float64) / c_pdf[:, None]
                    if t is None:
                        return {"pdf": c_pdf, "weight": c_w}
                    assert frac_close(s_pdf[lv], c_pdf, 2e-6) == 1.0, t + ": pdf at the returned direction"
                    assert frac_close(s_w[lv], c_w, 3e-6) == 1.0, t + ": weight at the returned direction"

                live = _check_units(tag, f"n-channel ({n_ch})", mode, u, lobe, d, got, want[2:], at_returned)
                assert live.mean() > 0.5, tag
                back = _np(g.pdf(*to_dev(wi[live], got[0][live]), material=mid))
                assert np.array_equal(_bits(back), _bits(got[1][live])), tag + ": pdf(wi, wo') == sample.pdf"
                fused = g.eval_sample_nch(dwi, dwo, du, n_ch, material=mid)
                _same(fused[2:], got, tag + ": eval_sample_nch")
                _same(g.sample_nch(wi, u, n_ch, material=mid), got, tag + ": host arrays")
                for what, idx in orders.items():
                    di = torch.from_numpy(idx).cuda()
                    _same(g.sample_nch(dwi[di].contiguous(), du[di].contiguous(), n_ch, material=mid), [a[idx] for a in got], f"{tag}: {what}")
                queue = torch.from_numpy(np.random.default_rng(11).permutation(n).astype(np.int32)).cuda()
                count = torch.tensor([n], dtype=torch.int32, device="cuda")
                _same(g.sample_queue_nch(dwi, du, queue, count, n_ch, material=mid), got, tag + ": queue")
                _same(g.eval_sample_queue_nch(dwi, dwo, du, queue, count, n_ch, material=mid), fused, tag + ": fused queue")


# ------------------------------------------------------------------ RGL
LDS_BATCH = 1 << 15            # the smallest launch that copies the search tables to LDS


def _tiled(n_unique, *arrs):
    reps = -(-LDS_BATCH // n_unique)
    return [np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))) for a in arrs]


def _both_searches(g, call, what):
    """call() with the search tables in LDS (MRL_OPT_RGL_SEARCH 0) and in memory (1): the same bits; returns the LDS results as numpy"""
    from mitsuba_customization_amd import host
    assert g.get_option(host.OPT_RGL_SEARCH) == 0
    lds = [_np(t).copy() for t in call()]
    g.set_option(host.OPT_RGL_SEARCH, 1)
    try:
        _same(call(), lds, what + ": memory search")
    finally:
        g.set_option(host.OPT_RGL_SEARCH, 0)
    return lds


@pytest.mark.parametrize("sparse", ["rows", "cols"])
def test_rgl_single_slice_files_at_the_edges_of_u(sparse):
    """The two single-slice files of test_rgl_cpu.py::test_product_on_the_host_at_the_edges_of_u (node rows / columns without mass:
    plateaus in the integrals) with that test's u set less the entries equal to 1, through sample and eval_sample"""
    from mitsuba_customization_amd import host, synth
    from oracle.binding import OracleRgl
    from tests.test_rgl_cpu import _host_matches_oracle
    f = synth.make_rgl_fields(seed=31, n_phi=1, n_theta=1, res=(19, 11), res_ndf=8, res_sigma=6, sparse=sparse)
    orc = OracleRgl(f)
    marg, cond = ue.rgl_luminance_integrals(orc)
    wi, wo, u = ue.rgl_edge_units(ue.rgl_edge_pairs(marg, cond, device=True))
    k = wi.shape[0]
    assert k == {"rows": 1656, "cols": 3288}[sparse] and (u < 1).all()
    twi, two, tu = _tiled(k, wi, wo, u)
    dwi, dwo, du = to_dev(twi, two, tu)
    with host.MerlHip(0) as g:
        mid = g.upload_rgl(f)
        fused = _both_searches(g, lambda: g.eval_sample(dwi, dwo, du, material=mid), "eval_sample")
        alone = _both_searches(g, lambda: g.sample(dwi, du, material=mid), "sample")
        small = [_np(t) for t in g.eval_sample(*to_dev(wi, wo, u), material=mid)]           # below 2^15 units: k_rgl
    _same(alone, fused[2:], "sample == eval_sample")
    for a in fused:                                                                       # every copy of a unit: the same bits
        _same([a[j * k:(j + 1) * k] for j in range(1, a.shape[0] // k)], [a[:k]] * (a.shape[0] // k - 1), "tiles")
    _same([a[:k] for a in fused], small, "small batch")
    out = np.concatenate([fused[0][:k], fused[1][:k, None], fused[2][:k], fused[3][:k, None], fused[4][:k]], axis=1)
    assert np.isfinite(out).all()
    o_wo, o_pdf, _ = orc.sample(wi, u)
    lv = (out[:, 7] > 0) & (o_pdf > 0)
    c_rgb, c_pdf = orc.eval_pdf(wi[out[:, 7] > 0], out[out[:, 7] > 0, 4:7])
    sharp = c_pdf >= 1e-6 * float(c_pdf.max())
    _record(f"RGL single slice ({sparse})", np.abs(out[lv, 4:7] - o_wo[lv]).max(), _rel(out[out[:, 7] > 0, 7], c_pdf),
            _rel(out[out[:, 7] > 0, 8:11][sharp], c_rgb[sharp] / c_pdf[sharp, None]))
    _host_matches_oracle(out, orc, wi, wo, u, 0.2, faint=1e-6)


@pytest.mark.parametrize("name,case", [("marg_only_6x5x40x40", dict(seed=71, n_phi=6, n_theta=5, res=40, res_ndf=16, res_sigma=8)),
                                       ("spectral_5", dict(seed=72, n_phi=1, n_theta=5, res=(21, 12), res_ndf=8, res_sigma=6, n_wavelengths=5))],
                         ids=["marg_only_6x5x40x40", "spectral_5"])
def test_rgl_multi_slice_files_on_their_own_integrals(name, case):
    """The same construction with the marginal / conditional values of the file's own luminance integrals (its first and last slice)
    on the file of test_gpu_rgl.py::test_marginal_rows_in_lds_... (sample: k_rgl_lds<.., MARG_ONLY>) and on a spectral file: LDS and
    memory search agree bit for bit, the oracle is checked at the returned direction (1e-6, as test_gpu_rgl.py)"""
    import torch
    from mitsuba_customization_amd import host, synth
    from oracle.binding import OracleRgl
    from tests.test_gpu_rgl import _close
    f = synth.make_rgl_fields(**case)
    orc = OracleRgl(f)
    n_slices = orc.c.luminance.n_slices
    pairs = np.unique(np.concatenate([ue.rgl_edge_pairs(*ue.rgl_luminance_integrals(orc, j), device=True) for j in (0, n_slices - 1)]), axis=0)
    wi, wo, u = ue.rgl_edge_units(pairs, seed=case["seed"], k=6)
    k = wi.shape[0]
    assert k <= 20000
    twi, two, tu = _tiled(k, wi, wo, u)
    dwi, dwo, du = to_dev(twi, two, tu)
    spectral = "n_wavelengths" in case
    with host.MerlHip(0) as g:
        mid = g.upload_rgl(f)
        if spectral:
            wl = np.tile(f["wavelengths"].astype(np.float32), (twi.shape[0], 1))
            dwl = torch.from_numpy(wl).cuda()
            fused = _both_searches(g, lambda: g.eval_sample_spectral(dwi, dwo, du, dwl, mid), "eval_sample_spectral")
            alone = _both_searches(g, lambda: g.sample_spectral(dwi, du, dwl, mid), "sample_spectral")
        else:
            fused = _both_searches(g, lambda: g.eval_sample(dwi, dwo, du, material=mid), "eval_sample")
            alone = _both_searches(g, lambda: g.sample(dwi, du, material=mid), "sample")
    _same(alone, fused[2:], "sample == eval_sample")
    wo2, pdf2, w = (a[:k] for a in alone)
    assert np.isfinite(wo2).all() and np.isfinite(pdf2).all() and np.isfinite(w).all()
    o_wo2, o_pdf2, _ = orc.sample_spectral(wi, u, wl[:k]) if spectral else orc.sample(wi, u)
    live = pdf2 > 0
    both = live & (o_pdf2 > 0)
    c_val, c_pdf = orc.eval_pdf_spectral(wi[live], wo2[live], wl[:k][live]) if spectral else orc.eval_pdf(wi[live], wo2[live])
    sharp = c_pdf >= 1e-6 * float(c_pdf.max())
    _record(f"RGL {name}", np.abs(wo2[both] - o_wo2[both]).max(), _rel(pdf2[live], c_pdf), _rel(w[live][sharp], c_val[sharp] / c_pdf[sharp, None]))
    assert live.mean() >= 0.2 and np.count_nonzero(live != (o_pdf2 > 0)) <= 2, (live.mean(), np.count_nonzero(live != (o_pdf2 > 0)))
    assert float(np.abs(wo2[both] - o_wo2[both]).max()) < 5e-7
    assert not wo2[~live].any() and not w[~live].any()
    excuse = {} if spectral else dict(orc=orc, wi=wi[live][sharp], wo=wo2[live][sharp], max_ill=2)      # near-mirror pairs, as test_gpu_rgl.py
    _close(pdf2[live][sharp], c_pdf[sharp], "sample pdf", **excuse)
    _close(pdf2[live][~sharp], c_pdf[~sharp], "faint sample pdf")
    _close(w[live][sharp], c_val[sharp] / c_pdf[sharp, None], "weight" if not spectral else "sample weight", **excuse)
    _close(w[live][~sharp] * pdf2[live][~sharp, None].astype(np.float64), c_val[~sharp], "faint sample weight x pdf")
