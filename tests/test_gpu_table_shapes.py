"""customized_measurement tables of free dimensions (mrl_material_upload_table, mrl_material_upload_table_nch) through every table
kernel, sampler and entry point, at shapes the other table tests never build: single-cell axes, no power of two, more theta_h bins
than k_sampling2d_scan has threads.  Everything is compared with oracle/merl_oracle.c on generate_pairs units plus units aimed at the
first and last cell of every axis (_targeted), and every entry point with the fused call bit for bit.  Which kernels a case reaches
follows route_batch (csrc/merl_kernels.hpp; tests/test_route_cpu.py checks it on the CPU), launch_build_sampling2d
(csrc/merl_kernels.hip) and launch_nch_cpad (csrc/merl_nch.hip):
  * MRL_OPT_KERNEL 0 .. 4 and queues: k_batch, k_table, k_table_dma (byte offsets in 32 bits: every case here is below 2^25 cells);
    a batch with material ids under variant 4 first partitions the units by kind (k_count_kinds, k_partition_kinds);
  * upload: k_build_bricks or k_build_rows, then k_sampling2d_mass<LAYOUT> + k_sampling2d_scan (the conditional table).
    n_th = 257, 512 and 777 give each of the scan's 256 threads 2, 2 and 4 (ragged: 777 = 256 * 3 + 9) theta_h bins;
  * the image cache: save converts bricks to rows (k_bricks_to_rows), load converts rows to bricks (k_rows_to_bricks);
  * the one-unit path: the host image of the table (mrl_material_host_table) and the scalar service;
  * n-channel tables: k_build_bricks_nch, then k_table_nch<., ., C, .> for C = 1, 2 and k_table_nch_wide for 5, 16, 32 channels.
Bars are those of test_gpu_parity.py, test_gpu_sampling.py and test_gpu_nch.py.  On the noise tables a unit with theta_h or theta_d
below 0.02 rad is ill-conditioned for the oracle (test_gpu_parity.py::test_adversarial_directions_match_oracle): its trilinear value
must lie inside the oracle's rounding range, and it is left out of the nearest and node-centred comparisons and of the n-channel
values."""
import functools

import numpy as np
import pytest

from tests import np_restatement as npr
from tests.test_gpu_parity import _conditioning_range
from tests.test_gpu_sampling import at_returned_direction, at_returned_direction_2d, frac_close

pytestmark = pytest.mark.gpu

REL = 1e-6
SCALE = (0.5, 2.0, 1.25)
LOOKUPS = ((1, 0), (1, 1), (0, 0))                 # (lookup, node): trilinear on integer nodes, on cell centres, nearest
VARIANTS = (0, 1, 2, 3, 4)

# name, (n_th, n_td, n_pd), synth.make_table kind, seed.  The thin and odd shapes carry noise: a GGX-shaped table with one theta_d
# texel holds only theta_d = 0, where phi_d does not matter.
CASES = [
    ("unit", (1, 1, 1), "noise", 1),
    ("thin_1x7x1", (1, 7, 1), "noise", 2),
    ("thin_5x1x2", (5, 1, 2), "noise", 3),
    ("thin_2x3x1", (2, 3, 1), "noise", 4),
    ("odd_7x5x3", (7, 5, 3), "noise", 5),
    ("odd_37x11x53", (37, 11, 53), "ggx_tab", 6),
    ("merl", (90, 90, 180), "ggx_tab", 7),
    ("scan_257x4x6", (257, 4, 6), "noise", 8),
    ("scan_512x3x5", (512, 3, 5), "ggx_tab", 9),
    ("scan_777x6x4", (777, 6, 4), "noise", 10),
]
IDS = [c[0] for c in CASES]
N_RANDOM = 4096
PER_GROUP = 48


def to_dev(*arrs):
    import torch
    return [torch.from_numpy(np.array(a, copy=True)).cuda() for a in arrs]


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_np(a)).view(np.int32)


def _same(got, want, what):
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(x), _bits(y)), (what, k)


@functools.lru_cache(maxsize=None)
def _table(case):
    from mitsuba_customization_amd import synth
    _, dims, kind, seed = case
    return synth.make_table(kind, seed, dims)


# ------------------------------------------------------------------ units aimed at the ends of every axis
def _from_angles(th, ph, td, pd):
    """(wi, wo) with half vector at (theta_h, phi_h) and difference vector at (theta_d, phi_d): the inverse of orc_half_diff"""
    dx, dy, dz = np.sin(td) * np.cos(pd), np.sin(td) * np.sin(pd), np.cos(td)
    x, y, z = dx * np.cos(th) + dz * np.sin(th), dy, -dx * np.sin(th) + dz * np.cos(th)
    wi = np.stack([x * np.cos(ph) - y * np.sin(ph), x * np.sin(ph) + y * np.cos(ph), z], 1)
    h = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    wo = 2.0 * np.sum(wi * h, axis=1, keepdims=True) * h - wi
    return wi, wo


def _angles(wi, wo):
    """the device's cancellation-free theta_h, theta_d of the f32 pairs"""
    a = wi.astype(np.float64); b = wo.astype(np.float64)
    a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
    s, e = a + b, a - b
    return np.arctan2(np.hypot(s[:, 0], s[:, 1]), s[:, 2]), np.arctan2(np.linalg.norm(e, axis=1), np.linalg.norm(s, axis=1))


def _targeted(T, dims, rng):
    """PER_GROUP pairs in the first and in the last cell of each axis: the last theta_h row (half vector within a few mrad of the
    horizon, phi_d near pi/2 so that both directions stay above it), theta_d near pi/2, and either side of the phi_d seam.  Each
    group is checked to land in its cell as the oracle indexes it.  Returns wi, wo (f32) and {group: slice}"""
    from oracle import binding as ob
    n_th, n_td, n_pd = dims
    k = PER_GROUP
    f = lambda: rng.uniform(0.2, 0.8, k)                                       # where inside the cell
    ph = lambda: rng.uniform(0.0, 2 * np.pi, k)
    th_of = lambda x: (x / n_th) ** 2 * (np.pi / 2)
    td_of = lambda x: x / n_td * (np.pi / 2)
    mid = lambda lo, hi: rng.uniform(lo, hi, k)

    def above(th, td):          # phi_d keeping both directions above the horizon: |tan td cos pd| < cot th, with a factor 2 to spare
        c = np.minimum(0.5 / (np.tan(th) * np.tan(td) + 1e-300), 1.0)
        return np.pi / 2 + np.arcsin(c * rng.uniform(-1, 1, k))

    groups = {}
    th = th_of(f()); td = mid(0.1, 1.2); groups["theta_h first"] = (th, td, above(th, td), 0, 0)
    th = th_of(n_th - 1 + f()); td = mid(0.2, 1.2); groups["theta_h last"] = (th, td, above(th, td), 0, n_th - 1)
    td = td_of(f()); th = mid(0.1, 0.6); groups["theta_d first"] = (th, td, above(th, td), 1, 0)
    td = td_of(n_td - 1 + f()); th = mid(0.05, 0.4); groups["theta_d last"] = (th, td, above(th, td), 1, n_td - 1)
    pd = f() / n_pd * np.pi; groups["phi_d first"] = (mid(0.1, 0.5), mid(0.1, 0.5), pd, 2, 0)
    pd = (n_pd - 1 + f()) / n_pd * np.pi - np.pi * (rng.random(k) < 0.5)      # below pi, or below 0 (folded by reciprocity)
    groups["phi_d last"] = (mid(0.1, 0.5), mid(0.1, 0.5), pd, 2, n_pd - 1)
    wi_p, wo_p, where, at = [], [], {}, 0
    for name, (th, td, pd, axis, cell) in groups.items():
        wi, wo = _from_angles(th, ph(), td, pd)
        wi, wo = wi.astype(np.float32), wo.astype(np.float32)
        assert (wi[:, 2] > 0).all() and (wo[:, 2] > 0).all(), name
        a = wi.astype(np.float64); b = wo.astype(np.float64)
        a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
        x = np.array([T.coords(*np.array(ob.half_diff(a[i], b[i]))[[0, 2, 3]]) for i in range(k)])
        landed = np.minimum(np.floor(x[:, axis]), dims[axis] - 1) == cell
        assert landed.sum() == k, (name, int(landed.sum()))                    # every unit of the group is in its cell
        wi_p.append(wi); wo_p.append(wo); where[name] = slice(at, at + k); at += k
    return np.concatenate(wi_p), np.concatenate(wo_p), where


@functools.lru_cache(maxsize=None)
def _units(case):
    """N_RANDOM generate_pairs units, then the targeted ones (their u from the generator as well); read-only arrays"""
    from oracle import binding as ob
    _, dims, _, seed = case
    wi, wo, u = ob.generate_pairs(0x5EED, seed << 20, N_RANDOM + 6 * PER_GROUP)
    twi, two, where = _targeted(ob.OracleTable(_table(case), SCALE), dims, np.random.default_rng(seed))
    wi[N_RANDOM:], wo[N_RANDOM:] = twi, two
    wi[7, 2] = -wi[7, 2]; wo[11, 2] = -wo[11, 2]                                # below-horizon guards
    for a in (wi, wo, u):
        a.flags.writeable = False
    return wi, wo, u, {k: slice(s.start + N_RANDOM, s.stop + N_RANDOM) for k, s in where.items()}


def _ill(case, wi, wo):
    th, td = _angles(wi, wo)
    return np.zeros(wi.shape[0], bool) if case[2] != "noise" else (th <= 0.02) | (td <= 0.02)


def _check_eval(case, T, wi, wo, got, want, lookup, node, tag):
    """rgb against the oracle: 1e-6 relative; nearest: at most one bin-edge flip; ill-conditioned noise units (trilinear, integer
    nodes) inside the oracle's rounding range"""
    ill = _ill(case, wi, wo)
    ok = np.abs(got.astype(np.float64) - want) <= REL * np.abs(want) + 1e-30
    if lookup == 1:
        assert ok[~ill].all(), (tag, int((~ok[~ill]).sum()))
    else:
        assert (~ok[~ill].all(axis=1)).sum() <= 1, tag
    if ill.any() and (lookup, node) == (1, 0):
        a = wi[ill].astype(np.float64); b = wo[ill].astype(np.float64)
        a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
        th, td = _angles(wi[ill], wo[ill])
        lo, hi = _conditioning_range(T, a, b, wo[ill, 2].astype(np.float64), th, td)
        g = got[ill].astype(np.float64)
        assert ((g >= lo * (1 - 1e-6) - 1e-30) & (g <= hi * (1 + 1e-6) + 1e-30)).all(), tag + ": ill-conditioned"


# ------------------------------------------------------------------ 1. parity: variants, layouts, lookups; entry points
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_table_shape_matches_oracle_in_every_variant_layout_and_lookup(oracle, case):
    from mitsuba_customization_amd import host
    name, dims, _, seed = case
    tab = _table(case)
    T = oracle.OracleTable(tab, SCALE)
    wi, wo, u, where = _units(case)
    dwi, dwo, du = to_dev(wi, wo, u)
    want = {lk: oracle.eval_sample_multi([T], wi, wo, u, None, oracle.make_opts(lookup=lk[0], node=lk[1])) for lk in LOOKUPS}
    results = {}
    for layout in (host.LAYOUT_ROWS, host.LAYOUT_BRICK):
        with host.MerlHip(0) as g:
            g.set_option(host.OPT_TABLE_LAYOUT, layout)
            mid = g.upload_table(tab, SCALE)
            assert g.material_info(mid) == (host.KIND_TABLE, dims)
            for lookup, node in LOOKUPS:
                g.set_option(host.OPT_LOOKUP, lookup); g.set_option(host.OPT_NODE, node)
                w = want[(lookup, node)]
                for variant in VARIANTS:
                    g.set_option(host.OPT_KERNEL, variant)
                    tag = f"{name} layout {layout} lookup {lookup} node {node} variant {variant}"
                    fused = [_np(t) for t in g.eval_sample(dwi, dwo, du, material=mid)]
                    _check_eval(case, T, wi, wo, fused[0], w[0], lookup, node, tag + " rgb")
                    assert np.array_equal(fused[1], w[1]) and np.array_equal(fused[2], w[2]) and np.array_equal(fused[3], w[3]), tag
                    ok = np.abs(fused[4].astype(np.float64) - w[4]) <= REL * np.abs(w[4]) + 1e-30
                    if lookup == 1:
                        assert ok.all(), (tag + " weight", int((~ok).sum()))
                    else:
                        assert (~ok.all(axis=1)).sum() <= 1, tag + " weight"
                    # every entry point gives the fused call's bits; host arrays the device arrays' bits
                    _same((g.eval(dwi, dwo, material=mid), g.pdf(dwi, dwo, material=mid)), fused[:2], tag + " eval, pdf")
                    _same(g.eval_pdf(dwi, dwo, material=mid), fused[:2], tag + " eval_pdf")
                    _same(g.sample(dwi, du, material=mid), fused[2:], tag + " sample")
                    _same(g.eval_sample(wi, wo, u, material=mid), fused, tag + " host arrays")
                    results[(layout, lookup, node, variant)] = fused[0]
    base = results[(host.LAYOUT_ROWS, 1, 0, 1)]
    for key, r in results.items():
        if key[1:3] == (1, 0):
            if key[3] >= 1:                                   # tuned variants: the same bits in both layouts
                assert np.array_equal(r, base), (name, key)
            else:
                ok = np.abs(r.astype(np.float64) - base) <= 5e-7 * np.abs(base.astype(np.float64)) + 1e-30
                assert ok.all(), (name, key)
    # the targeted groups really reach the kernels: some of each is non-zero
    for group, s in where.items():
        assert (base[s] > 0).any(), (name, group)


# ------------------------------------------------------------------ 2. table sampling: the marginal (1) and the conditional table (2)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_table_shape_samplers_match_oracle(oracle, case):
    from mitsuba_customization_amd import host
    name, dims, _, seed = case
    n_th = dims[0]
    tab = _table(case)
    T = oracle.OracleTable(tab, SCALE)
    wi, wo, u, _ = _units(case)
    dwi, dwo, du = to_dev(wi, wo, u)
    own = T.sampling2d_arrays(T.sampling2d(32))
    # The oracle takes theta_h as acos(h_z): in the first bins of a table with many theta_h bins (777: theta_h < 2.6e-6 rad) that
    # carries ~1e-4 of relative error, which on the noise table moves the bin's mass by up to 1.8e-5.  np_restatement's atan2 angles
    # do not.  So the densities go against the restatement everywhere, and against the oracle wherever the two references agree to
    # 1e-6; the bins where they do not must lie in the ill-conditioned corner (theta_h < 0.02 rad), at most 2 of them.
    ref = npr.sampling2d_reference(tab, SCALE)
    assert np.abs(own[:, :n_th + 1] - ref[:, :n_th + 1]).max() <= 1e-12
    own_off = (np.abs(own[:, n_th + 1:] - ref[:, n_th + 1:]) > 1e-6 * ref[:, n_th + 1:]).any(axis=0)
    th_hi = ((np.arange(n_th) + 1) / n_th) ** 2 * (np.pi / 2)
    assert own_off.sum() <= 2 and (th_hi[own_off] < 0.02).all(), np.nonzero(own_off)
    for layout in (host.LAYOUT_ROWS, host.LAYOUT_BRICK):
        with host.MerlHip(0) as g:
            g.set_option(host.OPT_TABLE_LAYOUT, layout)
            mid = g.upload_table(tab, SCALE)
            dev = g.material_sampling2d(mid)
            tag = f"{name} layout {layout}"
            assert dev.shape == own.shape == (32, 2 * n_th + 1), tag
            assert (dev[:, 0] == 0).all() and (dev[:, n_th] == 1).all(), tag
            assert (np.diff(dev[:, :n_th + 1], axis=1) > 0).all(), tag + ": cdf not strictly increasing"
            assert np.abs(dev[:, :n_th + 1] - own[:, :n_th + 1]).max() <= 2e-6, tag + ": cdf rows"
            assert np.abs(dev[:, :n_th + 1] - ref[:, :n_th + 1]).max() <= 2e-6, tag + ": cdf rows (restatement)"
            assert (np.abs(dev[:, n_th + 1:] - ref[:, n_th + 1:]) <= 2e-6 * ref[:, n_th + 1:]).all(), tag + ": densities (restatement)"
            ok = np.abs(dev[:, n_th + 1:] - own[:, n_th + 1:]) <= 2e-6 * own[:, n_th + 1:]
            assert ok[:, ~own_off].all(), tag + ": densities"
            sp = T.sampling2d(32, flat=dev)                    # the oracle's sampler on the device's table
            for disk in (0, 1):
                opts = oracle.make_opts(disk_map=disk)
                g.set_option(host.OPT_DISK_MAP, disk)
                for mode in (host.SAMPLING_TABLE, host.SAMPLING_TABLE_2D):
                    g.set_option(host.OPT_SAMPLING, mode)
                    if mode == host.SAMPLING_TABLE:
                        c_wo, c_pdf, c_w = T.sample_table(wi, u, opts)
                        c_pdf_q = T.pdf_table(wi, wo)
                        cos_branch = u[:, 0] < 0.5
                    else:
                        c_wo, c_pdf, c_w = T.sample_table2d(sp, wi, u, opts)
                        c_pdf_q = T.pdf_table2d(sp, wi, wo)
                        cos_branch = u[:, 0] < 0.125
                    for variant in (0, 1, 3):
                        g.set_option(host.OPT_KERNEL, variant)
                        t = f"{tag} disk {disk} sampling {mode} variant {variant}"
                        s_wo, s_pdf, s_w = [_np(x) for x in g.sample(dwi, du, material=mid)]
                        assert np.array_equal(s_wo[cos_branch], c_wo[cos_branch]), t + ": cosine branch"
                        assert np.abs(s_wo.astype(np.float64) - c_wo).max() <= 1.2e-7, t
                        assert np.array_equal(s_pdf > 0, c_pdf > 0), t + ": accept/reject decisions differ"
                        assert frac_close(s_pdf, c_pdf, 2e-6) > 0.9999, t
                        assert frac_close(s_w, c_w, 3e-6) > 0.9995, t
                        if mode == host.SAMPLING_TABLE:
                            at_returned_direction(T, wi, s_wo, s_pdf, s_w, t)
                        else:
                            at_returned_direction_2d(T, sp, wi, s_wo, s_pdf, s_w, t)
                        q = _np(g.pdf(dwi, dwo, material=mid))
                        assert frac_close(q, c_pdf_q, 2e-6) == 1.0, t + ": pdf"
                        f = g.eval_sample(dwi, dwo, du, material=mid)
                        _same(f[1:], (q, s_wo, s_pdf, s_w), t + ": fused")


# ------------------------------------------------------------------ 3. queues, the image cache, the one-unit path
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_table_shape_queues_image_cache_and_one_unit_path(oracle, case, tmp_path):
    import torch
    from mitsuba_customization_amd import host
    name, dims, _, seed = case
    tab = _table(case)
    T = oracle.OracleTable(tab, SCALE)
    wi, wo, u, where = _units(case)
    dwi, dwo, du = to_dev(wi, wo, u)
    n = wi.shape[0]
    perm = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)).to(torch.int32)
    k = n // 2 + 13
    queue = perm[: n - 100].contiguous()                                   # capacity n - 100, k of them live
    count = torch.tensor([k], dtype=torch.int32, device="cuda")
    live = torch.zeros(n, dtype=torch.bool, device="cuda")
    live[queue[:k].long()] = True
    sentinel = -7.0
    for layout in (host.LAYOUT_ROWS, host.LAYOUT_BRICK):
        path = str(tmp_path / f"{name}_{layout}.mrlimg")
        want = {}
        with host.MerlHip(0) as g:
            g.set_option(host.OPT_TABLE_LAYOUT, layout)
            mid = g.upload_table(tab, SCALE)
            for lookup, node in LOOKUPS:
                g.set_option(host.OPT_LOOKUP, lookup); g.set_option(host.OPT_NODE, node)
                # queues do not follow MRL_OPT_KERNEL: bricks with trilinear lookups take k_table_dma (the whole-array bits of variants
                # 1 to 4), the rest the generic kernel (variant 0's bits; test_gpu_queue.py::test_rows_layout_and_nearest_lookup_take_the_
                # generic_queue_kernel).  The option is set to the other variant for the queue calls.
                ref_variant = 3 if (layout, lookup) == (host.LAYOUT_BRICK, 1) else 0
                g.set_option(host.OPT_KERNEL, ref_variant)
                tag = f"{name} layout {layout} lookup {lookup} node {node} variant {ref_variant}"
                whole = g.eval_sample(dwi, dwo, du, material=mid)
                g.set_option(host.OPT_KERNEL, 3 - ref_variant)
                outs = tuple(torch.full_like(t, sentinel) for t in whole)
                g.eval_sample_queue(dwi, dwo, du, queue, count, material=mid, out=outs)
                for got, ref in zip(outs, whole):
                    assert torch.equal(got[live].view(torch.int32), ref[live].view(torch.int32)), tag
                    assert bool((got[~live] == sentinel).all()), tag + ": an unqueued slot was written"
                lv = live.nonzero().flatten()
                _same([t[lv] for t in g.eval_pdf_queue(dwi, dwo, queue, count, material=mid)], [t[lv] for t in whole[:2]], tag + " eval_pdf queue")
                _same([t[lv] for t in g.sample_queue(dwi, du, queue, count, material=mid)], [t[lv] for t in whole[2:]], tag + " sample queue")
                _same([g.eval_queue(dwi, dwo, queue, count, material=mid)[lv], g.pdf_queue(dwi, dwo, queue, count, material=mid)[lv]],
                      [t[lv] for t in whole[:2]], tag + " eval, pdf queue")
            g.set_option(host.OPT_LOOKUP, 1); g.set_option(host.OPT_NODE, 0); g.set_option(host.OPT_KERNEL, 3)
            for s in (0, 1, 2):
                g.set_option(host.OPT_SAMPLING, s)
                want[s] = [_np(t) for t in g.eval_sample(dwi, dwo, du, material=mid)]
            # the one-unit paths under the conditional sampler: the host image and the scalar service (bar of
            # test_gpu_sampling.py::test_conditional_table_build_and_sampler_match_oracle), random and targeted units
            f = want[2]
            picks = [0, 1, 2, 100] + [s.start for s in where.values()]
            with g.host_table(mid) as ht:
                assert ht.info()["sampling"] == 2 and ht.info()["dims"] == dims
                for i in picks:
                    got = ht.eval_sample(wi[i], wo[i], u[i])
                    ref = np.concatenate([f[0][i], [f[1][i]], f[2][i], [f[3][i]], f[4][i]])
                    assert np.allclose(got, ref, rtol=2e-7, atol=0), (name, layout, i)
                    assert np.array_equal(got, g.scalar_eval_sample(wi[i], wo[i], u[i], material=mid)) or np.allclose(got, ref, rtol=2e-7), (name, i)
            g.save_image(mid, path)
        # the image cache: rows on disk whatever the layout; loaded into a context of the same layout it answers with the same bits
        with host.MerlHip(0) as g:
            g.set_option(host.OPT_TABLE_LAYOUT, layout)
            mid = g.load_image(path)
            assert g.material_info(mid) == (host.KIND_TABLE, dims)
            for s in (0, 1, 2):
                g.set_option(host.OPT_SAMPLING, s)
                _same(g.eval_sample(dwi, dwo, du, material=mid), want[s], f"{name} layout {layout} image, sampling {s}")


# ------------------------------------------------------------------ 4. one batch with material ids over every shape
def test_id_batch_over_every_shape_a_merl_table_and_ggx(oracle):
    """All case tables, a MERL table and a GGX material in one batch with ids (the ids repeat in a fixed pattern): under variants 3
    (k_table_dma<M, true, ...>) and 4 (partitioned by kind first) every unit has the bits of its material's own call, and
    partition_by_material followed by one queue call per material gives the batch's bits"""
    import torch
    from mitsuba_customization_amd import host, synth
    n = (1 << 16) + 77
    with host.MerlHip(0) as g:
        ids = [g.upload_table(_table(c), SCALE) for c in CASES]
        ids.append(g.upload_merl(synth.make_table("ggx_tab", 11)))
        ids.append(g.ggx(0.2, (1.5, 1.5, 1.5), (3.0, 3.0, 3.0)))
        k = len(ids)
        wi, wo, u = g.generate_pairs(0x1D5, 0, n)
        mat = torch.tensor(ids, device="cuda", dtype=torch.int32)[(torch.arange(n, device="cuda") * 7) % k].contiguous()
        for variant in (3, 4):
            g.set_option(host.OPT_KERNEL, variant)
            mixed = [t.clone() for t in g.eval_sample(wi, wo, u, mat=mat)]
            for m in ids:
                sel = (mat == m).nonzero().flatten()
                single = g.eval_sample(wi[sel].contiguous(), wo[sel].contiguous(), u[sel].contiguous(), material=m)
                _same([t[sel] for t in mixed], single, ("variant", variant, "material", m))
            queue, offsets, counts = g.partition_by_material(mat)
            off = offsets.cpu().tolist()
            got = tuple(torch.full_like(t, -3.0) for t in mixed)
            for m in ids:
                g.eval_sample_queue(wi, wo, u, queue[off[m]:off[m + 1]], counts[m:m + 1], material=m, out=got)
            _same(got, mixed, ("variant", variant, "partitioned queues"))


# ------------------------------------------------------------------ 5. n-channel tables at the same shapes
@pytest.mark.parametrize("n_ch", [1, 2, 5, 16, 32])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_nch_table_shape_matches_oracle(oracle, case, n_ch):
    """k_table_nch (1, 2 channels) and k_table_nch_wide (5, 16, 32) against OracleTableNch, queue calls against the whole-array
    calls; an n-channel table has no conditional table, so MRL_OPT_SAMPLING 2 gives the bits of 1"""
    import torch
    from mitsuba_customization_amd import host, synth
    name, dims, _, seed = case
    tab = synth.make_table_nch("noise" if case[2] == "noise" else "spectral", n_ch, seed, dims)
    scale = [0.5 + 0.25 * c for c in range(n_ch)]
    wi, wo, u, _ = _units(case)
    ill = np.zeros(wi.shape[0], bool) if case[2] != "noise" else (lambda th, td: (th <= 0.02) | (td <= 0.02))(*_angles(wi, wo))
    dwi, dwo, du = to_dev(wi, wo, u)
    O = oracle.OracleTableNch(tab, scale)
    with host.MerlHip(0) as g:
        mid = g.upload_table_nch(tab, scale)
        assert g.material_channels(mid) == n_ch and g.material_info(mid) == (host.KIND_TABLE_NCH, dims)
        for lookup, node in LOOKUPS:
            g.set_option(host.OPT_LOOKUP, lookup); g.set_option(host.OPT_NODE, node)
            tag = f"{name} n_ch {n_ch} lookup {lookup} node {node}"
            want = oracle.eval_sample_nch([O], wi, wo, u, None, oracle.make_opts(lookup, node))
            fused = [_np(t) for t in g.eval_sample_nch(dwi, dwo, du, n_ch, material=mid)]
            ok = np.abs(fused[0].astype(np.float64) - want[0]) <= REL * np.abs(want[0]) + 1e-30
            if lookup == 1:
                assert ok[~ill].all(), (tag, int((~ok[~ill]).sum()))
            else:
                assert (~ok[~ill].all(axis=1)).sum() <= 1, tag
            assert np.array_equal(fused[1], want[1]) and np.array_equal(fused[2], want[2]) and np.array_equal(fused[3], want[3]), tag
            okw = np.abs(fused[4].astype(np.float64) - want[4]) <= REL * np.abs(want[4]) + 1e-30
            assert okw.all() if lookup == 1 else (~okw.all(axis=1)).sum() <= 1, tag + " weight"
            _same((g.eval_nch(dwi, dwo, n_ch, material=mid),), fused[:1], tag + " eval_nch")
            _same(g.eval_pdf_nch(dwi, dwo, n_ch, material=mid), fused[:2], tag + " eval_pdf_nch")
            _same(g.sample_nch(dwi, du, n_ch, material=mid), fused[2:], tag + " sample_nch")
            _same(g.eval_sample_nch(wi, wo, u, n_ch, material=mid), fused, tag + " host arrays")
        g.set_option(host.OPT_LOOKUP, 1); g.set_option(host.OPT_NODE, 0)
        # queues: a shuffled partial queue gives the whole-array bits on its slots and leaves every other slot alone
        n = wi.shape[0]
        perm = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)).to(torch.int32)
        queue, k = perm[: n - 50].contiguous(), n // 2 + 5
        count = torch.tensor([k], dtype=torch.int32, device="cuda")
        lv = queue[:k].long()
        rest = torch.ones(n, dtype=torch.bool, device="cuda"); rest[lv] = False
        whole = g.eval_sample_nch(dwi, dwo, du, n_ch, material=mid)
        outs = tuple(torch.full_like(t, -7.0) for t in whole)
        g.eval_sample_queue_nch(dwi, dwo, du, queue, count, n_ch, material=mid, out=outs)
        for got, ref in zip(outs, whole):
            assert torch.equal(got[lv].view(torch.int32), ref[lv].view(torch.int32)) and bool((got[rest] == -7.0).all()), name
        _same((g.eval_queue_nch(dwi, dwo, queue, count, n_ch, material=mid)[lv],), (whole[0][lv],), name + " eval_queue_nch")
        _same([t[lv] for t in g.eval_pdf_queue_nch(dwi, dwo, queue, count, n_ch, material=mid)], [t[lv] for t in whole[:2]], name + " eval_pdf_queue_nch")
        _same([t[lv] for t in g.sample_queue_nch(dwi, du, queue, count, n_ch, material=mid)], [t[lv] for t in whole[2:]], name + " sample_queue_nch")
        # table sampling: mode 2 falls back to the marginal sampler of mode 1
        g.set_option(host.OPT_SAMPLING, 1)
        one = [t.clone() for t in g.eval_sample_nch(dwi, dwo, du, n_ch, material=mid)]
        g.set_option(host.OPT_SAMPLING, 2)
        _same(g.eval_sample_nch(dwi, dwo, du, n_ch, material=mid), one, name + " sampling 2 == sampling 1")
