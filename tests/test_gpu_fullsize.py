"""Full-size GPU checks at BASELINE.json's batch sizes (64M single material, 256M mixed materials)
through size-independent properties — the oracle cannot evaluate 64M units in seconds, so it only
spot-checks a strided sample; everything else is checked on the device over ALL units:
  tile invariance (one launch == chunked launches, bit for bit), constant-table known answer,
  reciprocity, sample/eval consistency, linearity in the table, mixed == per-material launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N64 = 64 * (1 << 20)
SEED = 0x5EED


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from mitsuba_customization_amd import host
    h = host.MerlHip(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def batch64(gpu):
    return gpu.generate_pairs(SEED, 0, N64)


def _spot(n, k=8192):
    import torch
    return (torch.arange(k, device="cuda", dtype=torch.int64) * (n - 1)) // (k - 1)


def _rel_ok(got, want, rel=1e-6):
    got = got.astype(np.float64); want = want.astype(np.float64)
    return bool((np.abs(got - want) <= rel * np.abs(want) + 1e-30).all())


def test_64m_tile_invariance_and_oracle_spot_check(gpu, batch64, oracle, tables):
    import torch
    tab = tables("ggx_tab", 0)
    mid = gpu.upload_merl(tab)
    wi, wo, u = batch64
    one = gpu.eval_sample(wi, wo, u, material=mid)
    # the same units in 5 ragged launches
    cuts = [0, 13_000_001, 13_000_002, 40_000_000, 63_999_999, N64]
    parts = [gpu.eval_sample(wi[a:b], wo[a:b], u[a:b], material=mid) for a, b in zip(cuts, cuts[1:])]
    for k in range(5):
        assert torch.equal(one[k], torch.cat([p[k] for p in parts])), f"output {k} depends on the launch tiling"
    idx = _spot(N64)
    ref = oracle.eval_sample_multi([oracle.OracleTable(tab)], wi[idx].cpu().numpy(), wo[idx].cpu().numpy(), u[idx].cpu().numpy(), None)
    got = [o[idx].cpu().numpy() for o in one]
    assert _rel_ok(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[3], ref[3]) and _rel_ok(got[4], ref[4])
    # the device generator is the oracle's generator
    cwi, cwo, cu = oracle.generate_pairs(SEED, N64 - 1000, 1000)
    assert np.array_equal(wi[-1000:].cpu().numpy(), cwi) and np.array_equal(u[-1000:].cpu().numpy(), cu)


def test_64m_constant_table_known_answer(gpu, batch64, tables):
    import torch
    from mitsuba_customization_amd import synth
    mid = gpu.upload_merl(tables("constant"))
    wi, wo, u = batch64
    rgb = gpu.eval(wi, wo, material=mid)
    for c, raw in enumerate((300.0, 200.0, 100.0)):
        want = (wo[:, 2].double() * (raw * synth.MERL_SCALE[c])).float()
        # the 8 Float corner weights sum to 1 only up to rounding and the packed-Float blend adds 5 more roundings
        # (merl_device.hpp::blend_brick: bound 3.6e-7, + the cosine product's): 5e-7, half the 1e-6 parity bar
        assert bool(((rgb[:, c] - want).abs() <= 5e-7 * want.abs()).all())
    pdf = gpu.pdf(wi, wo, material=mid)
    assert torch.equal(pdf, wo[:, 2] * torch.tensor(0.31830988618379067154, dtype=torch.float32, device="cuda"))


def test_64m_reciprocity_and_sample_consistency(gpu, batch64, tables):
    import torch
    mid = gpu.upload_merl(tables("ggx_tab", 2))
    wi, wo, u = batch64
    f_io = gpu.eval(wi, wo, material=mid)
    f_oi = gpu.eval(wo, wi, material=mid)
    a = f_io.double() / wo[:, 2:3].double()
    b = f_oi.double() / wi[:, 2:3].double()
    assert bool(((a - b).abs() <= 4e-7 * a.abs() + 1e-30).all()), "f(wi,wo) != f(wo,wi)"
    del a, b, f_io, f_oi
    wo2, pdf2, w = gpu.sample(wi, u, material=mid)
    f2 = gpu.eval(wi, wo2, material=mid)
    assert torch.equal(w, f2 / pdf2[:, None]), "sample weight is not eval(wi, wo')/pdf in Float"
    assert bool((wo2[:, 2] > 0).all()) and bool(((wo2.double().norm(dim=1) - 1).abs() < 3e-7).all())
    # cosine-hemisphere law: E[z^2] = 1/2, E[z] = 2/3
    assert abs(float(wo2[:, 2].double().mean()) - 2 / 3) < 3e-4


def test_64m_linearity_in_the_table(gpu, batch64, tables):
    ta, tb = tables("ggx_tab", 4), tables("noise", 8)
    ta = np.maximum(ta, 0.0); tb = np.maximum(tb, 0.0)            # clamping is not linear: compare clamped tables
    ia, ib, iab = gpu.upload_merl(ta), gpu.upload_merl(tb), gpu.upload_merl(ta + tb)
    wi, wo, u = batch64
    fa = gpu.eval(wi, wo, material=ia).double()
    fb = gpu.eval(wi, wo, material=ib).double()
    fab = gpu.eval(wi, wo, material=iab).double()
    assert bool(((fab - (fa + fb)).abs() <= 5e-7 * fab.abs() + 1e-30).all())


def test_64m_standard_parameterisation_properties(batch64, oracle, tables):
    """A (theta_i, theta_o, |dphi|) table over all 64M units (MRL_OPT_TABLE_PARAM = standard): tile invariance; mirroring
    BOTH directions in the plane y = 0 flips the sign of dphi and nothing else, so eval is bit-identical; the full-azimuth
    form tells the two apart; a strided sample against the oracle."""
    import torch
    from mitsuba_customization_amd import host
    wi, wo, u = batch64
    dims = (64, 64, 128)
    scale = (1.0 / 1500.0, 1.15 / 1500.0, 1.66 / 1500.0)
    flip = torch.tensor([1.0, -1.0, 1.0], device="cuda")
    with host.MerlHip(0) as g:
        g.set_option(host.OPT_TABLE_PARAM, host.PARAM_STANDARD)
        std = g.upload_table(tables("noise", 21, dims), scale)
        g.set_option(host.OPT_TABLE_PARAM, host.PARAM_STANDARD_FULL)
        full = g.upload_table(tables("ggx_std_full", 3, dims), scale)
        one = g.eval_sample(wi, wo, u, material=std)
        cuts = [0, 21_000_003, 21_000_004, N64]
        parts = [g.eval_sample(wi[a:b], wo[a:b], u[a:b], material=std) for a, b in zip(cuts, cuts[1:])]
        for k in range(5):
            assert torch.equal(one[k], torch.cat([p[k] for p in parts])), f"output {k} depends on the launch tiling"
        rgb = one[0]
        mirrored = g.eval(wi * flip, wo * flip, material=std)
        assert torch.equal(rgb.view(torch.int32), mirrored.view(torch.int32))
        a = g.eval(wi[: 1 << 22], wo[: 1 << 22], material=full)
        b = g.eval(wi[: 1 << 22] * flip, wo[: 1 << 22] * flip, material=full)
        assert float(((a - b).abs() > 1e-3 * a.abs()).float().mean()) > 0.5
        idx = _spot(N64)
        ref = oracle.eval_sample_multi([oracle.OracleTable(tables("noise", 21, dims), scale, param=1)], wi[idx].cpu().numpy(), wo[idx].cpu().numpy(),
                                       u[idx].cpu().numpy(), None)
        got = [o[idx].cpu().numpy() for o in one]
    assert _rel_ok(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[3], ref[3]) and _rel_ok(got[4], ref[4])


def test_256m_mixed_16_materials(gpu, oracle, tables):
    """BASELINE config 4: 16 MERL materials mixed in one 256M batch."""
    import torch
    n = 256 * (1 << 20)
    tabs = [tables("ggx_tab", 200 + i) for i in range(16)]
    base = gpu.material_count()
    ids = [gpu.upload_merl(t) for t in tabs]
    assert ids == list(range(base, base + 16))
    wi, wo, u = gpu.generate_pairs(SEED, 0, n)
    mat = gpu.generate_materials(SEED, 0, n, 16)
    mat += base
    out = gpu.eval_sample(wi, wo, u, mat=mat)
    idx = _spot(n, 16384)
    local = (mat[idx] - base).cpu().numpy()
    ref = oracle.eval_sample_multi([oracle.OracleTable(t) for t in tabs], wi[idx].cpu().numpy(), wo[idx].cpu().numpy(),
                                   u[idx].cpu().numpy(), local)
    got = [o[idx].cpu().numpy() for o in out]
    assert _rel_ok(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[3], ref[3]) and _rel_ok(got[4], ref[4])
    # a mixed launch equals the single-material launch of each material on that material's units
    for k in (0, 7, 15):
        sel = torch.nonzero(mat[: 8 * (1 << 20)] == base + k).flatten()
        single = gpu.eval(wi[sel].contiguous(), wo[sel].contiguous(), material=base + k)
        assert torch.equal(single, out[0][sel])
    counts = torch.bincount((mat - base).long(), minlength=16).double() / n
    assert float((counts - 1 / 16).abs().max()) < 1e-3


def test_1b_units_100_resident_tables(oracle, tables):
    """BASELINE config 5's single-GPU worth and beyond: 100 MERL tables resident (18.7 GB of bricks), ONE
    launch over 2^30 units (80 GB of streams: every array is larger than 4 GB, so 64-bit indexing is live).
    Checked: oracle spot-check spread over the whole range incl. the last units, and tile invariance —
    the tail of the big launch equals a small launch over the same pair indices, bit for bit."""
    import torch
    from mitsuba_customization_amd import host
    n = 1 << 30
    free, _total = torch.cuda.mem_get_info()
    if free < 120 * (1 << 30):
        pytest.skip("needs ~105 GB of free HBM")
    distinct = [tables("ggx_tab", 500 + i) for i in range(4)]
    with host.MerlHip(0) as g:
        ids = [g.upload_merl(distinct[i % 4]) for i in range(100)]
        assert ids == list(range(100))
        wi, wo, u = g.generate_pairs(SEED, 0, n)
        mat = g.generate_materials(SEED, 0, n, 100)
        out = g.eval_sample(wi, wo, u, mat=mat)
        torch.cuda.synchronize()
        # spot check: 4096 units spread over the range + the last 64
        idx = torch.cat([_spot(n, 4096), torch.arange(n - 64, n, device="cuda")])
        hm = mat[idx].cpu().numpy()
        ref = oracle.eval_sample_multi([oracle.OracleTable(distinct[i % 4]) for i in range(100)],
                                       wi[idx].cpu().numpy(), wo[idx].cpu().numpy(), u[idx].cpu().numpy(), hm)
        got = [o[idx].cpu().numpy() for o in out]
        assert _rel_ok(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert np.array_equal(got[3], ref[3]) and _rel_ok(got[4], ref[4])
        # the generator at indices beyond 2^32 / 3 etc. is the oracle's
        cwi, _, cu = oracle.generate_pairs(SEED, n - 1000, 1000)
        assert np.array_equal(wi[-1000:].cpu().numpy(), cwi) and np.array_equal(u[-1000:].cpu().numpy(), cu)
        assert np.array_equal(mat[-1000:].cpu().numpy(), oracle.generate_materials(SEED, n - 1000, 1000, 100))
        # tail of the big launch == a separate small launch on the same units
        lo = n - 3_000_001
        small = g.eval_sample(wi[lo:].contiguous(), wo[lo:].contiguous(), u[lo:].contiguous(), mat=mat[lo:].contiguous())
        for a, b in zip(out, small):
            assert torch.equal(a[lo:], b)


def test_one_table_beyond_four_gigabytes(oracle):
    """A single customized_measurement table whose brick image exceeds 2^32 bytes (256 x 256 x 520 cells x 128 B = 4.36 GB):
    every byte offset into it needs 64-bit arithmetic.  Lookups are compared with the oracle over the whole table, and in
    particular in its last rows (the bytes beyond 4 GB)."""
    from mitsuba_customization_amd import host, synth
    dims = (256, 256, 520)
    tab = synth.noise_table(77, dims=dims, decades=3.0, negative_fraction=0.0)
    scale = (1.0, 1.0, 1.0)
    n = 200_000
    wi, wo, u = oracle.generate_pairs(0x5EED, 2468, n)
    # half of the pairs with BOTH directions grazing and 0.3 .. 2 rad apart in azimuth: the half vector grazes too, i.e.
    # theta_h near pi/2 = the table's last rows, with theta_d well away from 0
    k = n // 2
    rng = np.random.default_rng(5)
    z1, z2 = rng.uniform(1e-3, 0.05, k), rng.uniform(1e-3, 0.05, k)
    p1 = rng.uniform(0, 2 * np.pi, k); p2 = p1 + rng.uniform(0.3, 2.0, k)
    wi[:k] = np.stack([np.sqrt(1 - z1 * z1) * np.cos(p1), np.sqrt(1 - z1 * z1) * np.sin(p1), z1], 1).astype(np.float32)
    wo[:k] = np.stack([np.sqrt(1 - z2 * z2) * np.cos(p2), np.sqrt(1 - z2 * z2) * np.sin(p2), z2], 1).astype(np.float32)
    T = oracle.OracleTable(tab, scale)
    want = oracle.eval_sample_multi([T], wi, wo, u, None, oracle.make_opts())
    with host.MerlHip(0) as g:
        mid = g.upload_table(tab, scale)
        assert g.memory_info()["table_bytes"] > (1 << 32)
        got = [np.asarray(t) for t in g.eval_sample(wi, wo, u, material=mid)]
        one = g.scalar_eval_sample(wi[5], wo[5], u[5], material=mid)
    a = wi.astype(np.float64); b = wo.astype(np.float64)
    a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
    h = a + b
    th = np.arctan2(np.hypot(h[:, 0], h[:, 1]), h[:, 2])
    last_rows = np.sqrt(th / (np.pi / 2)) * dims[0] > 0.985 * dims[0]           # cells past byte offset 2^32
    assert last_rows.sum() > 1000
    td = np.arctan2(np.linalg.norm(a - b, axis=1), np.linalg.norm(h, axis=1))
    well = (th > 0.02) & (td > 0.02)                                         # the noise table's ill-conditioned corner: test_gpu_parity
    for kk in (0, 4):
        ok = np.abs(got[kk].astype(np.float64) - want[kk]) <= 1e-6 * np.abs(want[kk]) + 1e-30
        sel = well if kk == 0 else np.ones(n, bool)
        assert ok[sel].all(), (kk, int((~ok[sel]).sum()))
    assert (well & last_rows).sum() > 1000
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.allclose(one[:3], got[0][5], rtol=2e-6, atol=1e-30)


def test_largest_table_on_32_bit_byte_offsets(oracle):
    """The largest single table whose LDS-DMA fetch still takes 32-bit byte offsets (k_table_dma: offsets32 when n_th n_td n_pd
    <= 2^25): 256 x 256 x 512 = 2^25 cells, whose last brick starts at byte 2^32 - 128.  Lookups aimed at the last rows (as in
    test_one_table_beyond_four_gigabytes) against the oracle; variant 3 (k_table_dma) and variant 1 (k_table, 64-bit indexing)
    with the same bits."""
    import torch
    from mitsuba_customization_amd import host, synth
    dims = (256, 256, 512)
    assert dims[0] * dims[1] * dims[2] == 1 << 25
    tab = synth.noise_table(78, dims=dims, decades=3.0, negative_fraction=0.0)
    scale = (1.0, 1.0, 1.0)
    n = 200_000
    wi, wo, u = oracle.generate_pairs(0x5EED, 8642, n)
    k = n // 2
    rng = np.random.default_rng(7)
    z1, z2 = rng.uniform(1e-3, 0.05, k), rng.uniform(1e-3, 0.05, k)
    p1 = rng.uniform(0, 2 * np.pi, k); p2 = p1 + rng.uniform(0.3, 2.0, k)
    wi[:k] = np.stack([np.sqrt(1 - z1 * z1) * np.cos(p1), np.sqrt(1 - z1 * z1) * np.sin(p1), z1], 1).astype(np.float32)
    wo[:k] = np.stack([np.sqrt(1 - z2 * z2) * np.cos(p2), np.sqrt(1 - z2 * z2) * np.sin(p2), z2], 1).astype(np.float32)
    T = oracle.OracleTable(tab, scale)
    want = oracle.eval_sample_multi([T], wi, wo, u, None, oracle.make_opts())
    with host.MerlHip(0) as g:
        mid = g.upload_table(tab, scale)
        del tab
        assert g.memory_info()["table_bytes"] >= (1 << 32)
        assert g.get_option(host.OPT_KERNEL) == 3
        dwi, dwo, du = [torch.from_numpy(a).cuda() for a in (wi, wo, u)]
        dma = [t.cpu().numpy() for t in g.eval_sample(dwi, dwo, du, material=mid)]
        g.set_option(host.OPT_KERNEL, 1)
        tuned = [t.cpu().numpy() for t in g.eval_sample(dwi, dwo, du, material=mid)]
    for a, b in zip(dma, tuned):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "k_table_dma (32-bit offsets) and k_table differ"
    a = wi.astype(np.float64); b = wo.astype(np.float64)
    a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
    h = a + b
    th = np.arctan2(np.hypot(h[:, 0], h[:, 1]), h[:, 2])
    last_rows = np.sqrt(th / (np.pi / 2)) * dims[0] > 0.985 * dims[0]           # the bricks just below byte offset 2^32
    td = np.arctan2(np.linalg.norm(a - b, axis=1), np.linalg.norm(h, axis=1))
    well = (th > 0.02) & (td > 0.02)                                         # the noise table's ill-conditioned corner: test_gpu_parity
    assert (well & last_rows).sum() > 1000
    assert (np.floor(np.sqrt(th / (np.pi / 2)) * dims[0]) >= dims[0] - 1).sum() > 100   # the last theta_h row itself
    for kk in (0, 4):
        ok = np.abs(dma[kk].astype(np.float64) - want[kk]) <= 1e-6 * np.abs(want[kk]) + 1e-30
        sel = well if kk == 0 else np.ones(n, bool)
        assert ok[sel].all(), (kk, int((~ok[sel]).sum()))
    assert np.array_equal(dma[1], want[1]) and np.array_equal(dma[2], want[2]) and np.array_equal(dma[3], want[3])


def test_one_wide_table_beyond_four_gigabytes(oracle):
    """The same for the n-channel kernels: 8 channels x 160 x 160 x 680 cells x 256 B = 4.46 GB of bricks."""
    from mitsuba_customization_amd import host, synth
    dims, n_ch = (160, 160, 680), 8
    planes = [synth.noise_table(100 + c, dims=dims, decades=3.0, negative_fraction=0.0)[0] for c in range(n_ch)]
    tab = np.stack(planes, axis=0)
    del planes
    n = 100_000
    wi, wo, u = oracle.generate_pairs(0x5EED, 1357, n)
    k = n // 2
    rng = np.random.default_rng(6)
    z1, z2 = rng.uniform(1e-3, 0.05, k), rng.uniform(1e-3, 0.05, k)
    p1 = rng.uniform(0, 2 * np.pi, k); p2 = p1 + rng.uniform(0.3, 2.0, k)
    wi[:k] = np.stack([np.sqrt(1 - z1 * z1) * np.cos(p1), np.sqrt(1 - z1 * z1) * np.sin(p1), z1], 1).astype(np.float32)
    wo[:k] = np.stack([np.sqrt(1 - z2 * z2) * np.cos(p2), np.sqrt(1 - z2 * z2) * np.sin(p2), z2], 1).astype(np.float32)
    want = oracle.eval_sample_nch([oracle.OracleTableNch(tab)], wi, wo, u, None, oracle.make_opts())
    with host.MerlHip(0) as g:
        mid = g.upload_table_nch(tab)
        assert g.memory_info()["table_bytes"] > (1 << 32)
        got = [np.asarray(t) for t in g.eval_sample_nch(wi, wo, u, n_ch, material=mid)]
    a = wi.astype(np.float64); b = wo.astype(np.float64)
    a /= np.linalg.norm(a, axis=1, keepdims=True); b /= np.linalg.norm(b, axis=1, keepdims=True)
    h = a + b
    th = np.arctan2(np.hypot(h[:, 0], h[:, 1]), h[:, 2]); td = np.arctan2(np.linalg.norm(a - b, axis=1), np.linalg.norm(h, axis=1))
    well = (th > 0.02) & (td > 0.02)
    assert (well & (np.sqrt(th / (np.pi / 2)) * dims[0] > 0.985 * dims[0])).sum() > 1000
    ok = np.abs(got[0].astype(np.float64) - want[0]) <= 1e-6 * np.abs(want[0]) + 1e-30
    assert ok[well].all(), int((~ok[well]).sum())
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


def test_64m_ggx_rough_conductor(gpu, batch64, oracle):
    """BASELINE configs[2] at its size: GGX rough conductor alpha = 0.1, analytic eval + visible-normal sample over all 64M units —
    tile invariance (one launch == ragged launches, bit for bit), a strided sample against the oracle, the fused entry point against
    the separate ones, and the size-independent properties of the model over ALL units: reciprocity of f = eval / cos(theta_o)
    (the microfacet BRDF is symmetric), the pdf of a sampled direction re-evaluated by pdf(), energy bounds of the weight
    (F G1 <= 1 per channel), unit-length directions above the horizon."""
    import torch
    eta, k = (0.143, 0.375, 1.442), (3.983, 2.386, 1.603)
    mid = gpu.ggx(0.1, eta, k)
    wi, wo, u = batch64
    one = gpu.eval_sample(wi, wo, u, material=mid)
    cuts = [0, 7_000_001, 7_000_002, 33_554_432, 63_999_999, N64]
    parts = [gpu.eval_sample(wi[a:b], wo[a:b], u[a:b], material=mid) for a, b in zip(cuts, cuts[1:])]
    for q in range(5):
        assert torch.equal(one[q], torch.cat([p[q] for p in parts])), f"output {q} depends on the launch tiling"
    del parts
    rgb, pdf, wo2, pdf2, w = one
    # the separate entry points give the fused call's bits
    assert torch.equal(gpu.eval(wi, wo, material=mid), rgb) and torch.equal(gpu.pdf(wi, wo, material=mid), pdf)
    s_wo, s_pdf, s_w = gpu.sample(wi, u, material=mid)
    assert torch.equal(s_wo, wo2) and torch.equal(s_pdf, pdf2) and torch.equal(s_w, w)
    del s_wo, s_pdf, s_w
    # a strided sample against the oracle (tolerances of tests/test_gpu_parity.py::test_ggx_matches_oracle)
    idx = _spot(N64)
    G = oracle.OracleGgx(np.float32(0.1).item(), [np.float32(x).item() for x in eta], [np.float32(x).item() for x in k])
    hwi, hwo, hu = wi[idx].cpu().numpy(), wo[idx].cpu().numpy(), u[idx].cpu().numpy()
    assert _rel_ok(rgb[idx].cpu().numpy(), G.eval(hwi, hwo)) and _rel_ok(pdf[idx].cpu().numpy(), G.pdf(hwi, hwo))
    c_wo, c_pdf, c_w = G.sample(hwi, hu)
    assert float(np.abs(wo2[idx].cpu().numpy().astype(np.float64) - c_wo).max()) <= 1.2e-7
    assert _rel_ok(pdf2[idx].cpu().numpy(), c_pdf, rel=2e-6) and _rel_ok(w[idx].cpu().numpy(), c_w)
    # reciprocity of the BRDF over all units: eval(wi, wo) / wo.z == eval(wo, wi) / wi.z  (f64 results rounded once to Float)
    f_oi = gpu.eval(wo, wi, material=mid)
    a = rgb.double() / wo[:, 2:3].double()
    b = f_oi.double() / wi[:, 2:3].double()
    assert bool(((a - b).abs() <= 4e-7 * a.abs() + 1e-30).all()), "f(wi, wo) != f(wo, wi)"
    del a, b, f_oi
    # sample(): accepted directions are unit vectors above the horizon, their pdf is what pdf() says there, the weight F G1 is bounded
    live = pdf2 > 0
    assert 0.5 < float(live.float().mean()) <= 1.0
    assert bool((wo2[live][:, 2] > 0).all()) and bool(((wo2[live].double().norm(dim=1) - 1).abs() < 3e-7).all())
    back = gpu.pdf(wi, wo2, material=mid)
    rel = ((back[live].double() - pdf2[live].double()).abs() / pdf2[live].double())
    # (the device forms the pdf at the f64 direction, pdf() at its Float rounding: 1e-7 of direction error against a lobe of width alpha)
    assert float(rel.max()) < 5e-4 and float((rel > 3e-6).float().mean()) < 5e-3          # measured: 1.2e-4, 0.16 %
    assert bool((w[live] >= 0).all()) and bool((w[live] <= 1.0 + 1e-6).all())
    assert bool((w[~live] == 0).all()) and bool((wo2[~live] == 0).all())
