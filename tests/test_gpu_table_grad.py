"""mrl_table_grad_batch / MerlHip.table_grad, G += A^T g, against the numpy reference of A^T (tests/table_grad_reference.py).
Per cell and channel: |G - R| <= 1e-6 S with S = sum_u |a_u g_u| from the reference, and G == 0 exactly where S == 0."""
import numpy as np
import pytest

from tests import table_grad_reference as ref

pytestmark = pytest.mark.gpu

MERL = (90, 90, 180)
SCALE = (0.7, 1.3, 2.1)
N = 1 << 20


def _ctx(lookup=1, node=0, cosine=0, negative=0, variant=0):
    from mitsuba_customization_amd import host
    g = host.MerlHip(0)
    g.set_option(host.OPT_LOOKUP, lookup); g.set_option(host.OPT_NODE, node)
    g.set_option(host.OPT_COSINE_FACTOR, cosine); g.set_option(host.OPT_NEGATIVE, negative)
    g.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
    return g


def _shape_table(g, dims, param=ref.HALF_DIFF, scale=SCALE):
    return g.upload_table_param(np.ones((3,) + tuple(dims)), param, scale)


def _pairs(n, seed=0x5EED):
    from oracle import binding
    wi, wo, _ = binding.generate_pairs(seed, 0, n)
    return np.ascontiguousarray(wi, np.float32), np.ascontiguousarray(wo, np.float32)


def _signed(n, seed=1):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


def _drop_boundary_units(wi, wo, g, dims, param):
    near = ref.near_cell_boundary(wi, wo, dims, param)
    assert near.sum() <= 16, int(near.sum())                 # asserted on the reference alone
    return wi[~near], wo[~near], g[~near]


def _check(G, R, S, what, factor=1e-6):
    G = np.asarray(G)
    err = np.abs(G - R)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(S > 0, err / S, 0.0)))
    print(f"{what}: worst |G - R| / S = {worst:.3e}, cells reached {int((S > 0).sum())}")
    assert np.isfinite(G).all(), what
    assert (err <= factor * S).all(), (what, worst)
    assert (G[S == 0] == 0).all(), what


def _device(*arrays):
    import torch
    return [torch.from_numpy(a).cuda() for a in arrays]


@pytest.mark.parametrize("lookup,node,cosine", ((1, 0, 0), (1, 1, 0), (0, 0, 0), (1, 0, 1), (0, 0, 1)))
def test_merl_dims_random_pairs(lookup, node, cosine):
    wi, wo = _pairs(N); g = _signed(N)
    if not lookup:
        wi, wo, g = _drop_boundary_units(wi, wo, g, MERL, ref.HALF_DIFF)
    R, S = ref.adjoint(wi, wo, g, MERL, trilinear=bool(lookup), center=bool(node), cosine=not cosine, scale=SCALE)
    got = []
    for negative in (0, 1):                                   # clamp and keep: the same operator
        with _ctx(lookup, node, cosine, negative) as gpu:
            mid = _shape_table(gpu, MERL)
            G = gpu.table_grad(*_device(wi, wo, g), material=mid).cpu().numpy()
        _check(G, R, S, f"lookup {lookup} node {node} cosine {cosine} negative {negative}")
        got.append(G)
    assert (np.abs(got[0] - got[1]) <= 1e-12 * S).all()


@pytest.mark.parametrize("dims", ((7, 5, 12), (33, 17, 64)))
@pytest.mark.parametrize("param", (ref.HALF_DIFF, ref.STANDARD, ref.STANDARD_FULL))
def test_free_dims_and_parameterisations(dims, param):
    n = 1 << 18
    wi0, wo0 = _pairs(n, 0xF00D + param); g0 = _signed(n, 2)
    for lookup, node in ((1, 0), (1, 1), (0, 0)):
        wi, wo, g = (wi0, wo0, g0) if lookup else _drop_boundary_units(wi0, wo0, g0, dims, param)
        R, S = ref.adjoint(wi, wo, g, dims, param=param, trilinear=bool(lookup), center=bool(node), scale=SCALE)
        with _ctx(lookup, node) as gpu:
            mid = _shape_table(gpu, dims, param)
            G = gpu.table_grad(*_device(wi, wo, g), material=mid).cpu().numpy()
        _check(G, R, S, f"dims {dims} param {param} lookup {lookup} node {node}")


def test_coherent_set_is_accumulated_to_the_bar():
    from mitsuba_customization_amd import synth
    wi, wo = synth.coherent_pairs(N); g = _signed(N, 3)
    R, S = ref.adjoint(wi, wo, g, MERL, scale=SCALE)
    assert (S.sum(0) > 0).sum() < 50000                      # a few thousand hot cells take all 2^20 units
    with _ctx() as gpu:
        mid = _shape_table(gpu, MERL)
        G = gpu.table_grad(*_device(wi, wo, g), material=mid).cpu().numpy()
    _check(G, R, S, "coherent")


@pytest.mark.parametrize("variant", (0, 1, 2, 3))
def test_every_internal_variant_computes_the_same_operator(variant):
    n = 1 << 16
    half = n // 2
    from mitsuba_customization_amd import synth
    wi_r, wo_r = _pairs(half, 11); wi_c, wo_c = synth.coherent_pairs(half)
    wi_c[: half // 2] = wi_c[0]; wo_c[: half // 2] = wo_c[0]              # whole waves on one cell: the merged path's case
    wi = np.concatenate([wi_c, wi_r]); wo = np.concatenate([wo_c, wo_r]); g = _signed(n, 4)
    for lookup in (1, 0):
        a, b, c = (wi, wo, g) if lookup else _drop_boundary_units(wi, wo, g, (33, 17, 64), ref.HALF_DIFF)
        R, S = ref.adjoint(a, b, c, (33, 17, 64), trilinear=bool(lookup), scale=SCALE)
        with _ctx(lookup=lookup, variant=variant) as gpu:
            mid = _shape_table(gpu, (33, 17, 64))
            G = gpu.table_grad(*_device(a, b, c), material=mid).cpu().numpy()
        _check(G, R, S, f"variant {variant} lookup {lookup}")


def test_masking_accumulation_untouched_cells_and_empty_batch():
    import torch
    dims = (33, 17, 64)
    n = 1 << 14
    wi, wo = _pairs(n, 21); g = _signed(n, 5)
    wo[0::7, 2] *= -1.0; wi[1::7, 2] = 0.0 - wi[1::7, 2]      # below the horizon on either side
    wi[2::7] = np.nan; wo[3::7, 0] = np.inf; wi[4::7] = 0.0    # NaN, inf and zero-length directions
    dead = ~ref.guard(wi, wo)
    assert dead.sum() > n // 2
    g[dead] = np.where(np.arange(dead.sum())[:, None] % 2 == 0, np.nan, np.inf).astype(np.float32)
    live = ~dead
    R, S = ref.adjoint(wi[live], wo[live], g[live], dims, scale=SCALE)
    with _ctx() as gpu:
        mid = _shape_table(gpu, dims)
        dwi, dwo, dg = _device(wi, wo, g)
        G = gpu.table_grad(dwi, dwo, dg, material=mid)
        _check(G.cpu().numpy(), R, S, "masked units")
        again = gpu.table_grad(dwi, dwo, dg, material=mid, out=G)
        assert again is G
        _check(G.cpu().numpy(), 2 * R, 2 * S, "second call accumulates")
        # a pre-filled buffer: what no unit reaches keeps its bits (negative zeros and NaN payloads included)
        fill = np.random.default_rng(6).standard_normal(R.shape)
        fill[0, :2] = -0.0
        pre = torch.from_numpy(fill.copy()).cuda()
        gpu.table_grad(dwi, dwo, dg, material=mid, out=pre)
        out = pre.cpu().numpy()
        untouched = S == 0
        assert untouched.sum() > 0
        assert np.array_equal(out[untouched].view(np.uint64), fill[untouched].view(np.uint64))
        assert (np.abs(out - fill - R) <= 1e-6 * S + 1e-15 * np.abs(fill)).all()
        # n == 0: MRL_OK, nothing touched, whatever the pointers are
        before = pre.clone()
        assert gpu._lib.mrl_table_grad_batch(gpu._ctx, None, None, None, mid, 0, None) == 0
        empty = torch.empty((0, 3), dtype=torch.float32, device="cuda")
        gpu.table_grad(empty, empty, empty, material=mid, out=pre)
        gpu.synchronize()
        assert torch.equal(pre.view(torch.int64), before.view(torch.int64))


@pytest.mark.parametrize("dims,lookup,node", ((MERL, 1, 0), ((33, 17, 64), 1, 1), ((33, 17, 64), 0, 0)))
def test_transpose_of_the_shipped_forward(dims, lookup, node):
    n = 1 << 18
    wi, wo = _pairs(n, 31); g = _signed(n, 7)
    if not lookup:
        wi, wo, g = _drop_boundary_units(wi, wo, g, dims, ref.HALF_DIFF)
    T = np.random.default_rng(8).random((3,) + tuple(dims)) * 100.0
    _, S = ref.adjoint(wi, wo, g, dims, trilinear=bool(lookup), center=bool(node), scale=SCALE)
    with _ctx(lookup, node) as gpu:
        mid = gpu.upload_table(T, SCALE)
        dwi, dwo, dg = _device(wi, wo, g)
        ev = gpu.eval(dwi, dwo, material=mid).cpu().numpy().astype(np.float64)
        G = gpu.table_grad(dwi, dwo, dg, material=mid).cpu().numpy()
    lhs, rhs, terms = float((ev * g.astype(np.float64)).sum()), float((T * G).sum()), float((T * S).sum())
    print(f"<eval(T), g> = {lhs!r}, <T, G> = {rhs!r}, sum |terms| = {terms!r}, ratio {abs(lhs - rhs) / terms:.3e}")
    assert abs(lhs - rhs) <= 2e-6 * terms


def test_host_pointers_device_tensors_and_out_agree():
    import torch
    from mitsuba_customization_amd import host
    dims = (33, 17, 64)
    n = 100003                                                 # not a multiple of the staging chunk
    wi, wo = _pairs(n, 41); g = _signed(n, 9)
    R, S = ref.adjoint(wi, wo, g, dims, scale=SCALE)
    with _ctx() as gpu:
        gpu.set_option(host.OPT_HOST_CHUNK, 1 << 15)
        mid = _shape_table(gpu, dims)
        Gh = gpu.table_grad(wi, wo, g, material=mid)
        assert isinstance(Gh, np.ndarray) and Gh.dtype == np.float64 and Gh.shape == (3,) + dims
        _check(Gh, R, S, "host arrays")
        Gd = gpu.table_grad(*_device(wi, wo, g), material=mid)
        assert isinstance(Gd, torch.Tensor) and Gd.is_cuda and Gd.dtype == torch.float64
        _check(Gd.cpu().numpy(), R, S, "device tensors")
        out = np.zeros_like(Gh)
        assert gpu.table_grad(wi, wo, g, material=mid, out=out) is out
        gpu.table_grad(wi, wo, g, material=mid, out=out)
        _check(out, 2 * R, 2 * S, "host out= accumulates")


def test_refusals_return_their_codes_and_leave_the_buffer_alone(tmp_path):
    import torch
    from mitsuba_customization_amd import host, synth
    dims = (7, 5, 12)
    n = 64
    wi, wo = _pairs(n, 51); g = _signed(n, 10)
    with _ctx(negative=1) as gpu:
        L, ctx = gpu._lib, gpu._ctx
        mid = _shape_table(gpu, dims)
        ggx = gpu.ggx(0.2, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2))
        nch = gpu.upload_table_nch(np.ones((5,) + dims))
        gone = _shape_table(gpu, dims); gpu.release_material(gone)
        rgl = gpu.upload_rgl(synth.make_rgl_fields(0))
        spectral = gpu.upload_rgl(synth.make_rgl_fields(0, n_wavelengths=4))
        assert gpu.material_info(spectral)[0] == host.KIND_RGL_SPECTRAL
        # a table restored from its device image: the image does not record the channel scales the call needs
        image = str(tmp_path / "shape.image")
        gpu.save_image(mid, image)
        restored = gpu.load_image(image)
        assert gpu.material_info(restored) == gpu.material_info(mid)
        fill = np.random.default_rng(12).standard_normal((3,) + dims)
        G = fill.copy()
        p = lambda a: a.ctypes.data
        call = lambda a, b, c, i, d: L.mrl_table_grad_batch(ctx, a, b, c, i, n, d)
        for bad in (ggx, nch, gone, rgl, spectral, restored, 99, -1):
            assert call(p(wi), p(wo), p(g), bad, p(G)) == -6, bad
        assert call(None, p(wo), p(g), mid, p(G)) == -1 and call(p(wi), None, p(g), mid, p(G)) == -1
        assert call(p(wi), p(wo), None, mid, p(G)) == -1 and call(p(wi), p(wo), p(g), mid, None) == -1
        dwi, dwo, dg = _device(wi, wo, g)
        dG = torch.from_numpy(fill.copy()).cuda()
        for bad in (ggx, nch, gone, rgl, spectral, restored, 99, -1):
            assert call(dwi.data_ptr(), dwo.data_ptr(), dg.data_ptr(), bad, dG.data_ptr()) == -6, bad
        assert call(dwi.data_ptr(), p(wo), p(g), mid, p(G)) == -7
        assert call(dwi.data_ptr(), dwo.data_ptr(), dg.data_ptr(), mid, p(G)) == -7
        assert call(p(wi), p(wo), p(g), mid, dG.data_ptr()) == -7
        gpu.set_option(host.OPT_NEGATIVE, 2)                    # renormalise: eval is not linear
        assert call(p(wi), p(wo), p(g), mid, p(G)) == -1
        assert call(dwi.data_ptr(), dwo.data_ptr(), dg.data_ptr(), mid, dG.data_ptr()) == -1
        gpu.synchronize()
        assert np.array_equal(G, fill) and np.array_equal(dG.cpu().numpy(), fill)
        gpu.set_option(host.OPT_NEGATIVE, 1)                    # and the context still works
        R, S = ref.adjoint(wi, wo, g, dims, scale=SCALE)
        _check(gpu.table_grad(wi, wo, g, material=mid), R, S, "after the refusals")


def test_workspace_is_accounted_and_reused():
    with _ctx() as gpu:
        mid = _shape_table(gpu, (33, 17, 64))
        before = gpu.memory_info()["workspace_bytes"]
        dwi, dwo, dg = _device(*_pairs(1024, 61), _signed(1024, 13))
        gpu.table_grad(dwi, dwo, dg, material=mid)
        after = gpu.memory_info()["workspace_bytes"]
        assert after - before == 33 * 17 * 64 * 256
        gpu.table_grad(dwi, dwo, dg, material=mid)
        assert gpu.memory_info()["workspace_bytes"] == after


def test_splat_is_the_weighted_mean_of_a_nearest_lookup():
    from mitsuba_customization_amd import fit
    dims = (12, 10, 16)
    n = 1 << 16
    wi, wo = _pairs(n, 71)
    near = ref.near_cell_boundary(wi, wo, dims)
    wi, wo = wi[~near], wo[~near]
    y = np.random.default_rng(14).random((len(wi), 3)).astype(np.float32)
    with _ctx(lookup=0, cosine=1) as gpu:
        table, mask = fit.splat(gpu, dims, wi, wo, y, scale=SCALE)
    ones = np.ones_like(y)
    num, _ = ref.adjoint(wi, wo, y, dims, trilinear=False, cosine=False, scale=SCALE)
    cnt, _ = ref.adjoint(wi, wo, ones, dims, trilinear=False, cosine=False, scale=(1.0, 1.0, 1.0))
    sc = np.asarray(SCALE)[:, None, None, None]
    want = np.where(cnt > 0, num / np.maximum(cnt, 1) / (sc * sc), 0.0)      # a = scale: sum a y / sum a^2 = mean(y) / scale
    assert np.array_equal(mask, cnt > 0) and mask.sum() > 0 and (~mask).sum() > 0
    assert (table[~mask] == 0).all()
    assert (np.abs(table - want) <= 1e-6 * np.abs(want)).all()


def test_fit_table_cgls_descends_below_the_splat(oracle):
    from mitsuba_customization_amd import fit, synth
    dims = (12, 10, 16)
    n = 1 << 18
    wi, wo = _pairs(n, 81)
    truth = synth.make_table("ggx_tab", 3, dims)
    y = oracle.OracleTable(truth, (1.0, 1.0, 1.0)).eval(wi, wo, oracle.make_opts(negative=oracle.NEGATIVE_KEEP))
    with _ctx(negative=1) as gpu:
        table, res = fit.fit_table(gpu, dims, wi, wo, y, 20)
    print("CGLS residuals:", " ".join(f"{r:.6e}" for r in res))
    assert len(res) == 21 and table.shape == (3,) + dims and np.isfinite(table).all()
    for a, b in zip(res, res[1:]):
        assert b <= a * (1 + 1e-6), (a, b)
    assert res[-1] < res[0]
    # the residuals come from a recurrence: the returned table, evaluated by the oracle, has the last of them.  Both sides carry
    # Float outputs of ~2^18 x 3 values (6e-8 relative each, of |y| not of the residual): 1e-6 |y| covers them
    keep = oracle.make_opts(negative=oracle.NEGATIVE_KEEP)
    true = float(np.linalg.norm(oracle.OracleTable(table, (1.0, 1.0, 1.0)).eval(wi, wo, keep).astype(np.float64) - y.astype(np.float64)))
    norm_y = float(np.linalg.norm(y.astype(np.float64)))
    print(f"|A T - y| of the returned table by the oracle: {true:.6e}, reported {res[-1]:.6e}, |y| {norm_y:.6e}")
    assert abs(true - res[-1]) <= 1e-6 * norm_y
    # device tensors in -> device tensors out, the same fit
    import torch
    dwi, dwo, dy = _device(wi, wo, y)
    with _ctx(negative=1) as gpu:
        dtable, dres = fit.fit_table(gpu, dims, dwi, dwo, dy, 20)
        stable, smask = fit.splat(gpu, dims, dwi, dwo, dy)
    assert isinstance(dtable, torch.Tensor) and dtable.is_cuda and dtable.dtype == torch.float64 and tuple(dtable.shape) == (3,) + dims
    assert isinstance(stable, torch.Tensor) and stable.is_cuda and smask.dtype == torch.bool
    print("CGLS residuals (device tensors):", " ".join(f"{r:.6e}" for r in dres))
    # the sums are f64 atomics in no fixed order, so the two runs differ by f64 rounding, which 20 CGLS steps may amplify: only the
    # splat's residual (two A^T, one A) is compared between the runs; the device run is held to the same conditions as the host run
    assert abs(dres[0] - res[0]) <= 1e-9 * res[0]
    assert len(dres) == 21 and dres[-1] < dres[0] and all(b <= a * (1 + 1e-6) for a, b in zip(dres, dres[1:]))
    dtrue = float(np.linalg.norm(oracle.OracleTable(dtable.cpu().numpy(), (1.0, 1.0, 1.0)).eval(wi, wo, keep).astype(np.float64) - y.astype(np.float64)))
    assert abs(dtrue - dres[-1]) <= 1e-6 * norm_y
