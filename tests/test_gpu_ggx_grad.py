"""mrl_ggx_grad_batch on the device against central differences of the numpy restatement of the model (tests/ggx_grad_reference.py,
which tests/test_ggx_grad_cpu.py shows to be converged on these cases): every case of ggx_reference.CASES — 6 alpha x 4 metals, 2^15
generate_pairs units and the targeted block with its NaN, inf, zero-length and below-horizon units, whose g and h are NaN / inf
here — then the shapes around a wave and a block and past one round of the grid, accumulation, determinism, host arrays, the error
returns and fit.fit_ggx end to end.

The bar is the project's: |G - R| <= 1e-6 S per parameter with S = sum |g J|, |N - R2| <= 1e-6 S2 per entry with S2 = sum |h J_a J_b|.
Measured on MI355X: worst |G - R| / S = 3.4e-9 and worst |N - R2| / S2 = 4.2e-8 over the 24 cases (the reference's own truncation
error); fit_ggx recovers (alpha, eta, k) to 7.6e-8 relative from f32 measurements."""
import numpy as np
import pytest

from tests import ggx_grad_reference as gref
from tests import ggx_reference as ggx

pytestmark = pytest.mark.gpu

REL = 1e-6
SENTINEL = -777.25
CASE_IDS = [ggx.case_id(c) for c in ggx.CASES]
CROSS = np.array([[not gref.same_channel(a, b) for b in range(7)] for a in range(7)])
WORST = {"grad": 0.0, "normal": 0.0}
_CASE = {}


@pytest.fixture(scope="module")
def gpu(tables):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from mitsuba_customization_amd import host
    ctx = host.MerlHip(0)
    ids = {(alpha, metal): ctx.ggx(alpha, *ggx.METALS[metal]) for alpha, metal in ggx.CASES}
    table = ctx.upload_merl(tables("ggx_tab", 0))
    yield dict(ctx=ctx, ids=ids, table=table, host=host)
    ctx.close()


def to_dev(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def case_data(oracle, alpha, metal):
    """Inputs of a case (g signed standard normal, h = |standard normal|, both NaN / inf on the units eval masks) and the reference
    sums; computed once, read-only."""
    key = (alpha, metal)
    if key not in _CASE:
        wi, wo, _, special = ggx.case_units(oracle, alpha, metal)
        rng = np.random.default_rng(1000 + ggx.CASES.index(key))
        g = rng.standard_normal((len(wi), 3)).astype(np.float32)
        h = np.abs(rng.standard_normal((len(wi), 3))).astype(np.float32)
        dead = ~gref.live_units(wi, wo)
        assert dead[special].all()
        odd = (np.arange(dead.sum()) % 2 == 1)[:, None]
        g[dead] = np.where(odd, np.nan, np.inf); h[dead] = np.where(odd, np.inf, np.nan)
        al, eta, k = ggx.f32_params(alpha, metal)
        J = gref.jacobian(al, eta, k, wi, wo)
        d = dict(wi=wi, wo=wo, g=g, h=h, J=J, k=k, sums=gref.sums(J, g, h))
        for v in list(d.values()) + list(d["sums"]):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASE[key] = d
    return _CASE[key]


def fresh(device=True):
    """grad of zeros, and normal of zeros with the sentinel in the entries that couple two channels."""
    G, N = np.zeros(7), np.where(CROSS, SENTINEL, 0.0)
    return to_dev(G, N) if device else [G, N]


def bits(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def check(G, N, sums, tag, rel=REL):
    """G [7] and N [7, 7] (numpy) against the reference sums; returns the worst |error| / S of each."""
    R, S, R2, S2 = sums
    assert np.isfinite(G).all() and np.isfinite(N).all(), tag
    assert np.array_equal(N[CROSS], np.full(CROSS.sum(), SENTINEL)), f"{tag}: an entry that couples two channels was written"
    assert np.array_equal(bits(N), bits(N.T)), f"{tag}: normal is not symmetric bit for bit"
    eg = np.abs(G - R) / np.maximum(S, 1e-300)
    en = np.abs(N - R2)[~CROSS] / np.maximum(S2[~CROSS], 1e-300)
    print(f"{tag}: worst |G - R| / S = {eg.max():.2e}, worst |N - R2| / S2 = {en.max():.2e}")
    assert (np.abs(G - R) <= rel * S).all(), (tag, eg)
    assert (np.abs(N - R2)[~CROSS] <= rel * S2[~CROSS]).all(), (tag, en)
    return eg.max(), en.max()


def run(gpu, mid, wi, wo, g, h=None, normal=True):
    """One device-pointer call on fresh outputs -> numpy."""
    G, N = fresh()
    if normal:
        gpu["ctx"].ggx_grad(wi, wo, g, mid, curvature=h, normal=True, out=(G, N))
        return G.cpu().numpy(), N.cpu().numpy()
    gpu["ctx"].ggx_grad(wi, wo, g, mid, out=G)
    return G.cpu().numpy(), None


@pytest.mark.parametrize("case", ggx.CASES, ids=CASE_IDS)
def test_parity_with_central_differences(gpu, oracle, case):
    d = case_data(oracle, *case)
    G, N = run(gpu, gpu["ids"][case], *to_dev(d["wi"], d["wo"], d["g"], d["h"]))
    eg, en = check(G, N, d["sums"], ggx.case_id(case))
    WORST["grad"], WORST["normal"] = max(WORST["grad"], eg), max(WORST["normal"], en)
    print(f"worst so far: grad {WORST['grad']:.2e}, normal {WORST['normal']:.2e}")
    S = d["sums"][1]
    for c in range(3):
        if d["k"][c] == 0.0:                                 # F is even in k
            assert abs(G[4 + c]) <= 1e-9 * S[1 + c], (c, G[4 + c], S[1 + c])


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 257))
def test_shapes_around_a_wave_and_a_block(gpu, oracle, n):
    case = (0.3, "gold")
    d = case_data(oracle, *case)
    # the first units of the random block and the last of the targeted one (dead units with NaN / inf in g and h among them)
    sel = np.r_[0:(n + 1) // 2, len(d["wi"]) - n // 2:len(d["wi"])]
    assert len(sel) == n
    G, N = run(gpu, gpu["ids"][case], *to_dev(d["wi"][sel], d["wo"][sel], d["g"][sel], d["h"][sel]))
    check(G, N, gref.sums(d["J"][sel], d["g"][sel], d["h"][sel]), f"n={n}")


def test_more_units_than_one_round_of_the_grid(gpu, oracle):
    case = (0.3, "gold")
    d = case_data(oracle, *case)
    n, m = (1 << 20) + 37, len(d["wi"])
    copies, rest = divmod(n, m)
    assert n > 256 * 3 * gpu["ctx"].compute_units              # the grid-stride loop runs more than once
    tiled = [np.concatenate([np.tile(d[key], (copies, 1)), d[key][:rest]]) for key in ("wi", "wo", "g", "h")]
    assert len(tiled[0]) == n
    part = gref.sums(d["J"][:rest], d["g"][:rest], d["h"][:rest])
    sums = tuple(copies * full + p for full, p in zip(d["sums"], part))
    G, N = run(gpu, gpu["ids"][case], *to_dev(*tiled))
    check(G, N, sums, f"n={n}")


def test_accumulation_null_arguments_and_determinism(gpu, oracle):
    case = (0.05, "spread_k")
    d = case_data(oracle, *case)
    ctx, mid = gpu["ctx"], gpu["ids"][case]
    wi, wo, g, h = to_dev(d["wi"], d["wo"], d["g"], d["h"])
    S, S2 = d["sums"][1], d["sums"][3]
    G1, N1 = run(gpu, mid, wi, wo, g, h)
    # a second call adds to the first
    G, N = fresh()
    ctx.ggx_grad(wi, wo, g, mid, curvature=h, normal=True, out=(G, N))
    ctx.ggx_grad(wi, wo, g, mid, curvature=h, normal=True, out=(G, N))
    G2, N2 = G.cpu().numpy(), N.cpu().numpy()
    assert (np.abs(G2 - 2.0 * G1) <= 1e-14 * S).all()
    assert (np.abs(N2 - 2.0 * N1)[~CROSS] <= 1e-14 * S2[~CROSS]).all() and np.array_equal(N2[CROSS], N1[CROSS])
    # two device-pointer calls: the same bits
    G3, N3 = run(gpu, mid, wi, wo, g, h)
    assert np.array_equal(bits(G3), bits(G1)) and np.array_equal(bits(N3), bits(N1))
    # normal = NULL: the same grad_params bits
    G4, _ = run(gpu, mid, wi, wo, g, normal=False)
    assert np.array_equal(bits(G4), bits(G1))
    # curv_rgb = NULL is an array of ones (live units; the dead ones carry NaN / inf either way)
    import torch
    ones = torch.where(torch.isfinite(h), torch.ones_like(h), h)
    G5, N5 = run(gpu, mid, wi, wo, g, ones)
    G6, N6 = run(gpu, mid, wi, wo, g, None)
    assert np.array_equal(bits(G5), bits(G6)) and np.array_equal(bits(N5), bits(N6)) and np.array_equal(bits(G5), bits(G1))
    assert np.isfinite(N6).all() and (np.diag(N6) > 0).all()


def test_host_arrays_in_chunks_and_pointer_mix(gpu, oracle):
    case = (0.3, "aluminium")
    d = case_data(oracle, *case)
    ctx, mid, host = gpu["ctx"], gpu["ids"][case], gpu["host"]
    n = 3 * 4096 + 5
    sel = np.r_[0:n - 300, len(d["wi"]) - 300:len(d["wi"])]
    arrs = [np.ascontiguousarray(d[key][sel]) for key in ("wi", "wo", "g", "h")]
    sums = gref.sums(d["J"][sel], arrs[2], arrs[3])
    Gd, Nd = run(gpu, mid, *to_dev(*arrs))
    check(Gd, Nd, sums, "device pointers")
    chunk = ctx.get_option(host.OPT_HOST_CHUNK)
    ctx.set_option(host.OPT_HOST_CHUNK, 4096)
    try:
        Gh, Nh = fresh(device=False)
        ctx.ggx_grad(*arrs[:3], mid, curvature=arrs[3], normal=True, out=(Gh, Nh))
        Gh2 = ctx.ggx_grad(*arrs[:3], mid)
    finally:
        ctx.set_option(host.OPT_HOST_CHUNK, chunk)
    check(Gh, Nh, sums, "host arrays")
    assert (np.abs(Gh - Gd) <= 1e-12 * sums[1]).all() and (np.abs(Nh - Nd)[~CROSS] <= 1e-12 * sums[3][~CROSS]).all()
    assert (np.abs(Gh2 - Gd) <= 1e-12 * sums[1]).all()
    with pytest.raises(host.MerlHipError) as e:
        ctx.ggx_grad(to_dev(arrs[0])[0], arrs[1], arrs[2], mid)
    assert e.value.status == host.ERR_POINTER_MIX


def test_errors_and_memory_report(gpu, oracle):
    case = (0.3, "gold")
    d = case_data(oracle, *case)
    ctx, host = gpu["ctx"], gpu["host"]
    n = 64
    wi, wo, g = to_dev(d["wi"][:n], d["wo"][:n], d["g"][:n])
    released = ctx.ggx(0.2, (1.0, 1.1, 1.2), (2.0, 2.1, 2.2))
    ctx.release_material(released)
    for mid in (gpu["table"], released, ctx.material_count() + 5, -1):
        with pytest.raises(host.MerlHipError) as e:
            ctx.ggx_grad(wi, wo, g, mid)
        assert e.value.status == host.ERR_MATERIAL, mid
    G, N = fresh()
    before = (G.clone(), N.clone())
    call = ctx._lib.mrl_ggx_grad_batch
    mid = gpu["ids"][case]
    assert call(ctx._ctx, wi.data_ptr(), wo.data_ptr(), None, None, mid, n, G.data_ptr(), N.data_ptr()) == host.ERR_INVALID
    assert call(ctx._ctx, wi.data_ptr(), wo.data_ptr(), g.data_ptr(), None, mid, n, None, N.data_ptr()) == host.ERR_INVALID
    assert call(ctx._ctx, wi.data_ptr(), wo.data_ptr(), g.data_ptr(), None, mid, 0, G.data_ptr(), N.data_ptr()) == 0
    ctx.synchronize()
    assert np.array_equal(bits(G), bits(before[0])) and np.array_equal(bits(N), bits(before[1]))
    # the rows of partial sums are workspace of the context: 256 B per block, 3 blocks per compute unit, + 56 doubles
    ctx.ggx_grad(wi, wo, g, mid)
    assert ctx.memory_info()["workspace_bytes"] >= 3 * ctx.compute_units * 256 + 56 * 8


def test_fit_ggx_recovers_a_material_from_the_devices_own_eval(gpu):
    from mitsuba_customization_amd import fit
    ctx = gpu["ctx"]
    n = 1 << 16
    wi, wo, _ = ctx.generate_pairs(0xF17, 0, n)
    eta, k = (np.array(x, np.float64) for x in ggx.METALS["gold"])
    alpha = 0.1
    truth = ctx.ggx(alpha, eta, k)
    y = ctx.eval(wi, wo, material=truth)
    ctx.release_material(truth)
    a, e, kk, history = fit.fit_ggx(ctx, wi, wo, y, (0.3, eta * 1.5, k * 0.7), 30)
    rel = max(abs(a - alpha) / alpha, np.abs(e / eta - 1).max(), np.abs(kk / k - 1).max())
    print(f"fit_ggx: recovered to {rel:.2e} relative (f32 measurements); residual {history[0]:.3e} -> {history[-1]:.3e}")
    assert rel <= 1e-3, (a, e, kk)
    assert len(history) == 31 and all(b <= a_ for a_, b in zip(history, history[1:]))
