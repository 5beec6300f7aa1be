"""mrl_table_grad_batch where its intra-wave machinery can go wrong: n around half a pair, a wave, a block and one round of the
grid; waves of a stated make-up (merged groups with dead lanes, in one half, across the halves, 3 against 4 sharers, dead waves);
tables with an axis of one texel; hard directions; the workspace between tables of different dims; host arrays at chunk edges.

The units are interior units of one pool (ref.interior: at least 0.05 of a cell from every cell face, theta_h and theta_d above
0.02 rad), so the kernel and the numpy reference cannot disagree on a cell and the bar of tests/test_gpu_table_grad.py holds per
texel even where one unit reaches it: |G - R| <= 1e-6 S, G == 0 where S == 0.  tests/test_table_grad_waves_cpu.py checks the
inputs (pool, layouts, thin-table reference) without a GPU.

Measured on MI355X (worst over the cases of each test, to one digit where the order of the atomics moves it from run to
run; differences in units of S):
  sizes 1 .. 257         |G - R| / S 4e-16 (trilinear), 2e-16 (nearest); variant against variant 4e-16
  one round + 37         |G - R| / S 5e-14 (n = 524,325: 513 tiles of the sequence summed per slot)
  n = 257, standard      |G - R| / S 4e-16
  wave compositions      |G - R| / S 5e-16; variant against variant 5e-16; two runs of variant 0 3e-16
  thin tables            |G - R| / S 1.4e-11 (trilinear: one Float weight of 4096 an ulp apart), 3e-16 (nearest)
  hard directions        g = |normal| / Float(wo.z), every family a sixth of the sums: mass 5.2e-10 (trilinear), 3e-15 (nearest)
                         of the sum, transpose 1.3e-8 of <T, G>; the reference's own, on the CPU: 5.2e-10, 5e-15, and 5.3e-8
                         against the oracle.  g = |normal|, a few scaled units carry the sums: mass 5.6e-9, 1.4e-15, transpose 2.0e-8
  workspace reuse        against a fresh context 3e-16; |G - R| / S 3e-16
  host arrays            |G - R| / S 4e-16; against device pointers 3e-16
Interior units keep the Float weights away from the cell edges where the 2.8e-7 of DESIGN.md 5g comes from: what is left is f64
rounding.
"""
import functools

import numpy as np
import pytest

from tests import table_grad_reference as ref
from tests.test_gpu_table_grad import SCALE, _check, _ctx, _device, _shape_table

pytestmark = pytest.mark.gpu

DIMS = (7, 5, 12)
THIN = ((1, 1, 1), (1, 7, 1), (5, 1, 2), (2, 3, 1))
PARAMS = (ref.HALF_DIFF, ref.STANDARD, ref.STANDARD_FULL)
LOOKUPS = ((1, 0), (1, 1), (0, 0))                            # (MRL_OPT_LOOKUP, MRL_OPT_NODE)
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257)
BASE = 1021                                                   # the tiled sequence: odd, so every tile starts on another lane


@functools.lru_cache(maxsize=None)
def _pool():
    from oracle import binding
    wi, wo, _ = binding.generate_pairs(0x5EED, 0, 1 << 16)
    wi = np.ascontiguousarray(wi, np.float32); wo = np.ascontiguousarray(wo, np.float32)
    wi.setflags(write=False); wo.setflags(write=False)
    return wi, wo


@functools.lru_cache(maxsize=None)
def _sequence(dims, param, center, length):
    """(wi, wo, g) of ref.sequence: interior pool units, every 9th dead with a NaN or inf gradient.  Shared, read-only."""
    wi, wo = ref.sequence(*_pool(), dims, param, center, length)
    g = ref.poisoned(np.random.default_rng(length).standard_normal((length, 3)), wi, wo)
    for a in (wi, wo, g):
        a.setflags(write=False)
    return wi, wo, g


def _adjoint(wi, wo, g, dims, param, lookup, node):
    return ref.adjoint(wi, wo, g, dims, param=param, trilinear=bool(lookup), center=bool(node), scale=SCALE)


def _grad(gpu, mid, wi, wo, g):
    return gpu.table_grad(*_device(np.array(wi), np.array(wo), np.array(g)), material=mid).cpu().numpy()      # copies: the inputs are shared


def _same(a, b, S, what, worst):
    """|a - b| <= 1e-12 S; keeps the worst ratio seen in worst[0]."""
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst[0] = max(worst[0], float(np.max(np.where(S > 0, d / S, 0.0))))
    assert (d <= 1e-12 * S).all(), what


def _variants_agree(gpu, mid, wi, wo, g, R, S, what, worst, rerun=False):
    """The four MRL_OPT_TABLE_GRAD_KERNEL variants against the reference and against each other (and variant 0 run twice)."""
    from mitsuba_customization_amd import host
    got = []
    for variant in (0, 1, 2, 3) + ((0,) if rerun else ()):
        gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
        got.append(_grad(gpu, mid, wi, wo, g))
        _check(got[-1], R, S, f"{what} variant {variant}")
    for v in (1, 2, 3):
        _same(got[0], got[v], S, f"{what}: variant {v} against 0", worst)
    gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)
    return got


@pytest.mark.parametrize("lookup,node", LOOKUPS)
def test_sizes_around_a_pair_a_wave_a_block_and_a_round(lookup, node):
    wi, wo, g = _sequence(DIMS, ref.HALF_DIFF, bool(node), BASE)
    worst = [0.0]
    with _ctx(lookup, node) as gpu:
        mid = _shape_table(gpu, DIMS)
        for n in SIZES:
            R, S = _adjoint(wi[:n], wo[:n], g[:n], DIMS, ref.HALF_DIFF, lookup, node)
            _variants_agree(gpu, mid, wi[:n], wo[:n], g[:n], R, S, f"n {n} lookup {lookup} node {node}", worst)
        print(f"variants: worst difference {worst[0]:.3e} S")
        # more units than one round of the grid: rounds > 1, the last one ragged, the barriers inside the loop.  The sequence tiled;
        # A^T is linear, so the reference is q times the sequence's plus the remainder's
        n = 256 * 8 * gpu.compute_units + 37
        q, rem = divmod(n, BASE)
        Rb, Sb = _adjoint(wi, wo, g, DIMS, ref.HALF_DIFF, lookup, node)
        Rr, Sr = _adjoint(wi[:rem], wo[:rem], g[:rem], DIMS, ref.HALF_DIFF, lookup, node)
        tile = lambda a: np.concatenate([np.tile(a, (q, 1)), a[:rem]])
        G = _grad(gpu, mid, tile(wi), tile(wo), tile(g))
        _check(G, q * Rb + Rr, q * Sb + Sr, f"n {n} = one round + 37, lookup {lookup} node {node}")


@pytest.mark.parametrize("param", (ref.STANDARD, ref.STANDARD_FULL))
def test_a_ragged_second_block_on_the_standard_parameterisations(param):
    for node in (0, 1):
        wi, wo, g = _sequence(DIMS, param, bool(node), BASE)
        R, S = _adjoint(wi[:257], wo[:257], g[:257], DIMS, param, 1, node)
        with _ctx(1, node) as gpu:
            mid = _shape_table(gpu, DIMS, param)
            _check(_grad(gpu, mid, wi[:257], wo[:257], g[:257]), R, S, f"n 257 param {param} node {node}")


@pytest.mark.parametrize("wave", (1, 4))                      # a wave among live ones; the only wave of the ragged last block
@pytest.mark.parametrize("lookup,node", LOOKUPS)
def test_wave_compositions(lookup, node, wave):
    layouts = ref.wave_layouts(*_pool(), DIMS, ref.HALF_DIFF, bool(node), wave)
    between, twice = [0.0], [0.0]
    with _ctx(lookup, node) as gpu:
        mid = _shape_table(gpu, DIMS)
        for k, (name, (wi, wo)) in enumerate(layouts.items()):
            g = ref.poisoned(np.random.default_rng(100 + k).standard_normal((len(wi), 3)), wi, wo)
            R, S = _adjoint(wi, wo, g, DIMS, ref.HALF_DIFF, lookup, node)
            got = _variants_agree(gpu, mid, wi, wo, g, R, S, f"layout {name} wave {wave} lookup {lookup} node {node}", between, rerun=True)
            _same(got[0], got[4], S, f"layout {name}: two runs of variant 0", twice)
    print(f"variants: worst difference {between[0]:.3e} S; two runs: {twice[0]:.3e} S")


@pytest.mark.parametrize("dims", THIN)
@pytest.mark.parametrize("param", PARAMS)
def test_thin_tables(dims, param):
    from mitsuba_customization_amd import host
    for lookup, node in LOOKUPS:
        wi, wo, g = _sequence(dims, param, bool(node), 4096)
        R, S = _adjoint(wi, wo, g, dims, param, lookup, node)
        assert (S > 0).all()                                  # every texel, so every fold rule of a 1- and 2-texel axis, carries weight
        with _ctx(lookup, node) as gpu:
            mid = _shape_table(gpu, dims, param)
            for variant in (0, 1, 2, 3) if dims in ((1, 1, 1), (2, 3, 1)) else (0,):
                gpu.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
                _check(_grad(gpu, mid, wi, wo, g), R, S, f"dims {dims} param {param} lookup {lookup} node {node} variant {variant}")


FAMILIES = ("theta_h -> 0", "theta_d -> 0", "grazing wi", "grazing wo", "near the normal", "scaled by 1e+-10")


@functools.lru_cache(maxsize=None)
def _hard():
    """(wi, wo, family, {weighting: g}) of the 6000 adversarial pairs that are live.  g > 0, so nothing cancels.  The cosine factor
    is the raw Float wo.z and the last family scales wo by 1e+-10, so with g = |normal| a handful of scaled units carry the sums
    and the other five families 2e-8 of them: "level" divides g by Float(wo.z), which gives every unit a mass of scale x |normal|
    and every family a sixth of the sums."""
    from tests.test_gpu_parity import _adversarial_pairs
    wi, wo = _adversarial_pairs(np.random.default_rng(5), 6000)
    family = np.minimum(np.arange(6000) // 1000, 5)
    live = ref.guard(wi, wo)                                   # a near-mirror wo may dip below the horizon: unit 782 does
    assert (~live).sum() == 1 and not live[782]
    wi, wo, family = np.ascontiguousarray(wi[live]), np.ascontiguousarray(wo[live]), family[live]
    plain = np.abs(np.random.default_rng(15).standard_normal((len(wi), 3)))
    g = {"plain": plain.astype(np.float32), "level": (plain / wo[:, 2:3].astype(np.float64)).astype(np.float32)}
    assert np.isfinite(g["level"]).all() and (g["level"] > 0).all()
    return wi, wo, family, g


def _mass(wo, g):
    """Per unit and channel, in f64 from the inputs: scale x Float(wo.z) x g."""
    return np.asarray(SCALE)[None, :] * wo[:, 2:3].astype(np.float64) * g.astype(np.float64)


@pytest.mark.parametrize("dims", (DIMS, (2, 3, 1)))
@pytest.mark.parametrize("param", PARAMS)
def test_hard_directions_keep_the_mass_and_the_transpose(dims, param):
    """theta_h -> 0, theta_d -> 0, grazing, near-normal and scaled by 1e+-10: which cell such a unit lands in is ill-posed, these
    two identities are not.  Mass: a unit's corner weights sum to 1 up to eight Float roundings, so per channel the texels of G
    sum to sum_u scale x Float(wo.z) x g.  Transpose: <eval(T), g> = <T, G> against the shipped forward kernel.  Under both
    weightings of _hard; under "level" every family carries at least 5 % of either sum and one unit about 1.7e-4 of it, 170 times
    the bar, so a unit dropped or doubled in any family shows in the mass, and one put into another cell in the transpose."""
    from mitsuba_customization_amd import host
    wi, wo, family, gs = _hard()
    T = np.random.default_rng(8).uniform(50.0, 150.0, (3,) + tuple(dims))
    level = _mass(wo, gs["level"])
    share = np.array([level[family == f].sum(0) / level.sum(0) for f in range(6)])
    assert (share >= 0.05).all() and (level / level.sum(0) <= 2e-3).all(), share
    for lookup, node in LOOKUPS:
        with _ctx(lookup, node) as gpu:
            gpu.set_option(host.OPT_KERNEL, 3)                 # the forward kernels that share the adjoint's transform
            mid = gpu.upload_table_param(T, param, SCALE)
            for name, g in gs.items():
                mass = _mass(wo, g).sum(0)
                dwi, dwo, dg = _device(wi, wo, g)
                G = gpu.table_grad(dwi, dwo, dg, material=mid).cpu().numpy()
                ev = gpu.eval(dwi, dwo, material=mid).cpu().numpy().astype(np.float64)
                total = G.sum((1, 2, 3))
                print(f"dims {dims} param {param} lookup {lookup} node {node} g {name}: mass ratio {np.max(np.abs(total - mass) / mass):.3e}", end="")
                assert np.isfinite(G).all() and (G >= 0).all()
                assert (np.abs(total - mass) <= 1e-6 * mass).all(), (name, total, mass)
                if lookup:                                    # a flipped bin between two nearest kernels is legitimate
                    lhs, rhs = float((ev * g.astype(np.float64)).sum()), float((T * G).sum())   # T, g > 0: <T, S> = <T, G>
                    print(f", transpose ratio {abs(lhs - rhs) / rhs:.3e}", end="")
                    assert abs(lhs - rhs) <= 2e-6 * rhs, (name, lhs, rhs)
                print()


def test_workspace_is_reused_between_tables_of_different_dims():
    big, small = (33, 17, 64), DIMS
    calls = ((big, 1), (small, 1), (big, 1), (small, 0))       # (dims, lookup)
    inputs = {(dims, lookup): _sequence(dims, ref.HALF_DIFF, False, 4096) for dims, lookup in calls}
    fresh = {}
    for dims, lookup in set(calls):
        with _ctx(lookup) as gpu:
            fresh[dims, lookup] = _grad(gpu, _shape_table(gpu, dims), *inputs[dims, lookup])
        R, S = _adjoint(*inputs[dims, lookup], dims, ref.HALF_DIFF, lookup, 0)
        _check(fresh[dims, lookup], R, S, f"fresh context, dims {dims} lookup {lookup}")
        fresh[dims, lookup] = (fresh[dims, lookup], S)
    from mitsuba_customization_amd import host
    worst, sizes = [0.0], []
    with _ctx() as gpu:
        mids = {dims: _shape_table(gpu, dims) for dims in (big, small)}
        for dims, lookup in calls:
            gpu.set_option(host.OPT_LOOKUP, lookup)
            G = _grad(gpu, mids[dims], *inputs[dims, lookup])
            _same(G, *fresh[dims, lookup], f"dims {dims} lookup {lookup} after another table", worst)
            sizes.append(gpu.memory_info()["workspace_bytes"])
    print(f"against a fresh context: worst difference {worst[0]:.3e} S; workspace bytes {sizes}")
    assert sizes[1] == sizes[2] == sizes[3] == sizes[0]


def test_host_arrays_at_chunk_edges():
    from mitsuba_customization_amd import host
    wi, wo, g = _sequence(DIMS, ref.HALF_DIFF, False, 8192)
    worst = [0.0]
    with _ctx() as gpu:
        gpu.set_option(host.OPT_HOST_CHUNK, 4096)
        mid = _shape_table(gpu, DIMS)
        for n in (4095, 4096, 4097, 8192):
            a, b, c = (np.ascontiguousarray(x[:n]) for x in (wi, wo, g))
            R, S = _adjoint(a, b, c, DIMS, ref.HALF_DIFF, 1, 0)
            Gh = gpu.table_grad(a, b, c, material=mid)
            _check(Gh, R, S, f"host arrays, n {n}")
            _same(Gh, _grad(gpu, mid, a, b, c), S, f"host arrays against device pointers, n {n}", worst)
            assert gpu.table_grad(a, b, c, material=mid, out=Gh) is Gh
            _check(Gh, 2 * R, 2 * S, f"host out= accumulates, n {n}")
    print(f"host against device pointers: worst difference {worst[0]:.3e} S")
