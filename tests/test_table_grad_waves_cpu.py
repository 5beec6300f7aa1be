"""The inputs of tests/test_gpu_table_grad_waves.py, checked without a GPU and on the reference alone: the pool holds the interior
units and the full cells the layouts draw on, every layout's chosen wave has the make-up its name stands for (from ref.cell_index and
ref.guard only), and ref.adjoint stays the transpose of the CPU oracle's eval on tables with an axis of one texel."""
import numpy as np
import pytest

from tests import table_grad_reference as ref

DIMS = (7, 5, 12)
THIN = ((1, 1, 1), (1, 7, 1), (5, 1, 2), (2, 3, 1))
PARAMS = (ref.HALF_DIFF, ref.STANDARD, ref.STANDARD_FULL)
SCALE = (0.7, 1.3, 2.1)


@pytest.fixture(scope="module")
def pool(oracle):
    wi, wo, _ = oracle.generate_pairs(0x5EED, 0, 1 << 16)
    return np.ascontiguousarray(wi, np.float32), np.ascontiguousarray(wo, np.float32)


@pytest.mark.parametrize("param", PARAMS)
@pytest.mark.parametrize("center", (False, True))
def test_pool_holds_interior_units_and_full_cells(pool, param, center):
    wi, wo = pool
    inside = ref.interior(wi, wo, DIMS, param, center)
    cells = ref.cell_index(wi[inside], wo[inside], DIMS, param, center)
    full = int((np.bincount(cells, minlength=int(np.prod(DIMS))) >= 64).sum())
    print(f"param {param} center {center}: {int(inside.sum())} interior units, {full} cells with at least 64 of them")
    assert inside.sum() >= 40000
    assert full >= 8
    assert (cells >= 0).all() and ref.guard(wi[inside], wo[inside]).all()
    # what interior promises: the split coordinate is at least 0.05 of a cell from an integer, so every corner weight of the
    # trilinear lookup is 0 (a clamped end) or at least 0.05^3, and the nearest lookup's bin is not in doubt
    x0, x1, x2, _ = ref.table_coords(wi[inside], wo[inside], DIMS, param)
    for x in (x0, x1, x2):
        y = x - (0.5 if center else 0.0)
        assert (np.abs(y - np.round(y)) >= 0.05 - 1e-12).all()


@pytest.mark.parametrize("dims", THIN)
@pytest.mark.parametrize("param", PARAMS)
def test_thin_tables_are_reached_on_every_texel(pool, dims, param):
    """What the device test of thin tables relies on: every cell holds a wave of interior units of the pool, and the 4096 units it
    runs put weight on every texel under each lookup, so every fold rule of an axis of one or two texels carries weight."""
    wi, wo = pool
    inside = ref.interior(wi, wo, dims, param, False)
    cells = ref.cell_index(wi[inside], wo[inside], dims, param, False)
    assert (np.bincount(cells, minlength=int(np.prod(dims))) >= 64).all()
    for trilinear, center in ((True, False), (True, True), (False, False)):
        swi, swo = ref.sequence(wi, wo, dims, param, center, length=4096)
        _, S = ref.adjoint(swi, swo, np.ones((4096, 3), np.float32), dims, param=param, trilinear=trilinear, center=center)
        assert (S > 0).all(), (trilinear, center)


def test_kill_makes_each_kind_of_dead_unit_and_poisoned_marks_them(pool):
    wi, wo = pool[0][:20].copy(), pool[1][:20].copy()
    assert ref.guard(wi, wo).all()
    ref.kill(wi, wo, [1, 3, 5, 7, 9, 11])
    dead = ~ref.guard(wi, wo)
    assert np.array_equal(np.nonzero(dead)[0], [1, 3, 5, 7, 9, 11])
    assert wi[1, 2] < 0 and wo[3, 2] < 0 and np.isnan(wi[5]).any() and np.isinf(wo[7]).any() and not wi[9].any() and wi[11, 2] < 0
    g = ref.poisoned(np.ones((20, 3), np.float32), wi, wo)
    assert np.isnan(g[[1, 5, 9]]).all() and np.isinf(g[[3, 7, 11]]).all() and (g[~dead] == 1).all()
    swi, swo = ref.sequence(pool[0], pool[1], DIMS, length=257)
    dead = ~ref.guard(swi, swo)
    assert np.array_equal(np.nonzero(dead)[0], np.arange(8, 257, 9))
    assert ref.interior(swi, swo, DIMS)[~dead].all()


def _makeup(wi, wo, param, center, wave):
    """Of the chosen wave, from the reference's cells and guard alone: the dead lanes, the first live lane, the lanes that share its
    cell, and per cell with more than one lane its members in the low and in the high half."""
    at = slice(ref.WAVE * wave, ref.WAVE * (wave + 1))
    cell = ref.cell_index(wi[at], wo[at], DIMS, param, center)
    live = ref.guard(wi[at], wo[at])
    assert np.array_equal(cell >= 0, live)
    if not live.any():
        return ~live, None, np.zeros(0, int), {}
    first = int(np.nonzero(live)[0][0])
    sharers = np.nonzero(cell == cell[first])[0]
    groups = {}
    for c in np.unique(cell[live]):
        lanes = np.nonzero(cell == c)[0]
        if len(lanes) > 1:
            groups[int(c)] = (int((lanes < 32).sum()), int((lanes >= 32).sum()))
    return ~live, first, sharers, groups


# name: dead lanes, first live lane, lanes sharing its cell, (low, high) members of every cell with more than one lane, ordered
EXPECT = {
    "a": ([], 0, list(range(64)), [(32, 32)]),
    "b": ([], 0, [0, 1, 2, 3], [(0, 32), (4, 0)]),
    "c": (list(range(30)), 30, [30, 31, 32, 33], [(2, 2)]),
    "d": ([], 0, [0, 5, 11], [(3, 0), (8, 32)]),
    "e": ([], 0, [0, 5, 11, 17], [(4, 0), (8, 32)]),
    "f": (list(range(2, 48, 3)), 0, [l for l in range(48) if l % 3 != 2], [(22, 10)]),
    "g": (list(range(64)), None, [], []),
    "h": (list(range(1, 64, 2)), 0, [0], []),
    "i": (list(range(0, 64, 2)), 1, [1], []),
    "j": ([], 0, list(range(0, 64, 2)), [(16, 16), (16, 16)]),
}


@pytest.mark.parametrize("param", PARAMS)
@pytest.mark.parametrize("center", (False, True))
@pytest.mark.parametrize("wave", (1, 4))
def test_layouts_have_the_make_up_they_are_named_for(pool, param, center, wave):
    layouts = ref.wave_layouts(pool[0], pool[1], DIMS, param, center, wave)
    assert tuple(layouts) == ref.LAYOUT_NAMES == tuple(EXPECT)
    for name, (wi, wo) in layouts.items():
        assert wi.shape == wo.shape == (ref.LAYOUT_UNITS, 3) and wi.dtype == wo.dtype == np.float32
        dead, first, sharers, groups = _makeup(wi, wo, param, center, wave)
        want_dead, want_first, want_sharers, want_groups = EXPECT[name]
        assert np.array_equal(np.nonzero(dead)[0], want_dead), name
        assert first == want_first and np.array_equal(sharers, want_sharers), name
        assert sorted(groups.values()) == sorted(want_groups), (name, groups)
        # the auto rule of the kernel (at least 4 lanes on the first live lane's cell) takes the path the layout is meant for
        if name in "abcefj":
            assert len(sharers) >= 4, name
        if name in "dhi":
            assert len(sharers) < 4, name
        # every live unit is interior, the other waves are all live, and no unit is used twice
        live = ref.guard(wi, wo)
        assert ref.interior(wi, wo, DIMS, param, center)[live].all(), name
        others = np.ones(ref.LAYOUT_UNITS, bool); others[ref.WAVE * wave: ref.WAVE * (wave + 1)] = False
        assert live[others].all(), name
        both = np.concatenate([wi[live], wo[live]], 1)
        assert len(np.unique(both, axis=0)) == live.sum(), name


@pytest.mark.parametrize("dims", THIN)
@pytest.mark.parametrize("param", PARAMS)
@pytest.mark.parametrize("center", (False, True))
def test_reference_is_the_transpose_of_the_oracle_on_thin_tables(oracle, dims, param, center):
    rng = np.random.default_rng(100 * param + 10 * sum(dims) + center)
    n = 20000
    wi, wo, _ = oracle.generate_pairs(0xADD0 + param, 0, n)
    wi = np.array(wi, np.float32); wo = np.array(wo, np.float32)
    wo[::97, 2] *= -1.0
    opts = oracle.make_opts(lookup=1, node=int(center), cosine=0, negative=oracle.NEGATIVE_KEEP)
    kw = dict(param=param, trilinear=True, center=center, cosine=True, scale=SCALE)
    worst = 0.0
    for _ in range(3):
        T = rng.standard_normal((3,) + tuple(dims)) + 0.25
        g = rng.standard_normal((n, 3)).astype(np.float32)
        R, S = ref.adjoint(wi, wo, g, dims, **kw)
        ev = oracle.OracleTable(T, SCALE, param).eval(wi, wo, opts).astype(np.float64)
        lhs, rhs, terms = float((ev * g.astype(np.float64)).sum()), float((T * R).sum()), float((np.abs(T) * S).sum())
        worst = max(worst, abs(lhs - rhs) / terms)
        assert terms > 0 and abs(lhs - rhs) <= 1e-6 * terms, (lhs, rhs, terms)
    # texel by texel on one-hot tables: with an axis of one texel both corners of that axis fold onto the same texel
    assert (S > 0).all()
    for t in range(int(np.prod(dims))):
        c = t % 3
        T = np.zeros((3,) + tuple(dims)); T[c].flat[t] = 1.0
        ev = oracle.OracleTable(T, SCALE, param).eval(wi, wo, opts).astype(np.float64)
        lhs = float((ev * g.astype(np.float64)).sum())
        worst = max(worst, abs(lhs - R[c].flat[t]) / S[c].flat[t])
        assert abs(lhs - R[c].flat[t]) <= 1e-6 * S[c].flat[t], (t, lhs, R[c].flat[t], S[c].flat[t])
    print(f"dims {dims} param {param} center {center}: worst |lhs - rhs| / terms = {worst:.3e}")
