"""mrl_rgl_values_grad_batch / mrl_rgl_values_grad_queue (include/merl_hip_fit_rgl.h; MerlHip.rgl_values_grad / rgl_values_grad_queue):
the adjoint of eval in the measured values of RGB RGL materials on the GPU.  Reference: tests/rgl_values_grad_reference.py (autograd of
the torch-f64 restatement of the model).  Bars: per texel |G - R| <= 1e-6 S with the initial bits where S == 0; two forms of the same
sum agree within m_t 2^-52 S_t, m_t the number of terms of the texel (the bound of a reordered f64 sum of identical terms); the
adjoint identity |sum g . eval(R) - <R, G>| <= 2e-6 sum |g_c E_c| against the parent's eval.

The wave protocol (merl_grad_scatter.hpp, wave_scatter<L>) is run at every L — iso_theta1 (16 lanes per record), phi_only (32, the
phi pairing of slices), iso (32, the theta pairing), aniso (64) — on seven 256-unit patterns (_merge_inputs: the merge rule's
boundary kMergeMin and kMergeMin - 1, dead first lanes, a record with members in some lane groups only, four records interleaved),
and with records of S = 1, 2 and 4 in one merged wave of the id kernels, whole arrays and over a queue (_mixed_units).

Measured on MI355X, 14 files, worst |G - R| / S per file: iso 2.3e-9, iso_nojac 4.9e-9, iso_theta1 6.6e-10, iso_phi2
1.7e-9, aniso 1.2e-8, aniso_red2 1.1e-9, aniso_red4 4.7e-9, aniso_uneven 5.9e-10, iso_rows 9.5e-11, iso_cols 3.8e-10, iso_negative
1.9e-9, ggx_res32 6.5e-8 (the host-compiled function: 5.7e-8), phi_only 2.9e-9, phi_only_uneven 4.1e-9; the four kernel forms and
the host-array form within 0.36 of m_t 2^-52 S_t of each other on the seven patterns of the four files (iso 0.33, aniso 0.34,
iso_theta1 0.33, phi_only 0.36), a target of an id batch within 0.34 of its own call, a target of the three-shape batch or queue
within 0.33 (the worst of two runs: the order of the atomic adds varies); the three-shape batch against autograd 2.4e-8 (phi_only;
into the sentinel); the adjoint identity 1.0e-10 (iso) and 3.0e-10 (aniso) of sum |g E|; the file's 35 tests run in 4 s."""
import os
import re

import numpy as np
import pytest

from tests import rgl_values_grad_reference as vref

pytestmark = pytest.mark.gpu

SENTINEL = -4096.25            # larger than any sum of these tests: check() allows for the one rounding of an add into it
# lanes per gradient brick: 16 S.  iso_theta1 S = 1 (L = 16), phi_only S = 2 with the phi pairing of slices and iso S = 2 with the
# theta pairing (L = 32), aniso S = 4 (L = 64): the kernels compiled as MASK 1, 3, 5 and 15
WAVE_FILES = ["iso", "aniso", "iso_theta1", "phi_only"]
K_MERGE_MIN = int(re.search(r"constexpr int kMergeMin = (\d+);", open(os.path.join(
    vref.ROOT, "mitsuba_customization_amd", "csrc", "merl_grad_scatter.hpp")).read()).group(1))
_RECORDS = {}


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]


@pytest.fixture(scope="module")
def gpu():
    from mitsuba_customization_amd import host
    with host.MerlHip(0) as ctx:
        yield {"ctx": ctx, "host": host, "ids": {}}


def _mid(gpu, name):
    if name not in gpu["ids"]:
        gpu["ids"][name] = gpu["ctx"].upload_rgl(vref.case(name)["fields"])
    return gpu["ids"][name]


def _grad(gpu, mid, wi, wo, g, start=0.0, host_arrays=False, **kw):
    """one target, one material: G [n_phi, n_theta, 3, ny, nx] f64 numpy, added into an array that held `start`"""
    import torch
    ctx = gpu["ctx"]
    shape = ctx.rgl_values_shape(mid)
    if host_arrays:
        out = np.full(int(np.prod(shape)), start, np.float64)
        (G,) = ctx.rgl_values_grad(np.ascontiguousarray(wi), np.ascontiguousarray(wo), np.ascontiguousarray(g), [mid], material=mid, out=out, **kw)
        return G
    out = torch.full((int(np.prod(shape)),), start, dtype=torch.float64, device="cuda")
    (G,) = ctx.rgl_values_grad(*_dev(wi, wo, g), [mid], material=mid, out=out, **kw)
    return G.cpu().numpy()


def _same(a, b, m, S, what, worst):
    """two forms of one sum: |a - b| <= m_t 2^-52 S_t"""
    err = np.abs(a - b)
    bound = m * 2.0 ** -52 * S
    on = bound > 0
    worst[0] = max(worst[0], float((err[on] / bound[on]).max()) if on.any() else 0.0)
    assert (err <= bound).all(), (what, float(err.max()))


@pytest.mark.parametrize("name", vref.FILE_NAMES)
def test_every_file_against_the_reference(gpu, name):
    c = vref.case(name)
    mid = _mid(gpu, name)
    assert gpu["ctx"].rgl_values_shape(mid) == np.asarray(c["fields"]["rgb"]).shape
    vref.check(_grad(gpu, mid, c["wi"], c["wo"], c["g"], -0.0), c, -0.0, f"{name} device arrays")


@pytest.mark.parametrize("name", WAVE_FILES)
def test_wave_shapes(gpu, name):
    c = vref.case(name)
    mid = _mid(gpu, name)
    A = c["arrays"]
    live = np.flatnonzero(c["alive"])
    one_round = 256 * 2 * gpu["ctx"].compute_units
    for n in (1, 63, 64, 65, 255, 256, 257, one_round + 37):
        idx = np.resize(np.arange(len(c["wi"])), n)                # the case's units, tiled
        wi, wo, g = c["wi"][idx], c["wo"][idx], c["g"][idx]
        al = c["alive"][idx]
        q, rem = divmod(n, len(c["wi"]))
        if q:                                                      # A^T is linear: whole tiles of the case plus a rest
            Gr, Sr, _ = vref.values_grad(A, wi[:rem][al[:rem]], wo[:rem][al[:rem]], g[:rem][al[:rem]]) if rem else (0.0, 0.0, None)
            ref = dict(c, G=q * c["G"] + Gr, S=q * c["S"] + Sr)
        else:
            G, S, _ = vref.values_grad(A, wi[al], wo[al], g[al]) if al.any() else (np.zeros_like(c["G"]), np.zeros_like(c["S"]), None)
            ref = dict(c, G=G, S=S)
        vref.check(_grad(gpu, mid, wi, wo, g, -0.0), ref, -0.0, f"{name} n {n}")
    assert len(live)


def _by_record(c):
    """the live random units of a case grouped by gradient brick, most populated brick first: [[unit, ...], ...] and {unit: its
    place in that list}.  A unit's brick is read off the reference alone: the first texel of vref.weights names (bracket, cell)."""
    if c["name"] not in _RECORDS:
        live = np.flatnonzero(c["alive"][:vref.rref.N_RANDOM])
        _, cols, _ = vref.weights(c["arrays"], c["wi"][live], c["wo"][live])
        groups = {}
        for u, k in zip(live, cols[:, 0]):
            groups.setdefault(int(k), []).append(int(u))
        recs = sorted(groups.values(), key=lambda r: (-len(r), r[0]))
        _RECORDS[c["name"]] = (recs, {u: k for k, r in enumerate(recs) for u in r})
    return _RECORDS[c["name"]]


def _merge_inputs(c):
    """{pattern: (unit indices [256], g [256, 3])}, four waves of one block each.  all one identical pair; every wave half on one
    record and half scattered; 3 lanes of every wave on one record (below the merge rule), the rest scattered.  Then, with the units'
    records known (_by_record; units that share a record are different units where the record has that many, and every wave takes
    records of its own):
      * exactly kMergeMin lanes on the first live lane's record, no other lane on it: the boundary of the merge rule;
      * the first 5 lanes dead units of the fixed block with their dirty g, then 8 lanes on one record;
      * record X on lanes 0-3 and 32-35 only, Y on lanes 4-31 and 36-47, Z on lanes 48-63: with 16 lanes per record X has no member
        in lane groups 1 and 3, Y none in group 3, Z only in group 3; with 32, Z has none in group 0 — and the leader loop runs
        three times;
      * all 64 lanes on 4 records, interleaved lane by lane."""
    live = np.flatnonzero(c["alive"][:vref.rref.N_RANDOM])
    rng = np.random.default_rng(77)
    pick = lambda m: rng.choice(live, m, replace=False)
    g = rng.standard_normal((256, 3)).astype(np.float32)
    out = {}
    idx = np.full(256, live[3]); out["one pair"] = (idx, g)
    idx = pick(256); idx[np.arange(256) % 64 < 32] = live[5]; out["half on one record"] = (idx, g)
    idx = pick(256); idx[np.arange(256) % 64 < 3] = live[7]; out["3 lanes share"] = (idx, g)
    recs, rec_of = _by_record(c)
    assert len(recs) >= 16 and K_MERGE_MIN == 4
    dead = np.flatnonzero(~c["alive"])
    on = lambda k, m: np.resize(recs[k], m)                           # m units of record k (repeated where it holds fewer)

    def scattered(m, *avoid):
        pool = np.array([u for u in live if rec_of[u] not in avoid])
        return rng.choice(pool, m, replace=False)
    lanes = np.arange(64)
    at_min, dead_first, groups, four = (np.zeros(256, np.int64) for _ in range(4))
    g_dead = g.copy()
    for w in range(4):
        wave = slice(64 * w, 64 * w + 64)
        at_min[wave] = np.r_[on(w, K_MERGE_MIN), scattered(64 - K_MERGE_MIN, w)]
        dead_first[wave] = np.r_[dead[(5 * w + np.arange(5)) % len(dead)], on(4 + w, 8), scattered(51, 4 + w)]
        g_dead[64 * w:64 * w + 5] = c["g"][dead_first[64 * w:64 * w + 5]]
        x, y, z = w, 4 + w, 8 + w
        groups[wave] = np.where((lanes % 32) < 4, on(x, 64), np.where(lanes < 48, on(y, 64), on(z, 64)))
        four[wave] = np.stack([on(4 * w + q, 16) for q in range(4)], -1).reshape(-1)
    assert not np.isfinite(g_dead[~c["alive"][dead_first]]).any() and (~c["alive"][dead_first]).sum() == 20
    for w in range(4):                                               # the patterns are what they are said to be
        first = np.array([rec_of[u] for u in at_min[64 * w:64 * w + 64]])
        assert (first == first[0]).sum() == K_MERGE_MIN and (first[:K_MERGE_MIN] == first[0]).all()
        assert len({rec_of[u] for u in four[64 * w:64 * w + 64]}) == 4
    out[f"{K_MERGE_MIN} lanes share"] = (at_min, g)
    out["5 dead lanes first"] = (dead_first, g_dead)
    out["lane groups 0 and 2"] = (groups, g)
    out["4 records interleaved"] = (four, g)
    return out


@pytest.mark.parametrize("name", WAVE_FILES)
def test_merge_paths_on_every_kernel_variant_and_host_arrays(gpu, name):
    c = vref.case(name)
    ctx, host = gpu["ctx"], gpu["host"]
    mid = _mid(gpu, name)
    worst = [0.0]
    try:
        for pattern, (idx, g) in _merge_inputs(c).items():
            wi, wo, al = c["wi"][idx], c["wo"][idx], c["alive"][idx]
            G, S, _ = vref.values_grad(c["arrays"], wi[al], wo[al], g[al])      # the reference leaves the dead units out
            m = vref.term_counts(c["arrays"], wi[al], wo[al], g[al])
            ref = dict(c, G=G, S=S)
            got = []
            for variant in (0, 1, 2, 3):
                ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
                got.append(_grad(gpu, mid, wi, wo, g))
                vref.check(got[-1], ref, 0.0, f"{name} {pattern} variant {variant}")
            ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)
            got.append(_grad(gpu, mid, wi, wo, g, host_arrays=True))
            vref.check(got[-1], ref, 0.0, f"{name} {pattern} host arrays")
            for k in range(1, len(got)):
                _same(got[0], got[k], m, S, f"{name} {pattern}: form {k} against variant 0", worst)
    finally:
        ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)
    print(f"{name}: forms of one sum differ by at most {worst[0]:.3f} of m_t 2^-52 S_t")


def test_material_ids_with_stray_ids_and_a_sentinel(gpu):
    import torch
    ctx, host = gpu["ctx"], gpu["host"]
    a, b = vref.case("iso"), vref.case("aniso")
    ida, idb = _mid(gpu, "iso"), _mid(gpu, "aniso")
    other_rgl = _mid(gpu, "iso_phi2")
    table = ctx.upload_table(np.ones((3, 4, 3, 5)), (1.0, 1.0, 1.0))
    ggx = ctx.ggx(0.2, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2))
    released = ctx.upload_table(np.ones((3, 4, 3, 5)), (1.0, 1.0, 1.0)); ctx.release_material(released)
    strays = [other_rgl, table, ggx, released, -1, ctx.material_count() + 7]
    n = len(a["wi"])
    assert len(b["wi"]) == n
    rng = np.random.default_rng(5)
    role = rng.integers(0, 2 + len(strays), n)                     # 0: iso's unit, 1: aniso's, else a stray id
    wi = np.where((role == 1)[:, None], b["wi"], a["wi"]); wo = np.where((role == 1)[:, None], b["wo"], a["wo"])
    g = np.where((role == 1)[:, None], b["g"], a["g"]).astype(np.float32)
    g[role >= 2] = np.nan                                          # non-target units carry NaN
    mat = np.array([ida, idb] + strays, np.int32)[role]
    shapes = [ctx.rgl_values_shape(ida), ctx.rgl_values_shape(idb)]
    offsets = host.rgl_values_grad_layout(shapes)
    worst = [0.0]
    try:
        for variant in (0, 1, 2, 3):
            ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
            out = torch.full((offsets[-1],), SENTINEL, dtype=torch.float64, device="cuda")
            views = ctx.rgl_values_grad(*_dev(wi, wo, g), [ida, idb], mat=_dev(mat)[0], out=out)
            clean = ctx.rgl_values_grad(*_dev(wi, wo, g), [ida, idb], mat=_dev(mat)[0])          # from zeros: compared with the targets' own calls
            for k, (c, mid) in enumerate(((a, ida), (b, idb))):
                sel = role == k
                al = c["alive"] & sel
                G, S, _ = vref.values_grad(c["arrays"], c["wi"][al], c["wo"][al], c["g"][al])
                vref.check(views[k].cpu().numpy(), dict(c, G=G, S=S), SENTINEL, f"ids variant {variant} target {k}")
                own = _grad(gpu, mid, c["wi"][sel], c["wo"][sel], c["g"][sel])
                _same(clean[k].cpu().numpy(), own, vref.term_counts(c["arrays"], c["wi"][al], c["wo"][al], c["g"][al]), S,
                      f"ids variant {variant} target {k} against its own call", worst)
    finally:
        ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)
    print(f"ids: a target differs from its own single-material call by at most {worst[0]:.3f} of m_t 2^-52 S_t")


def _mixed_units(gpu):
    """one batch over three targets of different bracket shapes — iso_theta1 (S = 1), phi_only (S = 2), aniso (S = 4) — and stray ids:
    (cases, ids, role [n], unit [n], mat [n], wi, wo, g).  role 0 / 1 / 2: a unit of that target's case; 3 ..: a stray id (another
    RGL file, a table, a GGX material, a released id, -1, an id past the count) on a unit of the first case, with g = NaN.
      block 1 (4 waves): wave w starts with w dead units, then 6 units of one iso_theta1 record — at least kMergeMin on the first
        live lane's record, the wave is merged —, 8 units of one aniso record, 8 of one phi_only record, then units of all three;
      block 2 (4 waves): the roles rotated — 8 units of one aniso record first, 6 of a phi_only record, 6 of an iso_theta1 record;
      block 3: 1,024 random units, strays and the fixed blocks' dead units among them."""
    ctx = gpu["ctx"]
    names = ("iso_theta1", "phi_only", "aniso")
    cases = [vref.case(k) for k in names]
    ids = [_mid(gpu, k) for k in names]
    table = ctx.upload_table(np.ones((3, 4, 3, 5)), (1.0, 1.0, 1.0))
    ggx = ctx.ggx(0.2, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2))
    released = ctx.upload_table(np.ones((3, 4, 3, 5)), (1.0, 1.0, 1.0)); ctx.release_material(released)
    strays = [_mid(gpu, "iso_phi2"), table, ggx, released, -1, ctx.material_count() + 7]
    rng = np.random.default_rng(91)
    recs = [_by_record(c)[0] for c in cases]
    lives = [np.flatnonzero(c["alive"][:vref.rref.N_RANDOM]) for c in cases]
    dead0 = np.flatnonzero(~cases[0]["alive"])
    role, unit = [], []

    def add(r, units):
        role.extend([r] * len(units)); unit.extend(int(u) for u in units)
    for w in range(4):
        add(0, dead0[:w])
        add(0, np.resize(recs[0][w], 6)); add(2, np.resize(recs[2][w], 8)); add(1, np.resize(recs[1][w], 8))
        rest = 64 - w - 22
        for k, r in enumerate(rng.integers(0, 3, rest)):
            add(int(r), [rng.choice(lives[r])] if k % 3 else [recs[r][4 + w][k % len(recs[r][4 + w])]])     # every third: a shared record
    for w in range(4):
        add(2, np.resize(recs[2][8 + w], 8)); add(1, np.resize(recs[1][8 + w], 6)); add(0, np.resize(recs[0][8 + w], 6))
        for r in rng.integers(0, 3, 44):
            add(int(r), [rng.choice(lives[r])])
    n_total = len(cases[0]["wi"])
    for r in rng.integers(0, 3 + len(strays), 1024):
        add(int(r), [rng.integers(0, n_total)])
    role, unit = np.array(role), np.array(unit)
    assert len(role) == 1536 and all(len(c["wi"]) == n_total for c in cases)
    assert K_MERGE_MIN <= 6
    src = np.where(role >= 3, 0, role)
    wi = np.stack([cases[k]["wi"][u] for k, u in zip(src, unit)]); wo = np.stack([cases[k]["wo"][u] for k, u in zip(src, unit)])
    g = np.stack([cases[k]["g"][u] for k, u in zip(src, unit)]).astype(np.float32)
    g[role >= 3] = np.nan                                          # non-target units carry NaN
    mat = np.array(ids + strays, np.int32)[role]
    return cases, ids, role, unit, mat, wi, wo, g


def _target_refs(cases, role, unit, served):
    """per target: (its units among the slots `served` — in that order, a slot listed twice twice —, reference dict, term counts)"""
    out = []
    for k, c in enumerate(cases):
        mine = unit[served][role[served] == k]
        al = mine[c["alive"][mine]]
        G, S, _ = vref.values_grad(c["arrays"], c["wi"][al], c["wo"][al], c["g"][al])
        out.append((mine, dict(c, G=G, S=S), vref.term_counts(c["arrays"], c["wi"][al], c["wo"][al], c["g"][al])))
    return out


def test_material_ids_of_three_bracket_shapes_in_batch_and_queue_form(gpu):
    """MULTI kernels, whole arrays and over a queue: merged waves whose records have S = 1, 2 and 4 (the slot < 12 S predicate and the
    S of the first lane of a record), on the four kernel variants; every target against autograd and against its own
    single-material call; the queue form replayed twice from a captured graph."""
    import torch
    ctx, host = gpu["ctx"], gpu["host"]
    cases, ids, role, unit, mat, wi, wo, g = _mixed_units(gpu)
    n = len(role)
    offsets = host.rgl_values_grad_layout([ctx.rgl_values_shape(i) for i in ids])
    # the queue: a permutation of the slots that keeps the waves of blocks 1 and 2 whole (a wave of the queue launch is 64 consecutive
    # queue entries), one slot listed twice, the count below the capacity
    rng = np.random.default_rng(92)
    tail = 512 + rng.permutation(1024)
    waves = [np.arange(64 * w, 64 * w + 64) for w in rng.permutation(8)]
    slots = np.concatenate([tail[:512]] + waves + [tail[512:]]).astype(np.int32)
    assert np.array_equal(np.sort(slots), np.arange(n))
    slots[7] = slots[3]
    count_host = n - 300
    forms = {"batch": np.arange(n), "queue": slots[:count_host].astype(np.int64)}
    refs = {form: _target_refs(cases, role, unit, served) for form, served in forms.items()}
    dwi, dwo, dg, dmat, queue = _dev(wi, wo, g, mat, slots)
    count = torch.tensor([count_host], dtype=torch.int32, device="cuda")

    def run(form, out=None):
        if form == "batch":
            return ctx.rgl_values_grad(dwi, dwo, dg, ids, mat=dmat, out=out)
        return ctx.rgl_values_grad_queue(dwi, dwo, dg, queue, count, ids, mat=dmat, out=out)
    worst = [0.0]
    try:
        for variant in (0, 1, 2, 3):
            ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
            for form in forms:
                views = run(form, torch.full((offsets[-1],), SENTINEL, dtype=torch.float64, device="cuda"))
                clean = run(form)                                  # from zeros: compared with the targets' own calls
                for k, (c, mid) in enumerate(zip(cases, ids)):
                    mine, ref, m = refs[form][k]
                    assert len(mine) > 100
                    vref.check(views[k].cpu().numpy(), ref, SENTINEL, f"three shapes, {form}, variant {variant}, target {c['name']}")
                    own = _grad(gpu, mid, c["wi"][mine], c["wo"][mine], c["g"][mine])
                    _same(clean[k].cpu().numpy(), own, m, ref["S"], f"three shapes, {form}, variant {variant}, target {c['name']} against its own call", worst)
    finally:
        ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)
    print(f"three shapes: a target differs from its own single-material call by at most {worst[0]:.3f} of m_t 2^-52 S_t")
    # the queue form captured (the workspace has its size by now) and replayed twice: adds twice
    out = torch.full((offsets[-1],), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        run("queue", out)
    out.fill_(SENTINEL)
    graph.replay(); graph.replay()
    torch.cuda.synchronize()
    for k, c in enumerate(cases):
        _, ref, _ = refs["queue"][k]
        vref.check(out[offsets[k]:offsets[k + 1]].cpu().numpy(), dict(c, G=2 * ref["G"], S=2 * ref["S"]), SENTINEL,
                   f"three shapes, queue replayed twice from a graph, target {c['name']}", adds=2)
    ctx.use_own_stream()


def _queue_form_and_its_graph_replay(gpu, name, variant):
    import torch
    ctx, host = gpu["ctx"], gpu["host"]
    c = vref.case(name)
    mid = _mid(gpu, name)
    n = len(c["wi"])
    slots = np.random.default_rng(11).permutation(n)[:1200].astype(np.int32)
    slots[7] = slots[3]                                            # a slot listed twice adds twice
    wi, wo, g, queue = _dev(c["wi"], c["wo"], c["g"], slots)
    count = torch.tensor([700], dtype=torch.int32, device="cuda")   # below the capacity: slots past it are not served
    served = slots[:700]
    al = c["alive"][served]
    G, S, _ = vref.values_grad(c["arrays"], c["wi"][served][al], c["wo"][served][al], c["g"][served][al])
    ref = dict(c, G=G, S=S)
    shape = ctx.rgl_values_shape(mid)
    ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, variant)
    try:
        out = torch.full((int(np.prod(shape)),), SENTINEL, dtype=torch.float64, device="cuda")
        (view,) = ctx.rgl_values_grad_queue(wi, wo, g, queue, count, [mid], material=mid, out=out)
        vref.check(view.cpu().numpy(), ref, SENTINEL, f"{name} variant {variant}: queue, count below capacity, a slot twice")
        count.fill_(0)
        before = out.clone()
        ctx.rgl_values_grad_queue(wi, wo, g, queue, count, [mid], material=mid, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), before.view(torch.int64))
        # captured (the workspace has its size by now) and replayed twice: adds twice
        count.fill_(700)
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.graph(graph, stream=side):
            ctx.rgl_values_grad_queue(wi, wo, g, queue, count, [mid], material=mid, out=out)
        out.fill_(SENTINEL)
        graph.replay(); graph.replay()
        torch.cuda.synchronize()
        vref.check(out.cpu().numpy(), dict(c, G=2 * G, S=2 * S), SENTINEL, f"{name} variant {variant}: queue replayed twice from a graph", adds=2)
    finally:
        ctx.use_own_stream()
        ctx.set_option(host.OPT_TABLE_GRAD_KERNEL, 0)


def test_queue_form_and_its_graph_replay(gpu):
    _queue_form_and_its_graph_replay(gpu, "iso", 0)


@pytest.mark.parametrize("name,variant", [("iso", 1), ("iso_theta1", 0), ("iso_theta1", 1), ("phi_only", 0), ("phi_only", 1), ("aniso", 0), ("aniso", 1)])
def test_queue_form_on_every_bracket_shape_and_the_plain_kernel(gpu, name, variant):
    """k_rgl_values_bricks<false, true, 1 | 3 | 15> and k_rgl_values_plain<false, true>, as test_queue_form_and_its_graph_replay
    holds <false, true, 5>"""
    _queue_form_and_its_graph_replay(gpu, name, variant)


@pytest.mark.parametrize("name", ["iso", "aniso"])
def test_adjoint_identity_against_eval(gpu, name):
    ctx = gpu["ctx"]
    c = vref.case(name)
    mid = _mid(gpu, name)
    R = np.asarray(c["fields"]["rgb"], np.float64)
    assert R.min() >= 0.0
    g = np.where(c["alive"][:, None], c["g"], 0.0).astype(np.float32)          # eval's own zeros on dead units; a finite g there
    wi, wo, gd = _dev(c["wi"], c["wo"], g)
    E = ctx.eval(wi, wo, material=mid).cpu().numpy().astype(np.float64)
    G = _grad(gpu, mid, c["wi"], c["wo"], g)
    lhs, rhs, scale = float((g * E).sum()), float((R * G).sum()), float(np.abs(g * E).sum())
    print(f"{name}: sum g.eval(R) = {lhs:.9e}, <R, G> = {rhs:.9e}, |difference| = {abs(lhs - rhs) / scale:.3e} of sum |g E|")
    assert abs(lhs - rhs) <= 2e-6 * scale


def test_error_codes(gpu):
    import torch
    from mitsuba_customization_amd import synth
    ctx, host = gpu["ctx"], gpu["host"]
    c = vref.case("iso")
    mid = _mid(gpu, "iso")
    wi, wo, g = _dev(c["wi"][:64], c["wo"][:64], np.ones((64, 3), np.float32))
    table = ctx.upload_table(np.ones((3, 4, 3, 5)), (1.0, 1.0, 1.0))
    ggx = ctx.ggx(0.2, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2))
    spectral = ctx.upload_rgl(synth.make_rgl_fields(seed=3, n_phi=1, n_theta=3, res=8, n_wavelengths=4))
    released = ctx.upload_rgl(c["fields"]); ctx.release_material(released)

    def status(f):
        with pytest.raises(host.MerlHipError) as e:
            f()
        return e.value.status
    for bad in (table, ggx, spectral, released, -1, ctx.material_count() + 3):
        assert status(lambda: ctx.rgl_values_grad(wi, wo, g, [bad], material=mid)) == host.ERR_MATERIAL, bad
        assert status(lambda: ctx.rgl_values_grad(wi, wo, g, [mid, bad], material=mid)) == host.ERR_MATERIAL, bad
    assert status(lambda: ctx.rgl_values_grad(wi, wo, g, [mid, mid], material=mid)) == host.ERR_INVALID
    assert status(lambda: ctx.rgl_values_grad(wi, wo, g, [], material=mid)) == host.ERR_INVALID
    assert status(lambda: ctx.rgl_values_grad(wi, wo, g, [mid] * 17, material=mid)) == host.ERR_INVALID
    # the C calls themselves: n_targets out of range, null pointers, mixed pointers, a queue from host memory
    import ctypes as C
    lib, h = ctx._lib, ctx._ctx
    t = (C.c_int32 * 17)(*([mid] * 17))
    out = torch.zeros(int(np.prod(ctx.rgl_values_shape(mid))), dtype=torch.float64, device="cuda")
    P = lambda x: x.data_ptr()
    assert lib.mrl_rgl_values_grad_batch(h, P(wi), P(wo), P(g), None, mid, 64, t, 0, P(out)) == host.ERR_INVALID
    assert lib.mrl_rgl_values_grad_batch(h, P(wi), P(wo), P(g), None, mid, 64, t, 17, P(out)) == host.ERR_INVALID
    assert lib.mrl_rgl_values_grad_batch(h, None, P(wo), P(g), None, mid, 64, t, 1, P(out)) == host.ERR_INVALID
    assert lib.mrl_rgl_values_grad_batch(h, P(wi), P(wo), P(g), None, mid, 64, None, 1, P(out)) == host.ERR_INVALID
    assert lib.mrl_rgl_values_grad_batch(h, P(wi), P(wo), P(g), None, mid, 64, t, 1, None) == host.ERR_INVALID
    host_out = np.zeros(out.numel())
    assert lib.mrl_rgl_values_grad_batch(h, P(wi), P(wo), P(g), None, mid, 64, t, 1, host_out.ctypes.data) == host.ERR_POINTER_MIX
    queue = torch.arange(64, dtype=torch.int32, device="cuda"); count = torch.tensor([64], dtype=torch.int32, device="cuda")
    assert lib.mrl_rgl_values_grad_queue(h, P(wi), P(wo), P(g), None, mid, None, P(count), 64, t, 1, P(out)) == host.ERR_INVALID
    hq = np.arange(64, dtype=np.int32)
    assert lib.mrl_rgl_values_grad_queue(h, P(wi), P(wo), P(g), None, mid, hq.ctypes.data, P(count), 64, t, 1, P(out)) == host.ERR_POINTER_MIX
    assert lib.mrl_rgl_values_grad_queue(h, P(wi), P(wo), P(g), None, mid, P(queue), P(count), (1 << 32) + 1, t, 1, P(out)) == host.ERR_INVALID
    # empty calls: MRL_OK, nothing is touched, whatever the other arguments are
    assert lib.mrl_rgl_values_grad_batch(h, None, None, None, None, -5, 0, None, 0, None) == 0
    assert lib.mrl_rgl_values_grad_queue(h, None, None, None, None, -5, None, None, 0, None, 0, None) == 0
    # a single_id that is no target: nothing is added
    (none,) = ctx.rgl_values_grad(wi, wo, g, [mid], material=table)
    assert (none == 0).all()
    torch.cuda.synchronize()
    assert (out == 0).all()
    # the workspace is the context's, reported by mrl_memory_info
    assert ctx.memory_info()["workspace_bytes"] > 0
