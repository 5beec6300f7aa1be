"""mrl_rgl_values_grad_batch / mrl_rgl_values_grad_queue (include/merl_hip_fit_rgl.h; MerlHip.rgl_values_grad / rgl_values_grad_queue):
the adjoint of eval in the measured values of RGB RGL materials on the GPU.  Reference: tests/rgl_values_grad_reference.py (autograd of
the torch-f64 restatement of the model).  Bars: per texel |G - R| <= 1e-6 S with the initial bits where S == 0; two forms of the same
sum agree within m_t 2^-52 S_t, m_t the number of terms of the texel (the bound of a reordered f64 sum of identical terms); the
adjoint identity |sum g . eval(R) - <R, G>| <= 2e-6 sum |g_c E_c| against the parent's eval.

Measured on MI355X, worst |G - R| / S per file: iso 2.2e-9, iso_nojac 4.9e-9, iso_theta1 6.5e-10, iso_phi2 1.6e-9,
aniso 1.1e-8, aniso_red2 1.0e-9, aniso_red4 4.6e-9, aniso_uneven 5.8e-10, iso_rows 9.5e-11, iso_cols 3.7e-10, iso_negative 1.9e-9,
ggx_res32 5.6e-8; the four kernel forms and the host-array form within 0.36 of m_t 2^-52 S_t of each other, a target of an id batch
within 0.32 of its own call; the adjoint identity 1.0e-10 (iso) and 3.0e-10 (aniso) of sum |g E|; the file runs in 3 s."""
import numpy as np
import pytest

from tests import rgl_values_grad_reference as vref

pytestmark = pytest.mark.gpu

SENTINEL = -4096.25            # larger than any sum of these tests: check() allows for the one rounding of an add into it


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


@pytest.mark.parametrize("name", ["iso", "aniso"])
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


def _merge_inputs(c):
    """{pattern: (wi, wo, g)} of 256 live units each: all one identical pair; every wave half on one record and half scattered; 3
    lanes of every wave on one record (below the merge rule), the rest scattered"""
    live = np.flatnonzero(c["alive"][:vref.rref.N_RANDOM])
    rng = np.random.default_rng(77)
    pick = lambda m: rng.choice(live, m, replace=False)
    g = rng.standard_normal((256, 3)).astype(np.float32)
    out = {}
    idx = np.full(256, live[3]); out["one pair"] = idx
    idx = pick(256); idx[np.arange(256) % 64 < 32] = live[5]; out["half on one record"] = idx
    idx = pick(256); idx[np.arange(256) % 64 < 3] = live[7]; out["3 lanes share"] = idx
    return {k: (c["wi"][i], c["wo"][i], g) for k, i in out.items()}


@pytest.mark.parametrize("name", ["iso", "aniso"])
def test_merge_paths_on_every_kernel_variant_and_host_arrays(gpu, name):
    c = vref.case(name)
    ctx, host = gpu["ctx"], gpu["host"]
    mid = _mid(gpu, name)
    worst = [0.0]
    try:
        for pattern, (wi, wo, g) in _merge_inputs(c).items():
            G, S, _ = vref.values_grad(c["arrays"], wi, wo, g)
            m = vref.term_counts(c["arrays"], wi, wo, g)
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


def test_queue_form_and_its_graph_replay(gpu):
    import torch
    ctx = gpu["ctx"]
    c = vref.case("iso")
    mid = _mid(gpu, "iso")
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
    out = torch.full((int(np.prod(shape)),), SENTINEL, dtype=torch.float64, device="cuda")
    (view,) = ctx.rgl_values_grad_queue(wi, wo, g, queue, count, [mid], material=mid, out=out)
    vref.check(view.cpu().numpy(), ref, SENTINEL, "queue, count below capacity, a slot twice")
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
    vref.check(out.cpu().numpy(), dict(c, G=2 * G, S=2 * S), SENTINEL, "queue replayed twice from a graph", adds=2)
    ctx.use_own_stream()


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
