"""mrl_table_grad_dir_batch_nch / mrl_table_grad_dir_queue_nch on the device against the autograd reference of
tests/nch_dir_grad_reference.py (which tests/test_nch_dir_grad_cpu.py ties to the RGB reference slice by slice): 2^13 generate_pairs
units and the targeted block on dims (7, 5, 12) with 1, 2, 4, 5, 8 and 32 channels, a standard and a full-azimuth table, kept negative
texels, no cosine factor, the nearest lookup, 'flat6' and 16 channels on (33, 17, 64); then the embedding of an RGB table in 8 and in 4
channels (equal to mrl_table_grad_dir_batch as numbers), three channels forwarded to the RGB twin, the shapes around a wave, a block
and one round of the grid, NULL outputs, material ids, queues (also replayed from a graph), host arrays, the error returns, the
autograd wrapper and examples/fit_normal_spectral.py.

The bar is the project's: |G - R|_2 <= 1e-6 S per unit and side, S = sum_c |g_c| |J_c|_2, on every live unit that the reference does not
excuse; exact +0.0 on dead units; G == 0 where S == 0; everything finite.  The whole-array, material-id, queue and host-array forms are
compared bit for bit (the contract of the calls).
Measured on MI355X, worst |G - R| / S per case, wi / wo side, in units of 1e-8:
  spectral-c1-7x5x12-halfdiff-node0                5.72 / 5.82
  spectral-c2-7x5x12-halfdiff-node0                5.66 / 5.79
  spectral-c4-7x5x12-halfdiff-node0                5.37 / 5.74
  spectral-c5-7x5x12-halfdiff-node0                5.64 / 5.46
  spectral-c8-7x5x12-halfdiff-node0                5.32 / 5.31
  spectral-c32-7x5x12-halfdiff-node0               4.68 / 5.61
  spectral-c5-7x5x12-standard-node1                5.47 / 5.84
  noise-c8-7x5x12-full-node0-keep                  5.46 / 5.42
  spectral-c4-7x5x12-halfdiff-node0-nocos          5.79 / 5.38
  spectral-c2-7x5x12-halfdiff-node0-nearest        0 (exact) / 5.85
  flat6-c6-7x5x12-halfdiff-node0-nocos             5.56 / 5.73
  spectral-c16-33x17x64-halfdiff-node0             5.25 / 5.24
All of it is the rounding of the f32 output (2^-24 sqrt(3) = 1.03e-7 at most).  The embedded RGB tables return the RGB call's numbers
on every unit; fit_normal_spectral ends 2.5e-9 rad from the truth (from 0.2 rad), loss 4.2e4 -> 4.1e-11."""
import os
import sys

import numpy as np
import pytest

from tests import nch_dir_grad_reference as nref
from tests import table_dir_grad_reference as tref

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(nref.CASES) + [nref.BIG_CASE]
CASE_IDS = [nref.case_id(c) for c in CASES]
MAIN = nref.CASES[4]                                                     # 8 channels, two groups: the case of the tests that are not about accuracy
WORST = {"device": 0.0}


def make_context(host, case):
    node, no_cosine, keep, lookup = case[3:7]
    ctx = host.MerlHip(0)
    ctx.set_option(host.OPT_LOOKUP, lookup); ctx.set_option(host.OPT_NODE, node)
    ctx.set_option(host.OPT_COSINE_FACTOR, no_cosine); ctx.set_option(host.OPT_NEGATIVE, keep)
    return ctx


def upload(ctx, d):
    return ctx.upload_table_param(d["planar"], d["param"], d["scale"])


def to_dev(*arrs):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrs]            # a copy: the cases are read-only


def bits(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else x
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def sentinel(n, device=True):
    a = np.full((n, 3), SENTINEL, np.float32)
    return to_dev(a)[0] if device else a


def check(Gi, Go, d, sel, tag):
    """both sides of the units `sel` of case data d against the reference; returns the worst |G - R| / S"""
    Gi, Go = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (Gi, Go))
    wi = nref.check_side(Gi, d["Ji"][sel], d["g"][sel], d["alive"][sel], d["excused"][sel], tag + " wi")
    wo = nref.check_side(Go, d["Jo"][sel], d["g"][sel], d["alive"][sel], d["excused"][sel], tag + " wo")
    print(f"{tag}: worst |G - R| / S = {wi:.2e} (wi) {wo:.2e} (wo); {int(d['excused'][sel].sum())} units excused")
    return max(wi, wo)


@pytest.fixture(scope="module")
def gpu(oracle):
    """the context of MAIN's options with the 8-channel table, an 8-channel table of other dims in the standard form, a 5-channel
    table, an RGB table, a GGX and a released 8-channel id"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from mitsuba_customization_amd import host
    ctx = make_context(host, MAIN)
    d = nref.case_data(oracle, MAIN)
    main = upload(ctx, d)
    other8 = ctx.upload_table_param(nref.make_test_table("spectral", 8, (4, 6, 9), nref.STANDARD), nref.STANDARD, nref.scales(8))
    five = upload(ctx, nref.case_data(oracle, nref.CASES[3]))
    rgb = ctx.upload_table_param(tref.make_test_table("smooth", tref.SMALL_DIMS, tref.HALF_DIFF), tref.HALF_DIFF, tref.SCALE)
    ggx = ctx.ggx(0.3, (0.143, 0.375, 1.442), (3.983, 2.386, 1.603))
    released = upload(ctx, d)
    ctx.release_material(released)
    yield dict(ctx=ctx, host=host, d=d, main=main, other8=other8, five=five, rgb=rgb, ggx=ggx, released=released)
    ctx.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_parity_with_autograd(oracle, case):
    from mitsuba_customization_amd import host
    d = nref.case_data(oracle, case)
    with make_context(host, case) as ctx:
        mid = upload(ctx, d)
        assert ctx.material_channels(mid) == d["n_ch"] and ctx.material_param(mid) == d["param"]
        Gi, Go = ctx.table_grad_dir_nch(*to_dev(d["wi"], d["wo"], d["g"]), d["n_ch"], material=mid)
        Gi, Go = Gi.cpu().numpy(), Go.cpu().numpy()
    WORST["device"] = max(WORST["device"], check(Gi, Go, d, slice(None), nref.case_id(case)))
    print(f"worst so far: {WORST['device']:.2e}")
    if not d["lookup"]:
        assert not Gi.any() and not Go[:, :2].any()                 # nearest: grad_wi == 0 exactly, grad_wo along e_z
        assert np.abs(Go[:, 2]).max() > 0
    else:
        assert np.abs(Gi).max() > 0
    assert (~d["alive"]).sum() == nref.N_DEAD_TARGETED and not np.isfinite(d["g"][~d["alive"]]).any()


@pytest.mark.parametrize("n_ch, slots", [(8, (1, 4, 6)), (4, (0, 1, 2))], ids=("c8-at-1-4-6", "c4-at-0-1-2"))
@pytest.mark.parametrize("case", [tref.SMALL_CASES[0], tref.SMALL_CASES[3], tref.SMALL_CASES[9]],
                         ids=[tref.case_id(tref.SMALL_CASES[i]) for i in (0, 3, 9)])
def test_embedded_rgb_table_returns_the_rgb_call(oracle, case, n_ch, slots):
    """An RGB table T and an n_ch-channel table holding T's planes at `slots` with other planes in between, the same scales,
    parameterisation and options, g zero off those channels: the n-channel call must EQUAL mrl_table_grad_dir_batch on T as numbers on
    every unit (only the sign of a zero may differ) — the channels are summed in ascending order in one chain of FMAs, a zero g changes
    nothing, and everything after the t_k is the RGB function's code."""
    from mitsuba_customization_amd import host
    d = tref.case_data(oracle, case, nref.N_RANDOM)
    rng = np.random.default_rng(21)
    planar = rng.uniform(-50.0, 900.0, (n_ch,) + tuple(d["dims"]))
    scale = list(rng.choice([0.5, 1.0, 2.0], n_ch))
    g = rng.standard_normal((len(d["wi"]), n_ch)).astype(np.float32)
    g[:] = 0.0
    for c, slot in enumerate(slots):
        planar[slot], scale[slot] = d["planar"][c], tref.SCALE[c]
        g[:, slot] = d["g"][:, c]
    ctx = host.MerlHip(0)
    ctx.set_option(host.OPT_LOOKUP, d["lookup"]); ctx.set_option(host.OPT_NODE, d["node"])
    ctx.set_option(host.OPT_COSINE_FACTOR, d["no_cosine"]); ctx.set_option(host.OPT_NEGATIVE, d["keep"])
    with ctx:
        rgb = ctx.upload_table_param(d["planar"], d["param"], tref.SCALE)
        wide = ctx.upload_table_param(planar, d["param"], scale)
        wi, wo = to_dev(d["wi"], d["wo"])
        Ri, Ro = (x.cpu().numpy() for x in ctx.table_grad_dir(wi, wo, to_dev(d["g"])[0], material=rgb))
        Ni, No = (x.cpu().numpy() for x in ctx.table_grad_dir_nch(wi, wo, to_dev(g)[0], n_ch, material=wide))
    assert np.array_equal(Ni, Ri) and np.array_equal(No, Ro)
    assert np.abs(Ri).max() > 0 and np.isfinite(Ni).all() and np.isfinite(No).all()
    dead = ~d["alive"]
    assert not bits(Ni[dead]).any() and not bits(No[dead]).any()      # +0.0f


def test_three_channels_return_the_rgb_calls_bits(gpu):
    import torch
    ctx, d = gpu["ctx"], gpu["d"]
    wi, wo = to_dev(d["wi"], d["wo"])
    g = to_dev(np.ascontiguousarray(d["g"][:, :3]))[0]
    n = len(d["wi"])
    Ri, Ro = ctx.table_grad_dir(wi, wo, g, material=gpu["rgb"])
    Ni, No = ctx.table_grad_dir_nch(wi, wo, g, 3, material=gpu["rgb"])
    assert same_bits(Ni, Ri) and same_bits(No, Ro) and float(Ri.abs().max()) > 0
    queue = torch.arange(n, dtype=torch.int32, device="cuda")
    count = torch.full((1,), n, dtype=torch.int32, device="cuda")
    Qi, Qo = ctx.table_grad_dir_queue_nch(wi, wo, g, queue, count, 3, material=gpu["rgb"])
    assert same_bits(Qi, Ri) and same_bits(Qo, Ro)
    with pytest.raises(gpu["host"].MerlHipError) as e:               # the RGB twin's rule: an n-channel table is not an RGB table
        ctx.table_grad_dir_nch(wi, wo, g, 3, material=gpu["main"])
    assert e.value.status == gpu["host"].ERR_MATERIAL


def shape_selection(d, n):
    """the first units of the random block and the last of the targeted one (dead units with NaN / inf in g among them)"""
    sel = np.r_[0:(n + 1) // 2, len(d["wi"]) - n // 2:len(d["wi"])]
    assert len(sel) == n
    return sel


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 257))
def test_shapes_around_a_wave_and_a_block(gpu, n):
    d, ctx, c = gpu["d"], gpu["ctx"], gpu["d"]["n_ch"]
    sel = shape_selection(d, n)
    Gi, Go = ctx.table_grad_dir_nch(*to_dev(d["wi"][sel], d["wo"][sel], d["g"][sel]), c, material=gpu["main"])
    check(Gi, Go, d, sel, f"n={n}")
    # the same units run in two halves
    h = n // 2
    for part in (slice(0, h), slice(h, n)):
        if part.stop > part.start:
            Hi, Ho = ctx.table_grad_dir_nch(*to_dev(d["wi"][sel][part], d["wo"][sel][part], d["g"][sel][part]), c, material=gpu["main"])
            assert same_bits(Hi, Gi[part]) and same_bits(Ho, Go[part])


@pytest.mark.parametrize("n_ch", (2, 8), ids=("c2", "c8"))
def test_more_units_than_one_round_of_the_grid(oracle, gpu, n_ch):
    from mitsuba_customization_amd import host
    case = nref.CASES[1] if n_ch == 2 else MAIN
    d = nref.case_data(oracle, case)
    block, per_cu = nref.launch_shape(n_ch)
    with make_context(host, case) as ctx:
        mid = upload(ctx, d)
        n, m = block * per_cu * ctx.compute_units + 65, len(d["wi"])
        sel = np.arange(n) % m                                       # the case tiled: the reference is reused
        once = [x.cpu().numpy() for x in ctx.table_grad_dir_nch(*to_dev(d["wi"], d["wo"], d["g"]), n_ch, material=mid)]
        check(once[0], once[1], d, slice(None), f"n={m}")
        wi, wo, g = to_dev(d["wi"][sel], d["wo"][sel], d["g"][sel])
        Gi, Go = ctx.table_grad_dir_nch(wi, wo, g, n_ch, material=mid)
        # a unit's bits do not depend on n, the grid or its position
        assert same_bits(Gi, once[0][sel]) and same_bits(Go, once[1][sel])
        h = n // 2 + 1
        for part in (slice(0, h), slice(h, n)):
            Hi, Ho = ctx.table_grad_dir_nch(wi[part].contiguous(), wo[part].contiguous(), g[part].contiguous(), n_ch, material=mid)
            assert same_bits(Hi, Gi[part]) and same_bits(Ho, Go[part])
        Ii, Io = ctx.table_grad_dir_nch(wi, wo, g, n_ch, mat=to_dev(np.full(n, mid, np.int32))[0])
        assert same_bits(Ii, Gi) and same_bits(Io, Go)


def test_null_outputs(gpu):
    d, ctx, host, mid, c = gpu["d"], gpu["ctx"], gpu["host"], gpu["main"], gpu["d"]["n_ch"]
    wi, wo, g = to_dev(d["wi"], d["wo"], d["g"])
    n = len(d["wi"])
    Gi, Go = ctx.table_grad_dir_nch(wi, wo, g, c, material=mid)
    call = ctx._lib.mrl_table_grad_dir_batch_nch
    for keep, null in ((0, 1), (1, 0)):
        outs = [sentinel(n), sentinel(n)]
        ptrs = [o.data_ptr() for o in outs]
        ptrs[null] = None
        ctx.use_torch_stream()
        assert call(ctx._ctx, wi.data_ptr(), wo.data_ptr(), g.data_ptr(), None, mid, n, c, *ptrs) == 0
        ctx.synchronize()
        assert same_bits(outs[keep], (Gi, Go)[keep])
        assert same_bits(outs[null], sentinel(n, device=False))
        one = ctx.table_grad_dir_nch(wi, wo, g, c, material=mid, want=("wi", "wo")[keep])
        assert same_bits(one, (Gi, Go)[keep])
    assert call(ctx._ctx, wi.data_ptr(), wo.data_ptr(), g.data_ptr(), None, mid, n, c, None, None) == host.ERR_INVALID


def test_material_ids(gpu):
    import torch
    ctx, d, c = gpu["ctx"], gpu["d"], gpu["d"]["n_ch"]
    n = 4099
    sel = shape_selection(d, n)
    wi, wo, g = to_dev(d["wi"][sel], d["wo"][sel], d["g"][sel])
    mine8 = [gpu["main"], gpu["other8"]]
    choices = mine8 + [gpu["five"], gpu["rgb"], gpu["ggx"], gpu["released"], ctx.material_count() + 5, -1]
    mat = np.array(choices, np.int32)[np.random.default_rng(7).integers(0, len(choices), n)]
    Gi, Go = ctx.table_grad_dir_nch(wi, wo, g, c, mat=to_dev(mat)[0])
    only_wo = ctx.table_grad_dir_nch(wi, wo, g, c, mat=to_dev(mat)[0], want="wo")
    assert same_bits(only_wo, Go)
    for mid in mine8:
        Si, So = ctx.table_grad_dir_nch(wi, wo, g, c, material=mid)
        mine = mat == mid
        assert mine.sum() > 100
        assert same_bits(Gi.cpu().numpy()[mine], Si.cpu().numpy()[mine]) and same_bits(Go.cpu().numpy()[mine], So.cpu().numpy()[mine])
        assert float(Si.abs().max()) > 0
    other = ~np.isin(mat, mine8)
    assert other.sum() > 100
    zeros = np.zeros((int(other.sum()), 3), np.float32)
    assert same_bits(Gi.cpu().numpy()[other], zeros) and same_bits(Go.cpu().numpy()[other], zeros)
    assert torch.isfinite(Gi).all() and torch.isfinite(Go).all()
    # the other width sees the other table; a width no table of the context has: zeros everywhere
    g5 = to_dev(np.ascontiguousarray(d["g"][sel][:, :5]))[0]
    Fi, Fo = ctx.table_grad_dir_nch(wi, wo, g5, 5, mat=to_dev(mat)[0])
    Si, So = ctx.table_grad_dir_nch(wi, wo, g5, 5, material=gpu["five"])
    five = mat == gpu["five"]
    assert same_bits(Fi.cpu().numpy()[five], Si.cpu().numpy()[five]) and same_bits(Fo.cpu().numpy()[five], So.cpu().numpy()[five])
    assert not bits(Fi.cpu().numpy()[~five]).any() and not bits(Fo.cpu().numpy()[~five]).any() and float(Fi.abs().max()) > 0
    g16 = to_dev(np.ascontiguousarray(np.tile(d["g"][sel], (1, 2))))[0]
    Zi, Zo = ctx.table_grad_dir_nch(wi, wo, g16, 16, mat=to_dev(mat)[0], out=(sentinel(n), sentinel(n)))
    assert not bits(Zi).any() and not bits(Zo).any()


@pytest.mark.parametrize("with_ids", (False, True), ids=("single", "ids"))
def test_queue(gpu, with_ids):
    import torch
    ctx, d, c = gpu["ctx"], gpu["d"], gpu["d"]["n_ch"]
    cap = 1000
    sel = shape_selection(d, cap)
    wi, wo, g = to_dev(d["wi"][sel], d["wo"][sel], d["g"][sel])
    kw = dict(material=gpu["main"])
    if with_ids:
        choices = np.array([gpu["main"], gpu["other8"], gpu["five"], gpu["ggx"], -1], np.int32)
        kw = dict(mat=to_dev(choices[np.random.default_rng(8).integers(0, len(choices), cap)])[0])
    Wi, Wo = (x.cpu().numpy() for x in ctx.table_grad_dir_nch(wi, wo, g, c, **kw))
    order = np.random.default_rng(9).permutation(cap).astype(np.int32)
    queue = to_dev(order)[0]
    blank = sentinel(cap, device=False)

    def expect(whole, count):
        e = blank.copy()
        e[order[:count]] = whole[order[:count]]
        return e
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in (0, 1, 517, 5000):
        count.fill_(k)
        outs = (sentinel(cap), sentinel(cap))
        ctx.table_grad_dir_queue_nch(wi, wo, g, queue, count, c, out=outs, **kw)
        ctx.synchronize()
        served = min(k, cap)
        assert same_bits(outs[0], expect(Wi, served)) and same_bits(outs[1], expect(Wo, served)), k
    # one capture (a single branch: one launch on one stream), replayed with another device-side count
    outs = (sentinel(cap), sentinel(cap))
    count.fill_(3)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        ctx.table_grad_dir_queue_nch(wi, wo, g, queue, count, c, out=outs, **kw)
    for k in (3, 700):
        for o in outs:
            o.fill_(SENTINEL)
        count.fill_(k)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(outs[0], expect(Wi, k)) and same_bits(outs[1], expect(Wo, k)), k
    ctx.use_own_stream()


def test_host_arrays_in_chunks_and_pointer_mix(gpu):
    ctx, host, d, c = gpu["ctx"], gpu["host"], gpu["d"], gpu["d"]["n_ch"]
    n = 3 * 4096 + 5
    sel = np.arange(n) % len(d["wi"])
    arrs = [np.ascontiguousarray(d[key][sel]) for key in ("wi", "wo", "g")]
    choices = np.array([gpu["main"], gpu["other8"], gpu["ggx"], ctx.material_count() + 5], np.int32)
    mat = choices[np.random.default_rng(10).integers(0, 4, n)]
    Di, Do = ctx.table_grad_dir_nch(*to_dev(*arrs), c, mat=to_dev(mat)[0])
    Ds = ctx.table_grad_dir_nch(*to_dev(*arrs), c, material=int(choices[0]))
    chunk = ctx.get_option(host.OPT_HOST_CHUNK)
    ctx.set_option(host.OPT_HOST_CHUNK, 4096)
    try:
        Hi, Ho = ctx.table_grad_dir_nch(*arrs, c, mat=mat)
        only_wi = ctx.table_grad_dir_nch(*arrs, c, mat=mat, want="wi", out=sentinel(n, device=False))
        Hs = ctx.table_grad_dir_nch(*arrs, c, material=int(choices[0]))
    finally:
        ctx.set_option(host.OPT_HOST_CHUNK, chunk)
    assert isinstance(Hi, np.ndarray) and isinstance(Ho, np.ndarray)
    assert same_bits(Hi, Di) and same_bits(Ho, Do) and same_bits(only_wi, Di)
    assert same_bits(Hs[0], Ds[0]) and same_bits(Hs[1], Ds[1])
    assert np.abs(Hi).max() > 0 and (Hi[np.isin(mat, choices[2:])] == 0).all()
    with pytest.raises(host.MerlHipError) as e:
        ctx.table_grad_dir_nch(to_dev(arrs[0])[0], arrs[1], arrs[2], c, material=int(choices[0]))
    assert e.value.status == host.ERR_POINTER_MIX
    with pytest.raises(host.MerlHipError) as e:
        ctx.table_grad_dir_nch(*to_dev(*arrs), c, material=int(choices[0]), out=(np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)))
    assert e.value.status == host.ERR_POINTER_MIX


def test_errors_and_memory_report(gpu):
    import torch
    ctx, host, d, c = gpu["ctx"], gpu["host"], gpu["d"], gpu["d"]["n_ch"]
    n = 64
    wi, wo, g = to_dev(d["wi"][:n], d["wo"][:n], d["g"][:n])
    queue = torch.arange(n, dtype=torch.int32, device="cuda")
    count = torch.full((1,), n, dtype=torch.int32, device="cuda")
    # a single id that is not a live n-channel table of that width
    for mid in (gpu["five"], gpu["rgb"], gpu["ggx"], gpu["released"], ctx.material_count() + 5, -1):
        with pytest.raises(host.MerlHipError) as e:
            ctx.table_grad_dir_nch(wi, wo, g, c, material=mid)
        assert e.value.status == host.ERR_MATERIAL, mid
        with pytest.raises(host.MerlHipError) as e:
            ctx.table_grad_dir_queue_nch(wi, wo, g, queue, count, c, material=mid)
        assert e.value.status == host.ERR_MATERIAL, mid
    mid = gpu["main"]
    Gi, Go = sentinel(n), sentinel(n)
    batch, queued = ctx._lib.mrl_table_grad_dir_batch_nch, ctx._lib.mrl_table_grad_dir_queue_nch
    p = [wi.data_ptr(), wo.data_ptr(), g.data_ptr()]
    ctx.use_torch_stream()
    # the channel count: what mrl_eval_batch_nch returns for it
    values = torch.empty((n, 40), dtype=torch.float32, device="cuda")
    for bad in (0, -1, 33):
        want = ctx._lib.mrl_eval_batch_nch(ctx._ctx, p[0], p[1], None, mid, n, bad, values.data_ptr())
        assert want == host.ERR_INVALID
        assert batch(ctx._ctx, *p, None, mid, n, bad, Gi.data_ptr(), Go.data_ptr()) == want
        assert queued(ctx._ctx, *p, None, mid, queue.data_ptr(), count.data_ptr(), n, bad, Gi.data_ptr(), Go.data_ptr()) == want
    for missing in range(3):
        ins = [None if i == missing else x for i, x in enumerate(p)]
        assert batch(ctx._ctx, *ins, None, mid, n, c, Gi.data_ptr(), Go.data_ptr()) == host.ERR_INVALID
        assert queued(ctx._ctx, *ins, None, mid, queue.data_ptr(), count.data_ptr(), n, c, Gi.data_ptr(), Go.data_ptr()) == host.ERR_INVALID
    assert queued(ctx._ctx, *p, None, mid, None, count.data_ptr(), n, c, Gi.data_ptr(), Go.data_ptr()) == host.ERR_INVALID
    assert queued(ctx._ctx, *p, None, mid, queue.data_ptr(), None, n, c, Gi.data_ptr(), Go.data_ptr()) == host.ERR_INVALID
    assert queued(ctx._ctx, *p, None, mid, queue.data_ptr(), count.data_ptr(), n, c, None, None) == host.ERR_INVALID
    assert queued(ctx._ctx, *p, None, mid, queue.data_ptr(), count.data_ptr(), (1 << 32) + 1, c, Gi.data_ptr(), Go.data_ptr()) == host.ERR_INVALID
    # host pointers in a queue call
    assert queued(ctx._ctx, d["wi"][:n].ctypes.data, *p[1:], None, mid, queue.data_ptr(), count.data_ptr(), n, c, Gi.data_ptr(),
                  Go.data_ptr()) == host.ERR_POINTER_MIX
    # the renormalising blend is refused (the policy is context-wide and set before the first table)
    with host.MerlHip(0) as other:
        other.set_option(host.OPT_NEGATIVE, 2)
        rid = upload(other, d)
        for call in (lambda: other.table_grad_dir_nch(wi, wo, g, c, material=rid),
                     lambda: other.table_grad_dir_queue_nch(wi, wo, g, queue, count, c, material=rid),
                     lambda: other.table_grad_dir_nch(wi, wo, g, c, mat=torch.full((n,), rid, dtype=torch.int32, device="cuda"))):
            with pytest.raises(host.MerlHipError) as e:
                call()
            assert e.value.status == host.ERR_INVALID
    ctx.use_torch_stream()
    before = ctx.memory_info()
    assert batch(ctx._ctx, *p, None, mid, 0, c, Gi.data_ptr(), Go.data_ptr()) == 0
    assert queued(ctx._ctx, *p, None, mid, queue.data_ptr(), count.data_ptr(), 0, c, Gi.data_ptr(), Go.data_ptr()) == 0
    ctx.synchronize()
    blank = sentinel(n, device=False)
    assert same_bits(Gi, blank) and same_bits(Go, blank)
    ctx.table_grad_dir_nch(wi, wo, g, c, material=mid, out=(Gi, Go))
    ctx.table_grad_dir_queue_nch(wi, wo, g, queue, count, c, material=mid, out=(Gi, Go))
    ctx.table_grad_dir_nch(wi, wo, g, c, mat=torch.full((n,), mid, dtype=torch.int32, device="cuda"), out=(Gi, Go))
    ctx.synchronize()
    after = ctx.memory_info()
    assert after["workspace_bytes"] == before["workspace_bytes"] and after["table_bytes"] == before["table_bytes"]      # no workspace
    assert not same_bits(Gi, blank)


def test_autograd_wrapper(gpu):
    from mitsuba_customization_amd import diff
    ctx, d, c, mid = gpu["ctx"], gpu["d"], gpu["d"]["n_ch"], gpu["main"]
    live = d["alive"]
    wi0, wo0, w = to_dev(d["wi"][live], d["wo"][live], d["g"][live])
    Gi, Go = ctx.table_grad_dir_nch(wi0, wo0, w, c, material=mid)
    wi, wo = wi0.clone().requires_grad_(True), wo0.clone().requires_grad_(True)
    values = diff.table_eval_nch(ctx, wi, wo, c, material=mid)
    assert tuple(values.shape) == (len(wi0), c) and same_bits(values.detach(), ctx.eval_nch(wi0, wo0, c, material=mid))
    (values * w).sum().backward()
    assert same_bits(wi.grad, Gi) and same_bits(wo.grad, Go) and float(Gi.abs().max()) > 0
    # only the gradient the graph asks for: the call is made with want = that side alone
    calls = []
    real = ctx.table_grad_dir_nch

    def spy(*a, **kw):
        calls.append(kw.get("want"))
        return real(*a, **kw)
    ctx.table_grad_dir_nch = spy
    try:
        wi, wo = wi0.clone().requires_grad_(True), wo0.clone()
        (diff.table_eval_nch(ctx, wi, wo, c, material=mid) * w).sum().backward()
        assert same_bits(wi.grad, Gi) and wo.grad is None
        wi, wo = wi0.clone(), wo0.clone().requires_grad_(True)
        (diff.table_eval_nch(ctx, wi, wo, c, material=mid) * w).sum().backward()
        assert same_bits(wo.grad, Go) and wi.grad is None
    finally:
        del ctx.table_grad_dir_nch
    assert calls == [("wi",), ("wo",)]
    # with ids
    choices = np.array([mid, gpu["other8"], gpu["five"], -1], np.int32)
    mat = to_dev(choices[np.random.default_rng(11).integers(0, len(choices), len(wi0))])[0]
    Ti, To = ctx.table_grad_dir_nch(wi0, wo0, w, c, mat=mat)
    wi, wo = wi0.clone().requires_grad_(True), wo0.clone().requires_grad_(True)
    values = diff.table_eval_nch(ctx, wi, wo, c, mat=mat)
    assert same_bits(values.detach(), ctx.eval_nch(wi0, wo0, c, mat=mat))
    (values * w).sum().backward()
    assert same_bits(wi.grad, Ti) and same_bits(wo.grad, To)
    with pytest.raises(gpu["host"].MerlHipError) as e:
        wi = wi0.clone().requires_grad_(True)
        g5 = w[:, :5].contiguous()
        (diff.table_eval_nch(ctx, wi, wo0, 5, material=gpu["five"]) * g5).sum().backward()        # fine: the width matches
        (diff.table_eval_nch(ctx, wi, wo0, 5, material=mid) * g5).sum().backward()
    assert e.value.status == gpu["host"].ERR_MATERIAL


def test_fit_normal_spectral_end_to_end():
    """The loss never rises (the line search guarantees it) and the normal converges to below 1e-6 rad from the 0.2 rad it starts
    from (the RGB twin ends two orders below that).  Measured on MI355X: 0.2 rad -> 2.469e-09 rad in 8 steps, loss 4.188e+04 -> 4.086e-11."""
    from mitsuba_customization_amd import host, synth
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import fit_normal_spectral
    with host.MerlHip(0) as ctx:
        mid = ctx.upload_table_nch(synth.make_table_nch("spectral", 16, 0))
        wi, wo, _ = ctx.generate_pairs(0xF17, 0, 1 << 14)
        angles, history, errors = fit_normal_spectral.fit_spectral(ctx, mid, 16, wi, wo)
    print(f"fit_normal_spectral on the device: angle error {errors[0]:.3e} -> {errors[-1]:.3e} rad; loss {history[0]:.3e} -> {history[-1]:.3e}")
    assert 0.19 <= errors[0] <= 0.21
    assert errors[-1] < 1e-6
    assert all(b <= a for a, b in zip(history, history[1:]))
