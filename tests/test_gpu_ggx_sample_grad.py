"""mrl_ggx_pdf_grad_batch / _queue and mrl_ggx_sample_grad_batch / _queue on the device against the autograd reference of
tests/ggx_sample_grad_reference.py (which tests/test_ggx_sample_grad_cpu.py ties to the numpy model, the oracle's sampler and central
differences): every case of ggx_reference.CASES — 6 alpha x 4 metals, the first 2^13 generate_pairs units and the targeted block with
its NaN, inf, zero-length and below-horizon units, whose cotangents are NaN / inf here — then the host-compiled per-lane functions, the
shapes around a wave, a block and one round of the grid, every subset of NULL outputs, material ids, queues (also replayed from a
graph), host arrays, the error returns, the autograd wrappers and examples/fit_sampled_lobe.py.

The bar is the project's, per unit: |G - R|_2 <= 1e-6 S (check_pdf_case / check_sample_case of the reference module say what S is),
exact +0.0 on dead units, direction gradients orthogonal to their directions; alive / dead is what the forward call on the device says.
The whole-array, material-id, queue and host-array forms and every subset of outputs are compared bit for bit (the contract of the
calls).  Measured on MI355X over the 24 cases: worst |G - R| / S for the pdf gradient, each output at its own scale, 5.93e-8 (wi),
1.39e-7 (wo) and 5.95e-8 (alpha), 5.89e-8 at the scale of P's whole gradient; 5.92e-8 for the sample gradient in wi and 5.95e-8 in the
parameters; 0 random and 0 targeted sample units excluded by the stability rule in every case; the host-compiled functions and the
device agree bit for bit on 99.96 - 100 % of the units and to 8e-15 S on the rest; fit_sampled_lobe ends 5.5e-18 rad and
2.3e-8 in alpha from the truth on the device."""
import itertools
import os
import sys

import numpy as np
import pytest

from tests import ggx_reference as ggx
from tests import ggx_sample_grad_reference as sref

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
N_RANDOM = 1 << 13
CASE_IDS = [ggx.case_id(c) for c in ggx.CASES]
WORST = {"pdf": 0.0, "wi": 0.0, "params": 0.0}
PDF_OUTS = (("wi", 3), ("wo", 3), ("alpha", None))
SAMPLE_OUTS = (("wi", 3), ("params", 7))


@pytest.fixture(scope="module")
def gpu(tables):
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from mitsuba_customization_amd import host
    ctx = host.MerlHip(0)
    ids = {(alpha, metal): ctx.ggx(alpha, *ggx.METALS[metal]) for alpha, metal in ggx.CASES}
    table = ctx.upload_merl(tables("ggx_tab", 0))
    released = ctx.ggx(0.2, (1.0, 1.1, 1.2), (2.0, 2.1, 2.2))
    ctx.release_material(released)
    yield dict(ctx=ctx, ids=ids, table=table, released=released, host=host)
    ctx.close()


def to_dev(*arrs):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrs]            # a copy: the cases are read-only


def cpu(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def bits(x):
    return np.ascontiguousarray(cpu(x), np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def sentinel(n, cols, device=True):
    a = np.full((n,) if cols is None else (n, cols), SENTINEL, np.float32)
    return to_dev(a)[0] if device else a


def sentinels(n, outs, device=True):
    return tuple(sentinel(n, cols, device) for _, cols in outs)


class Call:
    """one of the two gradients: its inputs out of case data, its methods of the context, its raw symbols, its outputs"""
    def __init__(self, kind):
        self.kind = kind
        self.outs = PDF_OUTS if kind == "pdf" else SAMPLE_OUTS
        self.keys = ("wi", "wo", "gp") if kind == "pdf" else ("wi", "u", "go")
        self.names = tuple(name for name, _ in self.outs)

    def inputs(self, d, sel=slice(None)):
        return [np.ascontiguousarray(d[k][sel]) for k in self.keys]

    def finite_inputs(self, d, sel=slice(None)):
        """inputs() with finite cotangents everywhere: for calls whose units meet OTHER materials than the case's, under which a unit
        that is dead here (NaN / inf cotangent) may be alive"""
        ins = self.inputs(d, sel)
        ins[2] = np.where(np.isfinite(ins[2]), ins[2], np.float32(0.5)).astype(np.float32)
        return ins

    def batch(self, ctx, ins, **kw):
        return getattr(ctx, f"ggx_{self.kind}_grad")(*ins, **kw)

    def queue(self, ctx, ins, queue, count, **kw):
        return getattr(ctx, f"ggx_{self.kind}_grad_queue")(*ins, queue, count, **kw)

    def symbols(self, ctx):
        return getattr(ctx._lib, f"mrl_ggx_{self.kind}_grad_batch"), getattr(ctx._lib, f"mrl_ggx_{self.kind}_grad_queue")


CALLS = {"pdf": Call("pdf"), "sample": Call("sample")}
BOTH = pytest.mark.parametrize("call", list(CALLS.values()), ids=list(CALLS))


def forward_alive(ctx, d, sel, mid):
    """which units the forward calls on the device say are live: (pdf > 0 of the pair, pdf > 0 of the sample)"""
    wi, wo, u = to_dev(d["wi"][sel], d["wo"][sel], d["u"][sel])
    with np.errstate(all="ignore"):
        p = cpu(ctx.pdf(wi, wo, material=mid))
        s = cpu(ctx.sample(wi, u, material=mid)[1])
    return p > 0, s > 0


def subset(d, sel):
    """case data restricted to the units sel, for the reference module's checks"""
    out = dict(d)
    for key in ("wi", "wo", "u", "gp", "go", "sample_compared"):
        out[key] = d[key][sel]
    out["pdf"] = {k: v[sel] for k, v in d["pdf"].items()}
    out["sample"] = {k: v[sel] for k, v in d["sample"].items()}
    return out


def check(call, G, d, sel, alive, tag):
    """the outputs G of `call` on the units sel against the reference; returns the worst ratios by output group"""
    ds = subset(d, sel)
    G = [cpu(x) for x in G]
    if call.kind == "pdf":
        # a pair the forward pdf rounds to 0 in Float (a live f64 value below 1.4e-45) is still differentiated: alive is the reference's
        assert not (alive & ~ds["pdf"]["alive"]).any(), tag
        return {"pdf": sref.check_pdf_case(ds, G[0], G[1], G[2], ds["pdf"]["alive"], tag)}
    return {"wi": sref.check_sample_case(ds, G[0], None, alive, tag), "params": sref.check_sample_case(ds, None, G[1], alive, tag)}


@pytest.mark.parametrize("case", ggx.CASES, ids=CASE_IDS)
def test_parity_with_autograd(gpu, oracle, case):
    d = sref.case_data(oracle, *case, N_RANDOM)
    ctx, mid, tag = gpu["ctx"], gpu["ids"][case], ggx.case_id(case)
    alive_p, alive_s = forward_alive(ctx, d, slice(None), mid)
    r, t = sref.excluded_within_caps(d["sample_compared"], d["sample"]["alive"], d["n_random"], tag)
    for call, alive in ((CALLS["pdf"], alive_p), (CALLS["sample"], alive_s)):
        G = call.batch(ctx, to_dev(*call.inputs(d)), material=mid)
        for key, v in check(call, G, d, slice(None), alive, tag).items():
            WORST[key] = max(WORST[key], v)
    print(f"{tag}: excluded {r} random, {t} targeted; worst |G - R| / S so far: pdf {WORST['pdf']:.2e}  sample wi {WORST['wi']:.2e}  "
          f"params {WORST['params']:.2e}; pdf by output " + ", ".join(f"{k} {v:.2e}" for k, v in sref.PDF_WORST.items()))
    assert (~d["pdf"]["alive"]).sum() >= d["special"].sum() > 0 and alive_s.sum() >= 300


@pytest.mark.parametrize("case", [(1e-3, "gold"), (0.3, "aluminium"), (2.0, "spread_k")], ids=ggx.case_id)
def test_host_compiled_functions_agree_with_the_device(gpu, oracle, case, tmp_path_factory):
    """The same __host__ __device__ functions on both sides; they differ in the seeds of the reciprocals and square roots."""
    d = sref.case_data(oracle, *case, N_RANDOM)
    ctx, mid = gpu["ctx"], gpu["ids"][case]
    H = sref.run_harness(sref.build_harness(tmp_path_factory), tmp_path_factory.mktemp("sample_grad_gpu"), d["params"], d["wi"], d["wo"], d["u"],
                         d["gp"], d["go"])
    Dp = [cpu(x) for x in CALLS["pdf"].batch(ctx, to_dev(*CALLS["pdf"].inputs(d)), material=mid)]
    Ds = [cpu(x) for x in CALLS["sample"].batch(ctx, to_dev(*CALLS["sample"].inputs(d)), material=mid)]
    alive_p, alive_s = forward_alive(ctx, d, slice(None), mid)
    # host against device, per unit and per output, at the bar's own scale.  pdf: |g| |J_out| where the reference's J_out is stable, and
    # P's whole scale-free gradient on every live unit (ggx_sample_grad_reference.check_pdf_case); sample: the compared units
    P, S = d["pdf"], d["sample"]
    gp = np.where(P["alive"], d["gp"].astype(np.float64), 0.0)
    norm = lambda x: np.sqrt((x * x).sum(-1))
    with np.errstate(all="ignore"):
        li, lo = (np.where(P["alive"], norm(np.asarray(d[k], np.float64)), 1.0) for k in ("wi", "wo"))
    scales = {"pdf wi": np.abs(gp) * norm(P["Ji"]), "pdf wo": np.abs(gp) * norm(P["Jo"]), "pdf alpha": np.abs(gp * P["Ja"]),
              "sample wi": sref.contract_rows(S["Ji"], d["go"], S["alive"])[1], "sample params": sref.contract_params(S["Jp"], d["go"], S["alive"])[1]}
    rows = {"pdf wi": P["alive"] & P["stable_wi"], "pdf wo": P["alive"] & P["stable_wo"], "pdf alpha": P["alive"] & P["stable_alpha"],
            "sample wi": S["alive"] & d["sample_compared"], "sample params": S["alive"] & d["sample_compared"]}
    whole = np.sqrt((scales["pdf wi"] * li) ** 2 + (scales["pdf wo"] * lo) ** 2 + (scales["pdf alpha"] * d["params"][0]) ** 2)
    joint = np.zeros(len(whole))
    for name, h, dv in zip(scales, H, Dp + Ds):
        diff = np.abs(h.astype(np.float64) - dv.astype(np.float64))
        err = norm(diff) if name.endswith("wi") or name.endswith("wo") else diff
        use, sc = rows[name], scales[name]
        assert use.sum() >= (300 if name != "pdf wo" or case[0] != 1.0 else 0), name
        assert (err[use] <= sref.REL * sc[use]).all(), (name, int(np.flatnonzero(use)[np.argmax((err - sref.REL * sc)[use].reshape(int(use.sum()), -1).max(-1))]))
        if name.startswith("pdf"):
            joint += (err * {"pdf wi": li, "pdf wo": lo, "pdf alpha": d["params"][0]}[name]) ** 2
        # the two builds differ in the seeds of v_rcp / v_rsq, that is by ~1e-15 relative in an f64 result, amplified by the
        # conditioning of the unit (up to 1 / alpha = 1e3 here): a Float output component then rounds differently with probability
        # ~1e-12 / 2^-24 = 2e-5, ten components a unit: 2e-4 of the units at worst.  The floor leaves a factor of fifty
        identical = (bits(h) == bits(dv)).reshape(len(h), -1).all(-1)[use].mean() if use.any() else 1.0
        with np.errstate(all="ignore"):
            ratio = (err.reshape(len(h), -1) / sc.reshape(len(h), -1))[use]
        print(f"{ggx.case_id(case)} {name}: host and device bit-identical on {identical:.4f} of the units, worst difference "
              f"{np.nanmax(np.where(np.isfinite(ratio), ratio, 0.0)) if ratio.size else 0.0:.2e} S")
        assert identical >= 0.99, name
    assert (np.sqrt(joint)[P["alive"]] <= sref.REL * whole[P["alive"]]).all()
    check(CALLS["pdf"], H[:3], d, slice(None), alive_p, "host")
    check(CALLS["sample"], H[3:], d, slice(None), alive_s, "host")


def shape_selection(d, n):
    """the first units of the random block and the last of the targeted one (dead units with NaN / inf cotangents among them)"""
    sel = np.r_[0:(n + 1) // 2, len(d["wi"]) - n // 2:len(d["wi"])]
    assert len(sel) == n
    return sel


@BOTH
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 257))
def test_shapes_around_a_wave_and_a_block(gpu, oracle, call, n):
    case = (0.3, "gold")
    d = sref.case_data(oracle, *case, N_RANDOM)
    sel = shape_selection(d, n)
    ctx, mid = gpu["ctx"], gpu["ids"][case]
    alive = forward_alive(ctx, d, sel, mid)[call.kind == "sample"]
    G = call.batch(ctx, to_dev(*call.inputs(d, sel)), material=mid)
    check(call, G, d, sel, alive, f"n={n}")


@BOTH
def test_more_units_than_one_round_of_the_grid(gpu, oracle, call):
    case = (0.05, "aluminium")
    d = sref.case_data(oracle, *case, N_RANDOM)
    ctx, mid = gpu["ctx"], gpu["ids"][case]
    block, pdf_per_cu, sample_per_cu, sample_wi_per_cu = sref.launch_shape()
    one_round = block * max(pdf_per_cu, sample_per_cu, sample_wi_per_cu) * ctx.compute_units
    n, m = one_round + 37, len(d["wi"])
    sel = np.arange(n) % m                                       # the case tiled: the reference is reused
    G = call.batch(ctx, to_dev(*call.inputs(d, sel)), material=mid)
    once = call.batch(ctx, to_dev(*call.inputs(d)), material=mid)
    check(call, once, d, slice(None), forward_alive(ctx, d, slice(None), mid)[call.kind == "sample"], f"n={m}")
    # a unit's bits do not depend on n, the grid or its position
    for a, b in zip(G, once):
        assert same_bits(a, cpu(b)[sel])


@BOTH
def test_every_subset_of_null_outputs(gpu, oracle, call):
    case = (0.05, "spread_k")
    d = sref.case_data(oracle, *case, N_RANDOM)
    ctx, host, mid = gpu["ctx"], gpu["host"], gpu["ids"][case]
    ins = to_dev(*call.inputs(d))
    n = len(d["wi"])
    full = call.batch(ctx, ins, material=mid)
    batch, _ = call.symbols(ctx)
    k = len(call.outs)
    for keep in itertools.product((False, True), repeat=k):
        outs = sentinels(n, call.outs)
        ptrs = [o.data_ptr() if kept else None for o, kept in zip(outs, keep)]
        ctx.use_torch_stream()
        rc = batch(ctx._ctx, *(x.data_ptr() for x in ins), None, mid, n, *ptrs)
        ctx.synchronize()
        if not any(keep):
            assert rc == host.ERR_INVALID
        else:
            assert rc == 0
        for o, kept, whole, blank in zip(outs, keep, full, sentinels(n, call.outs, device=False)):
            assert same_bits(o, whole if kept else blank), keep
        if any(keep):
            want = tuple(name for name, kept in zip(call.names, keep) if kept)
            got = call.batch(ctx, ins, material=mid, want=want)
            for g, whole in zip((got,) if len(want) == 1 else got, (w for w, kept in zip(full, keep) if kept)):
                assert same_bits(g, whole), keep


@BOTH
def test_material_ids(gpu, oracle, call):
    import torch
    ctx = gpu["ctx"]
    cases = [(1e-3, "gold"), (0.05, "aluminium"), (0.3, "dielectric"), (2.0, "spread_k")]
    d = sref.case_data(oracle, 0.3, "gold", N_RANDOM)
    n = 4099
    sel = shape_selection(d, n)
    ins = to_dev(*call.finite_inputs(d, sel))
    choices = [gpu["ids"][c] for c in cases] + [gpu["table"], gpu["released"], ctx.material_count() + 5, -1]
    mat = np.array(choices, np.int32)[np.random.default_rng(7).integers(0, len(choices), n)]
    G = call.batch(ctx, ins, mat=to_dev(mat)[0])
    last = call.batch(ctx, ins, mat=to_dev(mat)[0], want=call.names[-1])
    assert same_bits(last, G[-1])
    for mid in choices[:4]:
        S = call.batch(ctx, ins, material=mid)
        mine = mat == mid
        assert mine.sum() > 100
        for a, b in zip(G, S):
            assert same_bits(cpu(a)[mine], cpu(b)[mine])
            assert float(b.abs().max()) > 0
    other = ~np.isin(mat, choices[:4])
    assert other.sum() > 100
    for a in G:
        assert not bits(cpu(a)[other]).any()
        assert torch.isfinite(a).all()


@BOTH
@pytest.mark.parametrize("with_ids", (False, True), ids=("single", "ids"))
def test_queue(gpu, oracle, call, with_ids):
    import torch
    ctx = gpu["ctx"]
    case = (0.3, "gold")
    d = sref.case_data(oracle, *case, N_RANDOM)
    cap = 1000
    sel = shape_selection(d, cap)
    ins = to_dev(*(call.finite_inputs(d, sel) if with_ids else call.inputs(d, sel)))
    kw = dict(material=gpu["ids"][case])
    if with_ids:
        choices = np.array([gpu["ids"][case], gpu["ids"][(0.05, "spread_k")], gpu["table"], -1], np.int32)
        kw = dict(mat=to_dev(choices[np.random.default_rng(8).integers(0, 4, cap)])[0])
    whole = [cpu(x) for x in call.batch(ctx, ins, **kw)]
    order = np.random.default_rng(9).permutation(cap).astype(np.int32)
    queue = to_dev(order)[0]
    blanks = sentinels(cap, call.outs, device=False)

    def expect(count):
        out = []
        for w, blank in zip(whole, blanks):
            e = blank.copy()
            e[order[:count]] = w[order[:count]]
            out.append(e)
        return out
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for c in (0, 1, 517, 5000):
        count.fill_(c)
        outs = sentinels(cap, call.outs)
        call.queue(ctx, ins, queue, count, out=outs, **kw)
        ctx.synchronize()
        for o, e in zip(outs, expect(min(c, cap))):
            assert same_bits(o, e), c
    # one capture (a single branch: one launch on one stream), replayed with another device-side count
    outs = sentinels(cap, call.outs)
    count.fill_(3)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        call.queue(ctx, ins, queue, count, out=outs, **kw)
    for c in (3, 700):
        for o in outs:
            o.fill_(SENTINEL)
        count.fill_(c)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, expect(c)):
            assert same_bits(o, e), c
    ctx.use_own_stream()


@BOTH
def test_host_arrays_in_chunks_and_pointer_mix(gpu, oracle, call):
    ctx, host = gpu["ctx"], gpu["host"]
    d = sref.case_data(oracle, 0.3, "aluminium", N_RANDOM)
    n = 3 * 4096 + 5
    sel = np.arange(n) % len(d["wi"])
    arrs = call.finite_inputs(d, sel)
    choices = np.array([gpu["ids"][(0.3, "aluminium")], gpu["ids"][(1e-2, "gold")], gpu["table"], ctx.material_count() + 5], np.int32)
    mat = choices[np.random.default_rng(10).integers(0, 4, n)]
    D = call.batch(ctx, to_dev(*arrs), mat=to_dev(mat)[0])
    chunk = ctx.get_option(host.OPT_HOST_CHUNK)
    ctx.set_option(host.OPT_HOST_CHUNK, 4096)
    try:
        H = call.batch(ctx, arrs, mat=mat)
        only_first = call.batch(ctx, arrs, mat=mat, want=call.names[0], out=sentinel(n, 3, device=False))
    finally:
        ctx.set_option(host.OPT_HOST_CHUNK, chunk)
    for h, dv in zip(H, D):
        assert isinstance(h, np.ndarray) and same_bits(h, dv)
        assert np.abs(h).max() > 0 and not h[np.isin(mat, choices[2:])].any()
    assert same_bits(only_first, D[0])
    with pytest.raises(host.MerlHipError) as e:
        call.batch(ctx, [to_dev(arrs[0])[0], arrs[1], arrs[2]], material=int(choices[0]))
    assert e.value.status == host.ERR_POINTER_MIX
    with pytest.raises(host.MerlHipError) as e:
        call.batch(ctx, to_dev(*arrs), material=int(choices[0]), out=sentinels(n, call.outs, device=False))
    assert e.value.status == host.ERR_POINTER_MIX


@BOTH
def test_errors_and_memory_report(gpu, oracle, call):
    import torch
    ctx, host = gpu["ctx"], gpu["host"]
    case = (0.3, "gold")
    d = sref.case_data(oracle, *case, N_RANDOM)
    n = 64
    ins = to_dev(*call.inputs(d, slice(0, n)))
    queue = torch.arange(n, dtype=torch.int32, device="cuda")
    count = torch.full((1,), n, dtype=torch.int32, device="cuda")
    for mid in (gpu["table"], gpu["released"], ctx.material_count() + 5, -1):
        with pytest.raises(host.MerlHipError) as e:
            call.batch(ctx, ins, material=mid)
        assert e.value.status == host.ERR_MATERIAL, mid
        with pytest.raises(host.MerlHipError) as e:
            call.queue(ctx, ins, queue, count, material=mid)
        assert e.value.status == host.ERR_MATERIAL, mid
    mid = gpu["ids"][case]
    outs = sentinels(n, call.outs)
    o = [x.data_ptr() for x in outs]
    batch, queued = call.symbols(ctx)
    p = [x.data_ptr() for x in ins]
    ctx.use_torch_stream()
    for missing in range(3):
        holes = [None if i == missing else x for i, x in enumerate(p)]
        assert batch(ctx._ctx, *holes, None, mid, n, *o) == host.ERR_INVALID
        assert queued(ctx._ctx, *holes, None, mid, queue.data_ptr(), count.data_ptr(), n, *o) == host.ERR_INVALID
    assert queued(ctx._ctx, *p, None, mid, None, count.data_ptr(), n, *o) == host.ERR_INVALID
    assert queued(ctx._ctx, *p, None, mid, queue.data_ptr(), count.data_ptr(), n, *([None] * len(o))) == host.ERR_INVALID
    before = ctx.memory_info()["workspace_bytes"]
    assert batch(ctx._ctx, *p, None, mid, 0, *o) == 0
    assert queued(ctx._ctx, *p, None, mid, queue.data_ptr(), count.data_ptr(), 0, *o) == 0
    ctx.synchronize()
    for x, blank in zip(outs, sentinels(n, call.outs, device=False)):
        assert same_bits(x, blank)
    call.batch(ctx, ins, material=mid, out=outs)
    call.queue(ctx, ins, queue, count, material=mid, out=outs)
    ctx.synchronize()
    assert ctx.memory_info()["workspace_bytes"] == before        # no workspace
    assert not same_bits(outs[0], sentinel(n, 3, device=False))


def test_autograd_wrappers(gpu, oracle):
    import torch
    from mitsuba_customization_amd import diff
    ctx = gpu["ctx"]
    case = (0.3, "gold")
    d = sref.case_data(oracle, *case, N_RANDOM)
    mid = gpu["ids"][case]
    # ---- pdf
    live = d["pdf"]["alive"]
    wi0, wo0, w = to_dev(d["wi"][live], d["wo"][live], d["gp"][live])
    Gi, Go, Ga = ctx.ggx_pdf_grad(wi0, wo0, w, material=mid)
    wi, wo = wi0.clone().requires_grad_(True), wo0.clone().requires_grad_(True)
    params = torch.tensor([np.float32(0.3), *ggx.METALS["gold"][0], *ggx.METALS["gold"][1]], dtype=torch.float64, requires_grad=True)
    p = diff.ggx_pdf(ctx, wi, wo, material=mid, params=params)
    assert same_bits(p.detach(), ctx.pdf(wi0, wo0, material=mid))
    (p * w).sum().backward()
    assert same_bits(wi.grad, Gi) and same_bits(wo.grad, Go)
    assert float(params.grad[0]) == float(Ga.double().sum(0)) and not params.grad[1:].any()          # the f64 sum of the per-unit array
    # only the gradient the graph asks for
    wi, wo = wi0.clone().requires_grad_(True), wo0.clone()
    seen = []
    real = ctx.ggx_pdf_grad
    ctx.ggx_pdf_grad = lambda *a, **kw: (seen.append(kw["want"]), real(*a, **kw))[1]
    try:
        (diff.ggx_pdf(ctx, wi, wo, material=mid) * w).sum().backward()
    finally:
        del ctx.ggx_pdf_grad
    assert seen == [("wi",)] and same_bits(wi.grad, Gi) and wo.grad is None
    # degree 0 in wi, through torch code in front of it and with material ids
    scale = torch.tensor(2.0, dtype=torch.float64, device="cuda", requires_grad=True)
    mat = torch.full((len(wi0),), mid, dtype=torch.int32, device="cuda")
    (diff.ggx_pdf(ctx, (wi0.double() * scale).float(), wo0, mat=mat) * w).sum().backward()
    total = float((Gi.double().norm(dim=1) * wi0.double().norm(dim=1)).sum())
    assert abs(float(scale.grad)) <= 1e-6 * total
    # ---- sample
    live = d["sample"]["alive"]
    wi0, u0, g = to_dev(d["wi"][live], d["u"][live], d["go"][live])
    Gi, Gp = ctx.ggx_sample_grad(wi0, u0, g, material=mid)
    wi = wi0.clone().requires_grad_(True)
    params = params.detach().clone().requires_grad_(True)
    out = diff.ggx_sample(ctx, wi, u0, material=mid, params=params)
    for a, b in zip(out, ctx.sample(wi0, u0, material=mid)):
        assert same_bits(a.detach(), b)
    ((out[0] * g[:, 0:3]).sum() + (out[1] * g[:, 3]).sum() + (out[2] * g[:, 4:7]).sum()).backward()
    assert same_bits(wi.grad, Gi)
    assert torch.equal(params.grad, Gp.double().sum(0).cpu())
    # a None incoming gradient is zeros in the packed cotangent; only grad_wi is issued
    g_dir = g.clone(); g_dir[:, 3:] = 0
    wi = wi0.clone().requires_grad_(True)
    seen = []
    real = ctx.ggx_sample_grad
    ctx.ggx_sample_grad = lambda *a, **kw: (seen.append(kw["want"]), real(*a, **kw))[1]
    try:
        (diff.ggx_sample(ctx, wi, u0, material=mid)[0] * g[:, 0:3]).sum().backward()
    finally:
        del ctx.ggx_sample_grad
    assert seen == [("wi",)] and same_bits(wi.grad, ctx.ggx_sample_grad(wi0, u0, g_dir, material=mid, want="wi"))
    # with ids: params.grad per material by index_add_
    other = gpu["ids"][(0.05, "spread_k")]
    mat_np = np.where(np.arange(len(wi0)) % 3 == 0, other, mid).astype(np.int32)
    mat = to_dev(mat_np)[0]
    pa = params.detach().clone().requires_grad_(True)
    pb = torch.tensor([np.float32(0.05), *ggx.METALS["spread_k"][0], *ggx.METALS["spread_k"][1]], dtype=torch.float64, requires_grad=True)
    out = diff.ggx_sample(ctx, wi0, u0, mat=mat, params={mid: pa, other: pb})
    ((out[0] * g[:, 0:3]).sum() + (out[1] * g[:, 3]).sum() + (out[2] * g[:, 4:7]).sum()).backward()
    rows = cpu(ctx.ggx_sample_grad(wi0, u0, g, mat=mat, want="params")).astype(np.float64)
    for t, m in ((pa, mid), (pb, other)):
        want = rows[mat_np == m].sum(0)
        assert np.abs(t.grad.numpy() - want).max() <= 1e-12 * np.abs(rows[mat_np == m]).sum(0).max()
    scale = torch.tensor(2.0, dtype=torch.float64, device="cuda", requires_grad=True)
    out = diff.ggx_sample(ctx, (wi0.double() * scale).float(), u0, material=mid)
    ((out[0] * g[:, 0:3]).sum() + (out[1] * g[:, 3]).sum() + (out[2] * g[:, 4:7]).sum()).backward()
    total = float((Gi.double().norm(dim=1) * wi0.double().norm(dim=1)).sum())
    assert abs(float(scale.grad)) <= 1e-6 * total


def test_fit_sampled_lobe_end_to_end(gpu):
    import torch
    from mitsuba_customization_amd import diff
    from tests.test_ggx_sample_grad_cpu import FIT_ALPHA_BOUND, FIT_ANGLE_BOUND
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import fit_sampled_lobe as fsl
    ctx = gpu["ctx"]
    mid = ctx.ggx(fsl.START[2], fsl.ETA, fsl.K)
    wi, _, u = ctx.generate_pairs(0xF17, 0, 1 << 12)
    r = fsl.rotation(torch.tensor(fsl.TRUTH[:2], dtype=torch.float64)).cuda()
    wi_w = wi.double() @ r
    x, history, errors, alphas = fsl.fit(lambda a, uu, p: diff.ggx_sample(ctx, a, uu, material=mid, params=p)[0], wi_w, u, iters=30)
    print(f"fit_sampled_lobe on the device: normal off by {errors[0]:.3e} -> {errors[-1]:.3e} rad, alpha off by {alphas[0]:.3e} -> "
          f"{alphas[-1]:.3e}; loss {history[0]:.3e} -> {history[-1]:.3e}")
    assert 0.09 <= errors[0] <= 0.11
    assert all(b <= a for a, b in zip(history, history[1:]))
    assert errors[-1] <= FIT_ANGLE_BOUND and alphas[-1] <= FIT_ALPHA_BOUND
