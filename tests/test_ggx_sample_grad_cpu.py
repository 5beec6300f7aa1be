"""The gradients of pdf and sample on GGX conductors (include/merl_hip_diff_sample.h) without a GPU: the autograd reference of
tests/ggx_sample_grad_reference.py is tied to the numpy model and to the oracle's sampler, shown to agree with central differences of
itself and to satisfy the chain identity between the two gradients; the per-lane functions the kernels run (csrc/merl_ggx_fast.hpp,
fast::ggx_pdf_grad and fast::ggx_sample_grad) are compiled for the host and held to the project's bar on every case the GPU test runs;
the header and the library carry the calls; the compiled kernels use no scratch and fit their launch shapes; and
examples/fit_sampled_lobe.py recovers a tilted normal and alpha with the reference standing in for the device.

Measured here (host build: the reciprocal and square-root seeds are the host's, the device's differ in the last bits), 4,096 random
units + the targeted block of each of the 24 cases: worst |G - R| / S for the pdf gradient, each output at its own scale, 5.93e-8
(wi), 2.96e-7 (wo, on targeted units near the mirror direction) and 5.95e-8 (alpha), 5.90e-8 at the scale of P's whole gradient;
5.87e-8 for the sample gradient in wi and 5.95e-8 in the parameters — the rounding of the f32 outputs; 0 random and 0 targeted sample
units excluded by the stability rule in every case; pdf outputs at the reference's rounding (held to the whole-gradient bar only): no
random unit except dP / d wo at alpha = 1, 160 - 168 (wo) and 23 - 41 (wi) of the 378 targeted units; the restatement's pdf equals
the numpy model to 1e-12; central differences agree on 99.87 % (wi at alpha = 1e-3) to 100 % of the units."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import ggx_reference as ggx
from tests import ggx_sample_grad_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_UNITS = 4096
CASE_IDS = [ggx.case_id(c) for c in ggx.CASES]
WORST = {"pdf": 0.0, "wi": 0.0, "params": 0.0}


# ------------------------------------------------------------------ the reference against the model and the oracle
@pytest.mark.parametrize("case", ggx.CASES, ids=CASE_IDS)
def test_restatement_equals_the_numpy_pdf_and_the_oracle_sampler(oracle, case):
    d = sref.case_data(oracle, *case, N_UNITS)
    al, eta, k = d["params"]
    P, S = d["pdf"], d["sample"]
    alive = P["alive"]
    want = ggx.pdf(al, d["wi"][alive], d["wo"][alive])
    assert alive.sum() >= N_UNITS // 2 and (want > 0).all()
    assert (np.abs(P["val"][alive] - want) <= 1e-12 * want).all()
    # the sampler: the oracle's accept / reject outside the band, its direction to a Float ulp, its pdf and weight inside the envelope
    # of the Float direction it returns
    G = oracle.OracleGgx(al, eta, k)
    with np.errstate(all="ignore"):
        wo2, pdf2, w = G.sample(d["wi"], d["u"])
    acc = pdf2 > 0
    clear = ~S["band"]
    assert np.array_equal(acc[clear], S["alive"][clear])
    assert clear.sum() >= len(clear) - 4
    both = acc & S["alive"]
    assert both.sum() >= 300
    out = S["val"][both, :3]
    assert (np.abs(wo2[both] - out) <= 2.0 ** -23 * np.abs(out) + 1e-9).all()

    def ratio(a, b):
        return G.eval(a, b).astype(np.float64) / G.pdf(a, b).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        p_lo, p_hi, w_lo, w_hi = ggx.envelope(G.pdf, ratio, d["wi"][both], wo2[both])
    assert ggx.inside(S["val"][both, 3], p_lo, p_hi).all()
    assert ggx.inside(S["val"][both, 4:], w_lo, w_hi).all()
    for J in (P["Ji"], P["Jo"], P["Ja"], S["Ji"], S["Jp"]):
        assert np.isfinite(J).all()
    assert not S["Ji"][~S["alive"]].any() and not S["Jp"][~S["alive"]].any() and not P["Ji"][~alive].any()


@pytest.mark.parametrize("case", ggx.CASES, ids=CASE_IDS)
def test_the_caps_on_excluded_units_hold(oracle, case):
    d = sref.case_data(oracle, *case, N_UNITS)
    r, t = sref.excluded_within_caps(d["sample_compared"], d["sample"]["alive"], d["n_random"], ggx.case_id(case))
    print(f"{ggx.case_id(case)}: {r} random and {t} of {len(d['wi']) - d['n_random']} targeted units excluded")
    # pdf: where an output is held to the whole-gradient bar only.  Among the random units that is dP / d wo at alpha = 1 (D is constant:
    # the true derivative is 0) and nothing else; in the targeted block the exact mirror pairs and their like
    P, nr = d["pdf"], d["n_random"]
    counts = {k: (int((P["alive"] & ~P["stable_" + k])[:nr].sum()), int((P["alive"] & ~P["stable_" + k])[nr:].sum())) for k in ("wi", "wo", "alpha")}
    print(f"{ggx.case_id(case)}: pdf outputs at the reference's rounding (random, targeted): {counts}")
    assert counts["wi"][0] == 0 and counts["alpha"] == (0, 0)
    assert counts["wo"][0] == (int(P["alive"][:nr].sum()) if case[0] == 1.0 else 0)


@pytest.mark.parametrize("case", [c for c in ggx.CASES if c[1] == "gold"], ids=[ggx.case_id(c) for c in ggx.CASES if c[1] == "gold"])
def test_central_differences_agree_with_autograd(oracle, case):
    """A reference that is wrong cannot pass this: the steps are fixed beforehand and the cap is a condition, not a measurement.  The
    branch of the base point is held, as the gradient holds it."""
    d = sref.case_data(oracle, *case, N_UNITS)
    al, eta, k = d["params"]
    S = d["sample"]
    use = S["alive"] & d["sample_compared"]
    wi, u = d["wi"][use].astype(np.float64), d["u"][use]
    length = np.sqrt((wi * wi).sum(-1))
    step = 1e-5 * np.minimum(min(al, 1.0), wi[:, 2] / length) * length
    fd = np.zeros((len(wi), 7, 3))
    same = np.ones(len(wi), bool)
    for axis in range(3):
        hi, lo = wi.copy(), wi.copy()
        hi[:, axis] += step; lo[:, axis] -= step
        (vh, ah), (vl, a_l) = (sref.sample_forward(d["params"], x, u, branch_of=wi) for x in (hi, lo))
        fd[:, :, axis] = (vh - vl) / (hi[:, axis] - lo[:, axis])[:, None]
        same &= ah & a_l
    ref = S["Ji"][use]
    err = np.sqrt(((fd - ref) ** 2).sum((1, 2)))
    agree = (err <= 1e-4 * np.sqrt((ref * ref).sum((1, 2))))[same]
    da = 1e-6 * al
    vh, ah = sref.sample_forward((al + da, eta, k), wi, u, branch_of=wi)
    vl, a_l = sref.sample_forward((al - da, eta, k), wi, u, branch_of=wi)
    both = ah & a_l
    ref_a = S["Jp"][use][:, :, 0]
    err_a = np.sqrt((((vh - vl) / (2 * da) - ref_a) ** 2).sum(-1))
    agree_a = (err_a <= 1e-4 * np.sqrt((ref_a * ref_a).sum(-1)))[both]
    print(f"{ggx.case_id(case)}: central differences within 1e-4 of autograd on {agree.mean():.4f} (wi) and {agree_a.mean():.4f} (alpha) of the units")
    assert same.sum() >= 0.9 * len(wi) and both.sum() >= 0.9 * len(wi)
    # measured: 0.9987 (wi at alpha = 1e-3, where the step meets the lobe's curvature) and 1.0000 everywhere else
    assert agree.mean() >= 0.995 and agree_a.mean() >= 0.999
    # eta and k of one channel each (they enter through the weight of that channel only), relative step 1e-6
    for column, (ch, which) in ((1 + 1, (1, "eta")), (4 + 2, (2, "k"))):
        base = (eta, k)[which == "k"][ch]
        h = 1e-6 * base
        moved = []
        for sign in (1.0, -1.0):
            e2, k2 = list(eta), list(k)
            (e2 if which == "eta" else k2)[ch] = base + sign * h
            moved.append(sref.sample_forward((al, e2, k2), wi, u, branch_of=wi)[0])
        fd_p = (moved[0] - moved[1]) / (2 * h)
        ref_p = S["Jp"][use][:, :, column]
        assert not ref_p[:, :4].any() and not ref_p[:, [c for c in (4, 5, 6) if c != 4 + ch]].any()      # the weight of that channel only
        err_p = np.abs(fd_p - ref_p).max(-1)
        agree_p = err_p <= 1e-4 * np.abs(ref_p).max(-1)
        print(f"{ggx.case_id(case)}: d / d {which}[{ch}] by central differences within 1e-4 of autograd on {agree_p.mean():.4f} of the units")
        assert np.abs(ref_p).max() > 0 and agree_p.mean() >= 0.999


@pytest.mark.parametrize("case", [(0.05, "gold"), (0.3, "aluminium"), (1.0, "spread_k")], ids=["a0.05-gold", "a0.3-aluminium", "a1-spread_k"])
def test_chain_identity_between_the_two_gradients(oracle, case):
    """d p' / d wi = dP / d wi + dP / d wo . d wo' / d wi at wo = wo', and d p' / d alpha likewise: the sampler's pdf IS pdf() of what it
    returns.  Both sides are the reference's own."""
    d = sref.case_data(oracle, *case, N_UNITS)
    S = d["sample"]
    use = S["alive"] & d["sample_compared"]
    wi = d["wi"][use].astype(np.float64)
    wo = S["val"][use, :3]
    P = sref.pdf_jacobian(d["params"][0], wi, wo)
    assert P["alive"].all()
    assert (np.abs(P["val"] - S["val"][use, 3]) <= 1e-10 * P["val"]).all()
    Ji, Jp = S["Ji"][use], S["Jp"][use]
    lhs = Ji[:, 3]
    rhs = P["Ji"] + np.einsum("uk,ukj->uj", P["Jo"], Ji[:, :3])
    scale = np.sqrt((P["Ji"] ** 2).sum(-1)) + np.sqrt((P["Jo"] ** 2).sum(-1)) * np.sqrt((Ji[:, :3] ** 2).sum((1, 2)))
    assert (np.sqrt(((lhs - rhs) ** 2).sum(-1)) <= 1e-8 * scale).all()
    rhs_a = P["Ja"] + np.einsum("uk,uk->u", P["Jo"], Jp[:, :3, 0])
    scale_a = np.abs(P["Ja"]) + np.sqrt((P["Jo"] ** 2).sum(-1)) * np.sqrt((Jp[:, :3, 0] ** 2).sum(-1))
    assert (np.abs(Jp[:, 3, 0] - rhs_a) <= 1e-8 * scale_a).all()


# ------------------------------------------------------------------ the product's per-lane functions on the host
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
@pytest.mark.parametrize("case", ggx.CASES, ids=CASE_IDS)
def test_per_lane_functions_on_the_host_meet_the_bar(oracle, case, tmp_path_factory):
    d = sref.case_data(oracle, *case, N_UNITS)
    out = sref.run_harness(sref.build_harness(tmp_path_factory), tmp_path_factory.mktemp("sample_grad"), d["params"], d["wi"], d["wo"], d["u"],
                           d["gp"], d["go"])
    tag = ggx.case_id(case)
    worst = {"pdf": sref.check_pdf_case(d, out[0], out[1], out[2], d["pdf"]["alive"], tag),
             "wi": sref.check_sample_case(d, out[3], None, d["sample"]["alive"], tag),
             "params": sref.check_sample_case(d, None, out[4], d["sample"]["alive"], tag)}
    for key, v in worst.items():
        WORST[key] = max(WORST[key], v)
    print(f"{tag}: worst |G - R| / S  pdf {worst['pdf']:.2e}  sample wi {worst['wi']:.2e}  params {worst['params']:.2e}   (so far "
          f"{WORST['pdf']:.2e} {WORST['wi']:.2e} {WORST['params']:.2e}; pdf by output " + ", ".join(f"{k} {v:.2e}" for k, v in sref.PDF_WORST.items()) + ")")
    assert (~d["pdf"]["alive"]).sum() >= d["special"].sum() > 0
    assert d["sample"]["alive"].sum() >= 300


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_unnormalised_wi_scales_the_gradient_with_the_inverse_length(oracle, tmp_path_factory):
    """wi scaled by a power of two: the normalised direction has the same bits, so grad_wi is divided by the scale exactly and every
    other output keeps its bits."""
    build = sref.build_harness(tmp_path_factory)
    d = sref.case_data(oracle, 0.3, "gold", N_UNITS)
    tmp = tmp_path_factory.mktemp("sample_grad_scale")
    base = sref.run_harness(build, tmp, d["params"], d["wi"], d["wo"], d["u"], d["gp"], d["go"])
    with np.errstate(all="ignore"):
        scaled = sref.run_harness(build, tmp, d["params"], d["wi"] * np.float32(4), d["wo"], d["u"], d["gp"], d["go"])
    fin = np.isfinite(d["wi"]).all(-1)
    for a, b in ((base[0], scaled[0]), (base[3], scaled[3])):
        assert np.array_equal((a[fin] / np.float32(4)).view(np.uint32), b[fin].view(np.uint32))
    for a, b in ((base[1], scaled[1]), (base[2], scaled[2]), (base[4], scaled[4])):
        assert np.array_equal(a[fin].view(np.uint32), b[fin].view(np.uint32))
    assert np.abs(base[3]).max() > 0 and np.abs(base[4]).max() > 0


# ------------------------------------------------------------------ header, bindings, kernels
def test_header_declares_and_library_exports_the_four_calls():
    import ctypes as C
    from mitsuba_customization_amd import build, host
    text = open(os.path.join(ROOT, "include", "merl_hip_diff_sample.h")).read()
    assert re.search(r'#include\s+"merl_hip.h"', text)
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = re.findall(r"^[ \t]*int[ \t]+(mrl_\w+)[ \t]*\(([^()]*)\)[ \t]*;", code, flags=re.M)
    names = ("mrl_ggx_pdf_grad_batch", "mrl_ggx_pdf_grad_queue", "mrl_ggx_sample_grad_batch", "mrl_ggx_sample_grad_queue")
    assert tuple(name for name, _ in protos) == host.DIFF_SAMPLE_ABI_SYMBOLS == names
    protos = dict(protos)
    others = [getattr(host, name) for name in dir(host) if name.endswith("ABI_SYMBOLS") and name != "DIFF_SAMPLE_ABI_SYMBOLS"]
    assert len(others) >= 12 and not set(names) & set().union(*map(set, others))
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "merl_hip_diff_sample.h":
            # no other header DECLARES them (merl_hip_diff.h points here in a comment)
            plain = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
            assert not any(re.search(r"\b%s\b" % name, plain) for name in names), other
    for word in ("orthogonal", "1 / |w|", "Not offered", "gradients in u", "tables and RGL", "device groups", "one-unit paths", "second derivatives",
                 "DETERMINISM", "held fixed"):
        assert word in text, word
    build.build_lib()
    lib = host.load_library()

    def c_class(decl):
        if "*" in decl or "[" in decl:
            return "pointer"
        return {"int": "i32", "int32_t": "i32", "size_t": "u64"}[[w for w in re.findall(r"\w+", decl) if w != "const"][0]]

    def ctypes_class(t):
        return "pointer" if t is C.c_void_p else {C.c_int32: "i32", C.c_uint64: "u64"}[t]
    want = {"mrl_ggx_pdf_grad_batch": ["pointer"] * 5 + ["i32", "u64"] + ["pointer"] * 3,
            "mrl_ggx_pdf_grad_queue": ["pointer"] * 5 + ["i32", "pointer", "pointer", "u64"] + ["pointer"] * 3,
            "mrl_ggx_sample_grad_batch": ["pointer"] * 5 + ["i32", "u64"] + ["pointer"] * 2,
            "mrl_ggx_sample_grad_queue": ["pointer"] * 5 + ["i32", "pointer", "pointer", "u64"] + ["pointer"] * 2}
    for name in names:
        assert hasattr(lib, name)
        assert [c_class(p) for p in protos[name].split(",")] == want[name]
        assert [ctypes_class(t) for t in getattr(lib, name).argtypes] == want[name]
    assert {host._CALLS[f, m][0] for f in ("batch", "queue") for m in ("ggx_pdf_grad", "ggx_sample_grad")} == set(names)
    assert lib.mrl_ggx_pdf_grad_batch(None, None, None, None, None, 0, 4, None, None, None) == -1            # no context: MRL_ERR_INVALID
    assert lib.mrl_ggx_pdf_grad_queue(None, None, None, None, None, 0, None, None, 4, None, None, None) == -1
    assert lib.mrl_ggx_sample_grad_batch(None, None, None, None, None, 0, 4, None, None) == -1
    assert lib.mrl_ggx_sample_grad_queue(None, None, None, None, None, 0, None, None, 4, None, None) == -1


def _kernels(asm):
    """{demangled kernel name: (scratch bytes per lane, VGPRs)}"""
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    names = subprocess.run(["c++filt"] + [b[0] for b in blocks], capture_output=True, text=True).stdout.splitlines()
    out = {}
    for (_, body), d in zip(blocks, names):
        d = d.replace("mrl::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        out[d] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                  int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)))
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_kernels_use_no_scratch_and_fit_their_launch_shapes():
    import isa_round_trips as irt
    kernels = _kernels(irt.compile_to_asm(sref.KERNEL_SOURCE))
    flags = ("false", "true")
    want = {f"k_ggx_pdf_grad<{p}, {i}>" for p in flags for i in flags} | {f"k_ggx_sample_grad<{p}, {i}, {w}>" for p in flags for i in flags for w in flags}
    assert want == set(kernels), sorted(kernels)
    block, pdf_per_cu, sample_per_cu, sample_wi_per_cu = sref.launch_shape()
    assert block % 64 == 0 and min(pdf_per_cu, sample_per_cu, sample_wi_per_cu) >= 1
    for name, (scratch, vgprs) in sorted(kernels.items()):
        assert scratch == 0, (name, scratch)
        per_cu = pdf_per_cu if "pdf" in name else (sample_per_cu if name.endswith("true>") else sample_wi_per_cu)
        # registers are allocated in granules of 8 out of 512 per lane and SIMD: the blocks the grid places on a compute unit
        # (block / 64 waves each, spread over 4 SIMDs) must all be resident
        waves_per_simd = min(8, 512 // ((vgprs + 7) // 8 * 8))
        print(f"{name}: {vgprs} VGPRs, {waves_per_simd} waves per SIMD, {per_cu} blocks per compute unit")
        assert per_cu * (block // 64) <= 4 * waves_per_simd, (name, vgprs)


# ------------------------------------------------------------------ examples/fit_sampled_lobe.py
# 10 x what the CPU run below ends at — where that is above the resolution of the Float data: the local directions and alpha reach the
# sampler rounded to Float (2^-24 relative), so an end point closer to the truth than that is a coincidence of the run, not a property
# of the fit, and the bound is 10 x 2^-24 (x alpha) there.  tests/test_gpu_ggx_sample_grad.py holds the device to the same two numbers.
FIT_ANGLE_BOUND = 10 * max(5.502e-18, 2.0 ** -24)             # rad: 5.96e-7
FIT_ALPHA_BOUND = 10 * max(2.156e-8, 0.3 * 2.0 ** -24)        # 2.16e-7


def test_fit_sampled_lobe_recovers_tilt_and_alpha_from_reference_data(oracle):
    """Measured on the reference (Float directions, values and parameters as on the device, 1,024 units, 30 iterations): the normal
    starts 0.100 rad and alpha 0.1 off; they end 5.502e-18 rad and 2.156e-8 off, the loss falls from 79.3 to exactly 0 and never rises."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import fit_sampled_lobe as fsl

    class Reference(torch.autograd.Function):
        """stands in for diff.ggx_sample's first result: forward the torch model, backward the reference Jacobians"""
        @staticmethod
        def forward(ctx, wi, u, params):
            p = [float(np.float32(v)) for v in params.detach().tolist()]         # the material holds Float parameters
            J = sref.sample_jacobian((p[0], p[1:4], p[4:7]), wi.detach().numpy(), u.numpy())
            ctx.J = (torch.from_numpy(J["Ji"][:, :3]), torch.from_numpy(J["Jp"][:, :3]))
            return torch.from_numpy(J["val"][:, :3].astype(np.float32))          # Float, as the device returns it

        @staticmethod
        def backward(ctx, g):
            g = g.to(torch.float64)
            return torch.einsum("uj,ujk->uk", g, ctx.J[0]).to(torch.float32), None, torch.einsum("uj,ujp->p", g, ctx.J[1])

    wi, _, u = oracle.generate_pairs(0xF17, 0, 1024)
    r = fsl.rotation(torch.tensor(fsl.TRUTH[:2], dtype=torch.float64)).numpy()
    wi_w = torch.from_numpy(np.asarray(wi, np.float64) @ r)
    x, history, errors, alphas = fsl.fit(Reference.apply, wi_w, torch.from_numpy(np.asarray(u, np.float32)), iters=30)
    print(f"fit_sampled_lobe: normal off by {errors[0]:.3e} -> {errors[-1]:.3e} rad, alpha off by {alphas[0]:.3e} -> {alphas[-1]:.3e}; "
          f"loss {history[0]:.3e} -> {history[-1]:.3e}")
    assert 0.09 <= errors[0] <= 0.11 and abs(alphas[0] - 0.1) < 1e-12
    assert all(b <= a for a, b in zip(history, history[1:]))
    assert errors[-1] <= FIT_ANGLE_BOUND and alphas[-1] <= FIT_ALPHA_BOUND
    assert math.isfinite(history[-1])
