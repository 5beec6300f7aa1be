"""The direction gradient of the GGX conductor (mrl_ggx_grad_dir_batch / _queue, include/merl_hip_diff.h) without a GPU: the autograd
reference of tests/ggx_dir_grad_reference.py is shown to restate the model and to agree with central differences of it, the per-lane
function the kernel runs (csrc/merl_ggx_fast.hpp, fast::ggx_eval_dir_grad) is compiled for the host and held to the project's bar on
every case the GPU test runs, the header and the library carry the calls, the compiled kernels use no scratch, and
examples/fit_normal.py recovers a tilted normal with the reference standing in for the device.

Measured here (host build: the reciprocal and square-root seeds are the host's, the device's differ in the last bits): worst
|G - R| / S = 5.89e-8 over the 24 cases and both sides — the rounding of the f32 output; the torch restatement equals the numpy model
to 1.6e-15; central differences agree with autograd on 98.9 % of the live units in the worst case; fit_normal ends 3.5e-17 rad from
the truth (f64 reference data)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import ggx_dir_grad_reference as dref
from tests import ggx_reference as ggx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_UNITS = 4096
CASE_IDS = [ggx.case_id(c) for c in ggx.CASES]
WORST = {"harness": 0.0}


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", ggx.CASES, ids=CASE_IDS)
def test_torch_restatement_equals_the_numpy_model(oracle, case):
    d = dref.case_data(oracle, *case, N_UNITS)
    al, eta, k = d["params"]
    want = ggx.eval(al, eta, k, d["wi"][d["alive"]], d["wo"][d["alive"]])
    got = d["val"][d["alive"]]
    rel = np.abs(got - want) / np.abs(want)
    print(f"{ggx.case_id(case)}: torch vs numpy model, worst relative difference {rel.max():.1e}")
    assert d["alive"].sum() >= N_UNITS and (want > 0).all()
    assert (rel <= 1e-12).all()
    for J in (d["Ji"], d["Jo"]):
        assert np.isfinite(J).all()
        assert not J[~d["alive"]].any()


def _central_differences(al, eta, k, wi, wo, side):
    """d eval_c / d w by central differences of the numpy model, step 1e-4 min(alpha, 1, a_z, b_z) |w| per unit: [n, 3 channels, 3]"""
    wi, wo = np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    li, lo = np.sqrt((wi * wi).sum(-1)), np.sqrt((wo * wo).sum(-1))
    w, lw = (wi, li) if side == 0 else (wo, lo)
    step = 1e-4 * np.minimum(np.minimum(al, 1.0), np.minimum(wi[:, 2] / li, wo[:, 2] / lo)) * lw
    J = np.zeros((len(wi), 3, 3))
    for axis in range(3):
        hi, lo_ = w.copy(), w.copy()
        hi[:, axis] += step; lo_[:, axis] -= step
        e = [ggx.eval(al, eta, k, *((x, wo) if side == 0 else (wi, x))) for x in (hi, lo_)]
        J[:, :, axis] = (e[0] - e[1]) / (hi[:, axis] - lo_[:, axis])[:, None]
    return J


@pytest.mark.parametrize("case", ggx.CASES, ids=CASE_IDS)
def test_central_differences_agree_with_autograd(oracle, case):
    """A reference that is wrong cannot pass this: the step is fixed beforehand and the cap is a condition, not a measurement."""
    d = dref.case_data(oracle, *case, N_UNITS)
    al, eta, k = d["params"]
    alive = d["alive"]
    fractions = []
    for side, J in enumerate((d["Ji"], d["Jo"])):
        fd = _central_differences(al, eta, k, d["wi"][alive], d["wo"][alive], side)
        ref = J[alive]
        err = np.sqrt(((fd - ref) ** 2).sum(-1))
        agree = err <= 1e-5 * np.sqrt((ref * ref).sum(-1))
        fractions.append(agree.mean())
        assert agree.mean() >= 0.95, (side, agree.mean())
    print(f"{ggx.case_id(case)}: central differences within 1e-5 of autograd on {min(fractions):.4f} of the live units (worst side)")


# ------------------------------------------------------------------ the product's per-lane function on the host
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
@pytest.mark.parametrize("case", ggx.CASES, ids=CASE_IDS)
def test_per_lane_function_on_the_host_meets_the_bar(oracle, case, tmp_path_factory):
    d = dref.case_data(oracle, *case, N_UNITS)
    Gi, Go = dref.run_harness(dref.build_harness(tmp_path_factory), tmp_path_factory.mktemp("dir_grad"), d["params"], d["wi"], d["wo"], d["g"])
    tag = ggx.case_id(case)
    worst = max(dref.check_side(Gi, d["Ji"], d["g"], d["wi"], d["alive"], tag + " wi"),
                dref.check_side(Go, d["Jo"], d["g"], d["wo"], d["alive"], tag + " wo"))
    WORST["harness"] = max(WORST["harness"], worst)
    print(f"{tag}: worst |G - R| / S = {worst:.2e} (so far {WORST['harness']:.2e})")
    assert (~d["alive"]).sum() >= d["special"].sum() > 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_unnormalised_inputs_scale_with_the_inverse_length(oracle, tmp_path_factory):
    """The unnormalised units of the targeted block, and the same directions normalised in f64 and rounded to Float: scaling wi by s
    divides grad_wi by s and leaves grad_wo as it is.  The rounding of the normalised copy moves a direction by 6e-8 relative, and a
    gradient that changes by 1 / alpha per unit of direction by 6e-8 / alpha: the comparison is made at alpha = 0.3 and 1."""
    build = dref.build_harness(tmp_path_factory)
    for alpha in (0.3, 1.0):
        d = dref.case_data(oracle, alpha, "gold", N_UNITS)
        wi, wo = d["wi"].astype(np.float64), d["wo"].astype(np.float64)
        li, lo = np.sqrt((wi * wi).sum(-1)), np.sqrt((wo * wo).sum(-1))
        with np.errstate(all="ignore"):
            scaled = d["alive"] & ((np.abs(li - 1) > 0.5) | (np.abs(lo - 1) > 0.5))
        assert scaled.sum() == 12
        li, lo = li[scaled][:, None], lo[scaled][:, None]
        raw = (d["wi"][scaled], d["wo"][scaled])
        unit = ((wi[scaled] / li).astype(np.float32), (wo[scaled] / lo).astype(np.float32))
        g = d["g"][scaled]
        tmp = tmp_path_factory.mktemp("dir_grad_scale")
        Gr, Gu = dref.run_harness(build, tmp, d["params"], *raw, g), dref.run_harness(build, tmp, d["params"], *unit, g)
        for side, length in enumerate((li, lo)):
            a, b = Gr[side].astype(np.float64) * length, Gu[side].astype(np.float64)
            assert (np.abs(a - b) <= 1e-5 * np.sqrt((b * b).sum(-1))[:, None]).all(), (alpha, side)
            assert (np.sqrt((b * b).sum(-1)) > 0).all()


# ------------------------------------------------------------------ header, bindings, kernels
def test_header_declares_and_library_exports_the_direction_gradient():
    import ctypes as C
    from mitsuba_customization_amd import build, host
    text = open(os.path.join(ROOT, "include", "merl_hip_diff.h")).read()
    assert re.search(r'#include\s+"merl_hip.h"', text)
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = dict(re.findall(r"^[ \t]*int[ \t]+(mrl_\w+)[ \t]*\(([^()]*)\)[ \t]*;", code, flags=re.M))
    assert set(protos) == set(host.DIFF_ABI_SYMBOLS) == {"mrl_ggx_grad_dir_batch", "mrl_ggx_grad_dir_queue"}
    assert host.DIFF_ABI_SYMBOLS == ("mrl_ggx_grad_dir_batch", "mrl_ggx_grad_dir_queue")
    assert not set(host.DIFF_ABI_SYMBOLS) & (set(host.ABI_SYMBOLS) | set(host.FIT_ABI_SYMBOLS))
    for word in ("orthogonal", "1 / |w|", "Not offered"):
        assert word in text
    build.build_lib()
    lib = host.load_library()

    def c_class(decl):
        if "*" in decl or "[" in decl:
            return "pointer"
        return {"int": "i32", "int32_t": "i32", "size_t": "u64"}[[w for w in re.findall(r"\w+", decl) if w != "const"][0]]

    def ctypes_class(t):
        return "pointer" if t is C.c_void_p else {C.c_int32: "i32", C.c_uint64: "u64"}[t]
    want = {"mrl_ggx_grad_dir_batch": ["pointer"] * 5 + ["i32", "u64", "pointer", "pointer"],
            "mrl_ggx_grad_dir_queue": ["pointer"] * 5 + ["i32", "pointer", "pointer", "u64", "pointer", "pointer"]}
    for name in host.DIFF_ABI_SYMBOLS:
        assert hasattr(lib, name)
        assert [c_class(p) for p in protos[name].split(",")] == want[name]
        assert [ctypes_class(t) for t in getattr(lib, name).argtypes] == want[name]
    assert lib.mrl_ggx_grad_dir_batch(None, None, None, None, None, 0, 4, None, None) == -1            # no context: MRL_ERR_INVALID
    assert lib.mrl_ggx_grad_dir_queue(None, None, None, None, None, 0, None, None, 4, None, None) == -1


def _kernels(asm):
    """{demangled kernel name: scratch bytes per lane}"""
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    names = subprocess.run(["c++filt"] + [b[0] for b in blocks], capture_output=True, text=True).stdout.splitlines()
    out = {}
    for (_, body), d in zip(blocks, names):
        d = d.replace("mrl::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        out[d] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                  int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)))
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_direction_gradient_kernels_use_no_scratch_and_fit_their_launch_shape():
    import isa_round_trips as irt
    kernels = _kernels(irt.compile_to_asm(dref.KERNEL_SOURCE))
    want = {f"k_ggx_grad_dir<{p}, {i}>" for p in ("false", "true") for i in ("false", "true")}
    assert want <= set(kernels), sorted(kernels)
    block, per_cu = dref.launch_shape()
    assert block % 64 == 0 and per_cu >= 1
    for name, (scratch, vgprs) in kernels.items():
        assert scratch == 0, (name, scratch)
        # registers are allocated in granules of 8 out of 512 per lane and SIMD: the blocks the grid places on a compute unit
        # (block / 64 waves each, spread over 4 SIMDs) must all be resident
        waves_per_simd = min(8, 512 // ((vgprs + 7) // 8 * 8))
        print(f"{name}: {vgprs} VGPRs, {waves_per_simd} waves per SIMD")
        assert per_cu * (block // 64) <= 4 * waves_per_simd, (name, vgprs)


# ------------------------------------------------------------------ examples/fit_normal.py
def test_fit_normal_recovers_a_tilted_normal_from_reference_data(oracle):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import fit_normal
    al, eta, k = ggx.f32_params(0.3, "gold")

    class Reference(torch.autograd.Function):
        """stands in for diff.ggx_eval: forward the torch model, backward the reference Jacobians"""
        @staticmethod
        def forward(ctx, wi, wo):
            Ji, Jo, val, _ = dref.jacobian(al, eta, k, wi.detach().numpy(), wo.detach().numpy())
            ctx.J = (torch.from_numpy(Ji), torch.from_numpy(Jo))
            return torch.from_numpy(val)

        @staticmethod
        def backward(ctx, g):
            return tuple(torch.einsum("uc,uck->uk", g, J) for J in ctx.J)

    wi, wo, _ = oracle.generate_pairs(0xF17, 0, 2048)
    wi_w, wo_w = fit_normal.world_pairs(np.asarray(wi, np.float64), np.asarray(wo, np.float64), fit_normal.TRUTH)
    angles, history, errors = fit_normal.fit(Reference.apply, torch.from_numpy(wi_w), torch.from_numpy(wo_w), dtype=torch.float64)
    print(f"fit_normal: angle error {errors[0]:.3e} -> {errors[-1]:.3e} rad; loss {history[0]:.3e} -> {history[-1]:.3e}")
    assert 0.19 <= errors[0] <= 0.21
    assert errors[-1] <= 1e-3 * errors[0]
    assert all(b <= a for a, b in zip(history, history[1:]))
