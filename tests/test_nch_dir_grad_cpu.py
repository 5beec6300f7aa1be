"""The direction gradient of eval_nch on n-channel tables (mrl_table_grad_dir_batch_nch / _queue_nch, include/merl_hip_diff_nch.h)
without a GPU: the C-channel Jacobian of tests/nch_dir_grad_reference.py is tied to the tested tref.jacobian on every 3-channel slice
of a table, the per-lane function the kernel runs (csrc/merl_nch_dir_grad.hpp, fast::nch_eval_dir_grad) is compiled for the host and
held to the project's bar — |G - R|_2 <= 1e-6 S per unit and side, S = sum_c |g_c| |J_c|_2, exact +0.0 on dead units, G == 0 where
S == 0, everything finite — on 1, 2, 4, 5, 8 and 32 channels, a standard and a full-azimuth table, kept negative texels, no cosine
factor, the nearest lookup and 'flat6' (a constant channel of 1000 in the first group, one of 1e-3 varying by 1e-6 of itself in the
second), the identities of the header are checked, the header and the library carry the two calls, and the compiled kernels use no
scratch and fit their launch shape.  The harness pads its bricks with 1e30: a padding channel that entered a sum
would fail every case whose channel count is not 1, 2 or a multiple of 4.

Measured here (host build), 8,192 random units + the targeted block per case, worst |G - R| / S over both sides: 4.68e-8 to 5.85e-8
over the eleven cases, flat6 (5.56e-8 / 5.73e-8) included: the rounding of the f32 output, 2^-24 sqrt(3) = 1.03e-7 at most; 0 random
units excused, 4 (standard form) or 9 of the 35 targeted ones; the 3-channel slices of the C-channel Jacobian equal tref.jacobian
bit for bit."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import nch_dir_grad_reference as nref
from tests import table_dir_grad_reference as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASE_IDS = [nref.case_id(c) for c in nref.CASES]
WORST = {"harness": 0.0}
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", [nref.CASES[3], nref.CASES[6], nref.CASES[7]], ids=[CASE_IDS[i] for i in (3, 6, 7)])
def test_c_channel_jacobian_equals_the_rgb_reference_on_every_three_channel_slice(oracle, case):
    """A channel's backward pass does not see the other channels: the slices must agree to the last bit."""
    d = nref.case_data(oracle, case)
    for c in range(d["n_ch"] - 2):
        Ji, Jo, val, alive, exc = tref.jacobian(d["table"][c:c + 3], d["wi"], d["wo"], d["param"], bool(d["lookup"]), bool(d["node"]), not d["no_cosine"])
        assert np.array_equal(alive, d["alive"]) and np.array_equal(exc, d["excused"])
        assert np.array_equal(Ji, d["Ji"][:, c:c + 3]) and np.array_equal(Jo, d["Jo"][:, c:c + 3]) and np.array_equal(val, d["val"][:, c:c + 3])
        assert np.abs(Ji).max() > 0 and np.abs(Jo).max() > 0
    assert d["excused"][:d["n_random"]].sum() == 0


# ------------------------------------------------------------------ the product's per-lane function on the host
@needs_hipcc
@pytest.mark.parametrize("case", nref.CASES, ids=CASE_IDS)
def test_per_lane_function_on_the_host_meets_the_bar(oracle, case, tmp_path_factory):
    d = nref.case_data(oracle, case)
    Gi, Go = nref.run_harness(nref.build_harness(tmp_path_factory), tmp_path_factory.mktemp("nch_dir_grad"), d)
    tag = nref.case_id(case)
    wi = nref.check_side(Gi, d["Ji"], d["g"], d["alive"], d["excused"], tag + " wi")
    wo = nref.check_side(Go, d["Jo"], d["g"], d["alive"], d["excused"], tag + " wo")
    WORST["harness"] = max(WORST["harness"], wi, wo)
    print(f"{tag}: worst |G - R| / S = {wi:.2e} (wi) {wo:.2e} (wo) (so far {WORST['harness']:.2e}); "
          f"{int(d['excused'].sum())} excused, {int(d['excused'][:d['n_random']].sum())} of them random")
    if not d["lookup"]:
        assert not Gi.any()                                          # nearest: grad_wi == 0 exactly
        assert not Go[:, :2].any() and np.abs(Go[:, 2]).max() > 0    # and grad_wo is along e_z
    else:
        assert np.abs(Gi).max() > 0
    assert (~d["alive"]).sum() == nref.N_DEAD_TARGETED and not np.isfinite(d["g"][~d["alive"]]).any()


@needs_hipcc
@pytest.mark.parametrize("case", [nref.CASES[3], nref.CASES[5], nref.CASES[8]], ids=[CASE_IDS[i] for i in (3, 5, 8)])
def test_identities(oracle, case, tmp_path_factory):
    """grad_wi . wi = 0 (degree 0 in wi); grad_wo . wo = sum_c g_c E_c with the cosine factor (Euler, degree 1 in the raw wo) and 0
    without.  G is the exact gradient rounded to Float, component by component: the dot product moves by at most
    sum_k 2^-24 |G_k w_k| <= 2^-24 |G| |w| = 6e-8 |G| |w|; the f64 arithmetic adds 1e-13.  E comes from the reference."""
    d = nref.case_data(oracle, case)
    Gi, Go = nref.run_harness(nref.build_harness(tmp_path_factory), tmp_path_factory.mktemp("nch_dir_grad_id"), d)
    held = d["alive"] & ~d["excused"]
    gE = d["g"][held].astype(np.float64) * d["val"][held]
    for G, w, side in ((Gi, d["wi"], "wi"), (Go, d["wo"], "wo")):
        G, w = G[held].astype(np.float64), w[held].astype(np.float64)
        want = gE.sum(-1) if (side == "wo" and not d["no_cosine"]) else np.zeros(len(G))
        slack = 1e-7 * np.sqrt((G * G).sum(-1)) * np.sqrt((w * w).sum(-1)) + 1e-12 * np.abs(gE).sum(-1)
        assert (np.abs((G * w).sum(-1) - want) <= slack).all(), side
        assert np.sqrt((G * G).sum(-1)).max() > 0


# ------------------------------------------------------------------ header, bindings, kernels
def test_header_declares_and_library_exports_the_nch_direction_gradient():
    import ctypes as C
    from mitsuba_customization_amd import build, host
    names = ("mrl_table_grad_dir_batch_nch", "mrl_table_grad_dir_queue_nch")
    text = open(os.path.join(ROOT, "include", "merl_hip_diff_nch.h")).read()
    assert re.search(r'#include\s+"merl_hip_diff_table.h"', text)
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = dict(re.findall(r"^[ \t]*int[ \t]+(mrl_\w+)[ \t]*\(([^()]*)\)[ \t]*;", code, flags=re.M))
    assert set(protos) == set(host.DIFF_NCH_ABI_SYMBOLS) == set(names)
    assert host.DIFF_NCH_ABI_SYMBOLS == names
    assert not set(host.DIFF_NCH_ABI_SYMBOLS) & (set(host.ABI_SYMBOLS) | set(host.FIT_ABI_SYMBOLS) | set(host.DIFF_ABI_SYMBOLS) | set(host.DIFF_TABLE_ABI_SYMBOLS))
    for other in ("merl_hip.h", "merl_hip_fit.h", "merl_hip_diff.h", "merl_hip_diff_table.h"):
        assert "_nch" not in "".join(re.findall(r"mrl_table_grad_dir\w*", re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)))
    for word in ("Euler", "1 / |w|", "Not offered", "renormalis", "DETERMINISM", "grad_values"):
        assert word in text
    build.build_lib()
    lib = host.load_library()

    def c_class(decl):
        if "*" in decl or "[" in decl:
            return "pointer"
        return {"int": "i32", "int32_t": "i32", "size_t": "u64"}[[w for w in re.findall(r"\w+", decl) if w != "const"][0]]

    def ctypes_class(t):
        return "pointer" if t is C.c_void_p else {C.c_int32: "i32", C.c_uint64: "u64"}[t]
    want = {names[0]: ["pointer"] * 5 + ["i32", "u64", "i32", "pointer", "pointer"],
            names[1]: ["pointer"] * 5 + ["i32", "pointer", "pointer", "u64", "i32", "pointer", "pointer"]}
    for name in names:
        assert hasattr(lib, name)
        assert [c_class(p) for p in protos[name].split(",")] == want[name]
        assert [ctypes_class(t) for t in getattr(lib, name).argtypes] == want[name]
    assert lib.mrl_table_grad_dir_batch_nch(None, None, None, None, None, 0, 4, 4, None, None) == -1            # no context: MRL_ERR_INVALID
    assert lib.mrl_table_grad_dir_queue_nch(None, None, None, None, None, 0, None, None, 4, 4, None, None) == -1


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


@needs_hipcc
def test_nch_direction_gradient_kernels_use_no_scratch_and_fit_their_launch_shape():
    import isa_round_trips as irt
    kernels = {k: v for k, v in _kernels(irt.compile_to_asm(nref.KERNEL_SOURCE)).items() if k.startswith("k_table_grad_dir_nch<")}
    want = {f"k_table_grad_dir_nch<{p}, {i}, {cpad}>" for p in ("false", "true") for i in ("false", "true") for cpad in (1, 2, 4)}
    assert want == set(kernels), sorted(kernels)
    for name, (scratch, vgprs) in sorted(kernels.items()):
        cpad = int(re.search(r", (\d)>$", name).group(1))
        block, per_cu = nref.launch_shape(cpad)                     # CPAD 1, 2: the calls of 1 and 2 channels; 4: of 4 .. 32
        assert block % 64 == 0 and per_cu >= 1
        assert scratch == 0, (name, scratch)
        # registers are allocated in granules of 8 out of 512 per lane and SIMD: the blocks the grid places on a compute unit
        # (block / 64 waves each, spread over 4 SIMDs) must all be resident
        waves_per_simd = min(8, 512 // ((vgprs + 7) // 8 * 8))
        print(f"{name}: {vgprs} VGPRs, {waves_per_simd} waves per SIMD, {per_cu} blocks per compute unit")
        assert per_cu * (block // 64) <= 4 * waves_per_simd, (name, vgprs)
