"""The gradient of eval_spectral in the spectra of spectral RGL materials (include/merl_hip_fit_rgl_spectral.h) without
a GPU: the header against the library's symbols, the layout function, the per-lane functions and the fold compiled for the host (and
once more under the host sanitizers) against the autograd reference of tests/rgl_spectral_values_grad_reference.py, the fold's record ->
texel map, the factors of a 3-node file that holds an RGB file's arrays against rgl::values_grad_unit, wavelengths on and beyond the
nodes, and the compiled kernels' metadata.

Measured on the host, worst |G - R| / S per case, bricks + fold and plain form alike, MASK 0 and the file's own MASK alike — the two
have the same bits — (the bar is 1e-6): iso W = 4 4.5e-9, aniso 2.7e-9, phi_only 2.4e-9, iso W = 7 8.5e-9, iso on its own nodes
7.3e-9: what eval's own f64 building blocks leave in the cell fractions next to torch's libm."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import rgl_spectral_dir_grad_reference as sref
from tests import rgl_spectral_values_grad_reference as vref

ROOT = vref.ROOT


def test_header_declares_and_library_exports_the_spectral_values_calls():
    import ctypes as C
    from mitsuba_customization_amd import build, host
    text = open(os.path.join(ROOT, "include", "merl_hip_fit_rgl_spectral.h")).read()
    assert re.search(r'#include\s+"merl_hip.h"', text)
    assert re.search(r"#define\s+MRL_RGL_SPECTRAL_GRAD_MAX_TARGETS\s+16\b", text) and host.RGL_SPECTRAL_GRAD_MAX_TARGETS == 16
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = dict(re.findall(r"^[ \t]*int[ \t]+(mrl_\w+)[ \t]*\(([^()]*)\)[ \t]*;", code, flags=re.M))
    assert set(protos) == set(host.FIT_RGL_SPECTRAL_ABI_SYMBOLS) and len(host.FIT_RGL_SPECTRAL_ABI_SYMBOLS) == 5
    others = (host.ABI_SYMBOLS, host.FIT_ABI_SYMBOLS, host.DIFF_ABI_SYMBOLS, host.DIFF_TABLE_ABI_SYMBOLS, host.DIFF_NCH_ABI_SYMBOLS,
              host.DIFF_RGL_ABI_SYMBOLS, host.DIFF_RGL_SPECTRAL_ABI_SYMBOLS, host.FIT_TABLE_ABI_SYMBOLS, host.FIT_NCH_ABI_SYMBOLS,
              host.FIT_GGX_ABI_SYMBOLS, host.UPDATE_ABI_SYMBOLS, host.FIT_RGL_ABI_SYMBOLS)
    assert not set(host.FIT_RGL_SPECTRAL_ABI_SYMBOLS) & set().union(*map(set, others))
    for word in ("NOT touched", "Out of scope", "luminance distribution is NOT rebuilt", "caller's responsibility", "POINTERS", "keeps its bits",
                 "Value clamp", "Clamped wavelength", "NaN wavelength", "Dead units", "records x n_wl x S x 32 B"):
        assert word in text, word
    build.build_lib()
    lib = host.load_library()

    def c_class(decl):
        if "*" in decl or "[" in decl:
            return "pointer"
        return {"int": "i32", "int32_t": "i32", "size_t": "u64"}[[w for w in re.findall(r"\w+", decl) if w != "const"][0]]

    def ctypes_class(t):
        if t in (C.c_int, C.c_int32):
            return "i32"
        if t is C.c_size_t:
            return "u64"
        return "pointer"
    for name in host.FIT_RGL_SPECTRAL_ABI_SYMBOLS:
        assert hasattr(lib, name), name
        assert [ctypes_class(t) for t in getattr(lib, name).argtypes] == [c_class(p) for p in protos[name].split(",")], name
    t = (C.c_int32 * 1)(0)
    assert lib.mrl_rgl_spectral_values_grad_batch(None, None, None, None, 4, None, None, 0, 4, t, 1, None) == -1     # no context: MRL_ERR_INVALID
    assert lib.mrl_rgl_spectral_values_grad_queue(None, None, None, None, 4, None, None, 0, None, None, 4, t, 1, None) == -1
    assert lib.mrl_rgl_spectral_values_shape(None, 0, (C.c_int * 5)()) == -1
    assert lib.mrl_material_update_rgl_spectral_values(None, 0, None, 0) == -1
    assert lib.mrl_rgl_spectral_values_grad_layout(None, 1, None) == -1


def test_layout_function_on_hand_computed_shapes_and_its_refusals():
    from mitsuba_customization_amd import host
    L = host.rgl_spectral_values_grad_layout
    # doubles of [n_phi][n_theta][n_wl][ny][nx], end to end
    assert L([(1, 6, 5, 12, 12)]) == [0, 4320]
    assert L([(1, 6, 5, 12, 12), (8, 4, 4, 10, 12), (1, 1, 1, 2, 2)]) == [0, 4320, 4320 + 15360, 4320 + 15360 + 4]
    assert L([(2, 3, 7, 5, 4)] * 16)[-1] == 16 * 840
    assert L([(1, 1, 4096, 2, 2)]) == [0, 4 * 4096]
    for bad in ([], [(1, 6, 5, 12, 12)] * 17, [(0, 6, 5, 12, 12)], [(1, 0, 5, 12, 12)], [(1, 6, 0, 12, 12)], [(1, 6, 4097, 12, 12)], [(1, 6, 5, 1, 12)],
                [(1, 6, 5, 12, 1)], [(1, 6, 5, 12)], [(1, 6, 5, 12, 2 ** 31)]):
        with pytest.raises(ValueError):
            L(bad)
    # (record, node) pairs: (n_phi - 1 or 1) (n_theta - 1 or 1) (ny - 1) (nx - 1) n_wl per target, at most 2^31 - 1 = 2,147,483,647 in all
    assert L([(1, 2, 1, 46341, 46341)])[-1] == 2 * 46341 * 46341                      # 46340^2 = 2,147,395,600 pairs: fits
    with pytest.raises(ValueError):
        L([(1, 2, 2, 46341, 46341)])                                                   # two nodes: twice that
    assert L([(1, 1, 4096, 725, 725)])[-1] == 4096 * 725 * 725                        # 724^2 x 4096 = 2,147,024,896: fits
    with pytest.raises(ValueError):
        L([(1, 1, 4096, 726, 725)])                                                    # 725 x 724 x 4096 = 2,149,990,400
    assert len(L([(1, 2, 1, 46341, 46341), (1, 1, 4, 149, 149)])) == 3                 # + 148^2 x 4 = 87,616: 2,147,483,216
    with pytest.raises(ValueError):
        L([(1, 2, 1, 46341, 46341), (1, 1, 4, 150, 149)])                              # + 149 x 148 x 4 = 88,208: 2,147,483,808


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return vref.build_harness(tmp_path_factory)


@pytest.mark.parametrize("name,W", vref.CASES)
def test_per_lane_functions_and_fold_against_the_reference(harness, tmp_path_factory, name, W):
    """MASK 0 (the id and plain kernels' form) and the file's own MASK (the single-material brick kernels'): both meet the bar, in the
    gradient bricks after the fold and in the plain form, and have the same bits."""
    c = vref.case(name, W)
    start = -0.0                                                   # x + 0 would turn it into +0: an unreached texel keeps its bits
    args = (c["fields"], c["wi"], c["wo"], c["g"], c["wl"], start)
    B0, P0, F0 = vref.run_harness(harness, tmp_path_factory.mktemp("sv_m0"), *args)
    vref.check(B0, c, start, f"{c['name']} host bricks + fold")
    vref.check(P0, c, start, f"{c['name']} host plain")
    B, P, F = vref.run_harness(harness, tmp_path_factory.mktemp("sv_m"), *args, own_mask=True)
    mask = sref.file_mask(c["fields"])
    vref.check(B, c, start, f"{c['name']} host bricks + fold, MASK {mask}")
    vref.check(P, c, start, f"{c['name']} host plain, MASK {mask}")
    assert np.array_equal(B.view(np.uint64), B0.view(np.uint64)) and np.array_equal(P.view(np.uint64), P0.view(np.uint64))
    assert np.array_equal(F.view(np.uint64), F0.view(np.uint64))
    assert np.abs(B).max() > 0
    if name == "iso_negative":                                     # the clamp is at work: some wavelength of some unit contributes nothing
        al = c["alive"]
        d = vref.values_grad(c["arrays"], c["wi"][al], c["wo"][al], c["wl"][al], c["g"][al], spectra=np.abs(np.asarray(c["fields"]["spectra"])))
        assert np.abs(d[1] - c["S"]).max() > 0.0


@pytest.mark.parametrize("name,W", [("iso", 4), ("aniso", 4), ("phi_only", 4), ("iso", None)])
def test_per_lane_functions_and_fold_under_the_host_sanitizers(tmp_path_factory, tmp_path, name, W):
    san = vref.build_harness(tmp_path_factory, sanitize=True)
    c = vref.case(name, W)
    for own in (False, True):
        B, P, _ = vref.run_harness(san, tmp_path, c["fields"], c["wi"], c["wo"], c["g"], c["wl"], 0.0, own_mask=own)
        vref.check(B, c, 0.0, f"{c['name']} host bricks + fold, own MASK {own}, ASan + UBSan")
        vref.check(P, c, 0.0, f"{c['name']} host plain, own MASK {own}, ASan + UBSan")


@pytest.mark.parametrize("n_wl", [1, 3])
@pytest.mark.parametrize("n_phi,n_theta", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_fold_maps_every_slot_to_the_texel_the_copy_rule_implies(harness, tmp_path, n_phi, n_theta, n_wl):
    nx, ny = 3, 4
    S = (2 if n_phi > 1 else 1) * (2 if n_theta > 1 else 1)
    records = max(n_phi - 1, 1) * max(n_theta - 1, 1) * (nx - 1) * (ny - 1)
    doubles = records * n_wl * 4 * S
    passes = (doubles + 49) // 50
    out = tmp_path / "fold.bin"
    r = subprocess.run([str(harness), "fold", str(n_phi), str(n_theta), str(n_wl), str(nx), str(ny), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, np.float64).reshape(passes, n_phi, n_theta, n_wl, ny, nx)
    seen = 0
    for p in range(passes):
        # every slot a distinct power of two within its pass (sums of at most 16 of 50 distinct powers are exact)
        want = vref.fold_expected(n_phi, n_theta, n_wl, nx, ny, lambda at: 2.0 ** (at - 50 * p) if 50 * p <= at < 50 * p + 50 else 0.0)
        assert np.array_equal(got[p], want), (n_phi, n_theta, n_wl, p)
        seen += sum(bin(int(v)).count("1") for v in want.reshape(-1))
    assert seen == doubles                                         # no padding: every slot reaches exactly one texel


@pytest.mark.parametrize("name", ["iso", "aniso", "phi_only"])
def test_three_node_file_with_an_rgb_file_s_arrays_has_the_rgb_unit_s_factors(harness, tmp_path, name):
    """wavelengths == NULL on sref.rgb_as_spectral(f): ws, wc and the three a0 are the bits of rgl::values_grad_unit on f"""
    from tests import rgl_values_grad_reference as rgbref
    c = rgbref.case(name)
    n = len(c["wi"])
    rgbref.rref.write_fields(tmp_path / "rgb.bin", c["fields"])
    with open(tmp_path / "ru.bin", "wb") as o:
        np.array([n], np.uint64).tofile(o)
        for x in (c["wi"], c["wo"], c["g"]):
            np.ascontiguousarray(x, np.float32).tofile(o)
    r = subprocess.run([str(harness), "rgb", str(tmp_path / "rgb.bin"), str(tmp_path / "ru.bin"), str(tmp_path / "ro.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = np.fromfile(tmp_path / "ro.bin", np.float64).reshape(n, 11)
    _, _, F = vref.run_harness(harness, tmp_path, sref.rgb_as_spectral(c["fields"]), c["wi"], c["wo"], c["g"], None)
    assert np.abs(want[:, 8:]).max() > 0 and np.isfinite(want[c["alive"]]).all()
    live = c["alive"]
    assert np.array_equal(F[live, :8].view(np.uint64), want[live, :8].view(np.uint64))
    assert np.array_equal(F[live, 8::3], np.broadcast_to(np.arange(3.0), (int(live.sum()), 3)))          # c0 = k
    assert np.array_equal(F[live, 9::3].view(np.uint64), want[live, 8:].view(np.uint64))                  # a0 = values_grad_unit's a
    assert not F[live, 10::3].any() and not F[~live].any()


def test_wavelengths_on_nodes_and_beyond_both_ends_put_the_whole_weight_on_one_node(harness, tmp_path_factory):
    """lambda exactly on node j, below the first node, above the last, -inf and +inf: only that node's texels change, the others keep
    the bits of the start (-0.0), and what the node receives has the bits of the call on the file's own nodes with g in column j alone"""
    c = vref.case("iso", 4)
    A = c["arrays"]
    al = c["alive"]
    wi, wo = c["wi"][al][:512], c["wo"][al][:512]
    n, n_wl = len(wi), A.n_wl
    g1 = np.random.default_rng(5).standard_normal((n, 1)).astype(np.float32)
    nodes = np.asarray(c["fields"]["wavelengths"], np.float32)

    def run(wl, g):
        B, P, F = vref.run_harness(harness, tmp_path_factory.mktemp("sv_nodes"), c["fields"], wi, wo, g, wl, -0.0)
        return B, P, F
    for lam, j in [(nodes[k], k) for k in range(n_wl)] + [(nodes[0] - 7.0, 0), (nodes[-1] + 7.0, n_wl - 1), (-np.inf, 0), (np.inf, n_wl - 1)]:
        B, P, F = run(np.full((n, 1), lam, np.float32), g1)
        own = np.zeros((n, n_wl), np.float32)
        own[:, j] = g1[:, 0]
        B_own, P_own, _ = run(None, own)
        assert ((F[:, 9] != 0) ^ (F[:, 10] != 0)).all(), lam      # one factor, never both (g != 0, J > 0, nothing clamped on this file)
        for got, want in ((B, B_own), (P, P_own)):
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (lam, j)
            rest = np.delete(got, j, axis=2)
            assert np.array_equal(rest.view(np.uint64), np.full(rest.shape, -0.0).view(np.uint64)), (lam, j)
            assert np.abs(got[:, :, j]).max() > 0
    # a NaN wavelength in one column of live units: that column adds nothing, the rest are the bits of the call without it
    wl = np.random.default_rng(6).uniform(nodes[0], nodes[-1], (n, 3)).astype(np.float32)
    g3 = np.random.default_rng(7).standard_normal((n, 3)).astype(np.float32)
    wl_nan = wl.copy(); wl_nan[:, 1] = np.nan
    g_cut = g3.copy(); g_cut[:, 1] = 0.0
    Bn, Pn, Fn = run(wl_nan, g3)
    Bc, Pc, _ = run(wl, g_cut)
    assert np.array_equal(Bn.view(np.uint64), Bc.view(np.uint64)) and np.array_equal(Pn.view(np.uint64), Pc.view(np.uint64))
    assert not Fn[:, 8 + 3 + 1:8 + 3 + 3].any() and np.isfinite(Bn).all()


def _kernels(asm):
    """{demangled kernel name: (scratch bytes per lane, VGPRs)} from the compiler's per-kernel metadata"""
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    names = subprocess.run(["c++filt"] + [b[0] for b in blocks], capture_output=True, text=True).stdout.splitlines()
    out = {}
    for (mangled, body), d in zip(blocks, names):
        short = re.sub(r"^(void )?mrl::\(anonymous namespace\)::", "", d).split("(")[0]
        out[short] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                      int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)))
    return out


def test_compiled_kernels_use_no_scratch_and_keep_their_registers(tmp_path):
    asm_path = tmp_path / "sv.s"
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", str(asm_path), vref.KERNEL_SOURCE],
                          timeout=900)
    kernels = _kernels(open(asm_path).read())
    accumulate = [k for k in kernels if k.startswith(("k_rgl_spectral_values_bricks<", "k_rgl_spectral_values_plain<"))]
    # 2 (ids / one material's four shapes) x 2 (whole arrays / queue): 10 brick kernels, 4 plain ones
    assert len(accumulate) == 14 and {"k_rgl_spectral_values_fold", "k_rgl_spectral_values_write"} <= set(kernels)
    for name, (scratch, vgprs) in kernels.items():
        print(f"{name}: {vgprs} VGPRs, {scratch} B scratch")
        assert scratch == 0, (name, scratch)
        # __launch_bounds__(256, 2): two waves per SIMD, 256 registers each
        assert vgprs <= 256, (name, vgprs)
