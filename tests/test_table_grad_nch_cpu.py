"""The n-channel table adjoint (include/merl_hip_fit_nch.h) without a GPU: the numpy reference of A^T
(tests/table_grad_nch_reference.py) is pinned to the CPU oracle's n-channel eval, never to the code under test; the header declares
exactly host.FIT_NCH_ABI_SYMBOLS and the library exports them; mrl_table_grad_layout_nch is driven at its bounds; the compiled kernels
of merl_table_grad_nch.hip keep their values in registers and add with f64 atomics; and the inputs of
tests/test_gpu_table_grad_nch.py have the make-up that file relies on — checked on the reference alone."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from tests import table_grad_mat_inputs as inp
from tests import table_grad_nch_reference as nref
from tests import table_grad_reference as ref
from tests.test_table_grad_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SPECS = (((7, 5, 12), ref.HALF_DIFF), ((9, 4, 6), ref.STANDARD), ((33, 17, 64), ref.STANDARD_FULL))
WIDTHS = (1, 2, 4, 5, 8, 31, 32)                                 # of tests/test_gpu_table_grad_nch.py


@pytest.mark.parametrize("n_ch", (1, 5, 16))
@pytest.mark.parametrize("dims,param", SPECS)
def test_reference_is_the_transpose_of_the_oracle(oracle, n_ch, dims, param):
    """<eval_nch(T), g> = <T, A^T g> for a random positive T with non-unit scales; the error scale is the sum of the magnitudes of all
    terms, <|T|, S>.  2e-6: the bar tests/test_table_grad_cpu.py uses for the same identity (it covers the Float rounding of the eval
    outputs)."""
    rng = np.random.default_rng(100 * n_ch + 10 * param + dims[0])
    n = 20000
    wi0, wo0, _ = oracle.generate_pairs(0xADD0 + param, 0, n)
    wi0 = np.array(wi0, np.float32); wo0 = np.array(wo0, np.float32)
    wo0[::97, 2] *= -1.0                                         # some units below the horizon: masked on both sides
    scale = nref.scales(n_ch, 1)
    for trilinear, center in ((True, False), (True, True), (False, False)):
        wi, wo = wi0, wo0
        if not trilinear:
            near = ref.near_cell_boundary(wi, wo, dims, param)
            assert near.sum() <= 16, int(near.sum())            # asserted on the reference alone
            wi, wo = wi[~near], wo[~near]
        u = np.zeros((len(wi), 2), np.float32)
        for cosine in (True, False):
            opts = oracle.make_opts(lookup=int(trilinear), node=int(center), cosine=0 if cosine else 1)
            T = rng.random((n_ch,) + tuple(dims)) + 0.25
            g = rng.standard_normal((len(wi), n_ch)).astype(np.float32)
            R, S = nref.adjoint_nch(wi, wo, g, dims, param, trilinear, center, cosine, scale)
            assert R.shape == S.shape == T.shape
            ev = oracle.eval_sample_nch([oracle.OracleTableNch(T, scale, param)], wi, wo, u, None, opts)[0].astype(np.float64)
            lhs, rhs = float((ev * g.astype(np.float64)).sum()), float((T * R).sum())
            terms = float((np.abs(T) * S).sum())
            print(f"n_ch {n_ch} dims {dims} trilinear {trilinear} center {center} cosine {cosine}: |lhs - rhs| / terms = {abs(lhs - rhs) / terms:.3e}")
            assert terms > 0 and abs(lhs - rhs) <= 2e-6 * terms, (lhs, rhs, terms)


def test_reference_masks_dead_units_whatever_their_gradient():
    dims = (7, 5, 12)
    wi = np.array([[0.3, 0.1, 0.9], [0.3, 0.1, -0.9], [np.nan, 0.0, 1.0], [0.0, 0.0, 0.0], [0.2, 0.2, 0.9]], np.float32)
    wo = np.array([[0.1, -0.4, 0.8], [0.1, -0.4, 0.8], [0.1, -0.4, 0.8], [0.1, -0.4, 0.8], [np.inf, 0.0, 1.0]], np.float32)
    g = np.array([[1, 2, 3, 4, 5], [np.nan] * 5, [np.inf] * 5, [np.nan] * 5, [np.inf] * 5], np.float32)
    R, S = nref.adjoint_nch(wi, wo, g, dims, scale=nref.scales(5))
    R1, S1 = nref.adjoint_nch(wi[:1], wo[:1], g[:1], dims, scale=nref.scales(5))
    assert np.isfinite(R).all() and np.array_equal(R, R1) and np.array_equal(S, S1) and S.sum() > 0
    # three of its channels with the RGB reference's scales: the RGB reference up to its weights' rounding to Float
    R3, S3 = nref.adjoint_nch(wi, wo, g[:, :3], dims, scale=(0.7, 1.3, 2.1))
    Rr, Sr = ref.adjoint(wi, wo, g[:, :3], dims, scale=(0.7, 1.3, 2.1))
    assert (np.abs(R3 - Rr) <= 1e-7 * Sr).all() and ((S3 > 0) == (Sr > 0)).all()


def test_header_declares_and_library_exports_the_calls():
    import ctypes as C
    from mitsuba_customization_amd import build, host
    text = open(os.path.join(ROOT, "include", "merl_hip_fit_nch.h")).read()
    assert re.search(r'#include\s+"merl_hip_fit_table.h"', text)
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = re.findall(r"^[ \t]*int[ \t]+(mrl_\w+)[ \t]*\(([^()]*)\)[ \t]*;", code, flags=re.M)
    assert host.FIT_NCH_ABI_SYMBOLS == ("mrl_table_grad_batch_nch", "mrl_table_grad_queue_nch", "mrl_table_grad_layout_nch")
    assert tuple(name for name, _ in protos) == host.FIT_NCH_ABI_SYMBOLS          # exactly these, in this order
    protos = dict(protos)
    others = (host.ABI_SYMBOLS, host.FIT_ABI_SYMBOLS, host.DIFF_ABI_SYMBOLS, host.DIFF_TABLE_ABI_SYMBOLS, host.DIFF_NCH_ABI_SYMBOLS,
              host.FIT_TABLE_ABI_SYMBOLS, host.FIT_GGX_ABI_SYMBOLS)
    assert not set(host.FIT_NCH_ABI_SYMBOLS) & set().union(*others)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other == "merl_hip_fit_nch.h" or not other.endswith(".h"):
            continue
        plain = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not any(re.search(r"\b%s\b" % name, plain) for name in host.FIT_NCH_ABI_SYMBOLS), other
    for word in ("Not offered", "device groups", "RGL", "one-unit", "autograd", "ACCUMULATED", "MRL_ERR_POINTER_MIX", "HIP graph",
                 "1.49 GB", "2.99 GB", "behaves as 2"):
        assert word in text, word
    # the headers that named the hole now point here
    for other in ("merl_hip.h", "merl_hip_fit_table.h", "merl_hip_diff_nch.h"):
        assert "merl_hip_fit_nch.h" in open(os.path.join(ROOT, "include", other)).read(), other
    build.build_lib()
    lib = host.load_library()

    def c_class(decl):
        if "*" in decl or "[" in decl:
            return "pointer"
        return {"int": "i32", "int32_t": "i32", "size_t": "u64"}[[w for w in re.findall(r"\w+", decl) if w != "const"][0]]

    def ctypes_class(t):
        return {C.c_int32: "i32", C.c_int: "i32", C.c_uint64: "u64", C.c_size_t: "u64"}.get(t, "pointer")
    want = {"mrl_table_grad_batch_nch": ["pointer"] * 5 + ["i32", "u64", "i32", "pointer", "i32", "pointer"],
            "mrl_table_grad_queue_nch": ["pointer"] * 5 + ["i32", "pointer", "pointer", "u64", "i32", "pointer", "i32", "pointer"],
            "mrl_table_grad_layout_nch": ["pointer", "i32", "i32", "pointer"]}
    for name in host.FIT_NCH_ABI_SYMBOLS:
        assert hasattr(lib, name)
        assert [c_class(p) for p in protos[name].split(",")] == want[name]
        assert [ctypes_class(t) for t in getattr(lib, name).argtypes] == want[name]
    # no context: MRL_ERR_INVALID
    assert lib.mrl_table_grad_batch_nch(None, None, None, None, None, 0, 4, 5, None, 1, None) == -1
    assert lib.mrl_table_grad_queue_nch(None, None, None, None, None, 0, None, None, 4, 5, None, 1, None) == -1
    # both are rows of the host's call table
    assert (host._CALLS["batch", "table_grad_nch"][0], host._CALLS["queue", "table_grad_nch"][0]) == host.FIT_NCH_ABI_SYMBOLS[:2]
    assert callable(host.MerlHip.table_grad_nch) and callable(host.MerlHip.table_grad_queue_nch)


def test_layout_offsets_and_the_bound_on_the_brick_index():
    import ctypes as C
    from mitsuba_customization_amd import build, host
    build.build_lib()
    lib = host.load_library()
    slots = host.TABLE_GRAD_MAX_TARGETS + 1

    def layout(dims_list, n_ch, n=None, want_offsets=True):
        flat = (C.c_int * max(3 * len(dims_list), 1))(*[int(v) for d in dims_list for v in d])
        out = (C.c_size_t * slots)(*([12345] * slots))
        rc = lib.mrl_table_grad_layout_nch(flat, len(dims_list) if n is None else n, n_ch, out if want_offsets else None)
        return rc, list(out[:len(dims_list) + 1])

    def rgb(dims_list):
        flat = (C.c_int * (3 * len(dims_list)))(*[int(v) for d in dims_list for v in d])
        out = (C.c_size_t * slots)()
        return lib.mrl_table_grad_layout(flat, len(dims_list), out), list(out[:len(dims_list) + 1])
    three = [(7, 5, 12), (1, 1, 1), (5, 1, 2)]
    assert layout(three, 5) == (0, [0, 2100, 2105, 2155])
    assert layout(three, 3) == rgb(three) == (0, [0, 1260, 1263, 1293])
    assert layout(three, 1) == (0, [0, 420, 421, 431]) and layout(three, 32) == (0, [0, 13440, 13472, 13792])
    # sum cells x ceil(n_ch / 4) may reach 2^31 - 1 and no more
    top = [(2 ** 31 - 1, 1, 1)]
    assert layout(top, 4) == (0, [0, 4 * (2 ** 31 - 1)]) and layout(top, 1)[0] == 0
    assert layout(top, 5)[0] == -1 and layout(top, 5, want_offsets=False)[0] == -1 and layout(top, 32)[0] == -1
    assert layout([(2 ** 29, 1, 1), (2 ** 29 - 1, 1, 1)], 8)[0] == 0 and layout([(2 ** 29, 1, 1)] * 2, 8)[0] == -1      # two groups
    assert layout([(90, 90, 180)] * 16, 32)[0] == 0
    # everything mrl_table_grad_layout refuses
    assert lib.mrl_table_grad_layout_nch(None, 1, 5, None) == -1
    assert layout([(7, 5, 12)], 5, n=0)[0] == -1 and layout([(7, 5, 12)] * 17, 5)[0] == -1 and layout([(7, 5, 12)], 5, n=-1)[0] == -1
    assert layout([(7, 0, 12)], 5)[0] == -1 and layout([(7, 5, 12), (-3, 5, 12)], 5)[0] == -1
    assert layout([(2 ** 31 - 1, 1, 1), (1, 1, 1)], 1)[0] == -1 and layout([(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)], 1)[0] == -1
    # the channel count
    assert layout(three, 0)[0] == -1 and layout(three, 33)[0] == -1 and layout(three, -1)[0] == -1
    # the Python face of it
    assert host.table_grad_layout_nch(three, 5) == [0, 2100, 2105, 2155]
    assert host.table_grad_layout_nch(three, 3) == host.table_grad_layout(three)
    for bad, n_ch in ((top, 5), ([], 5), ([(7, 5, 12)] * 17, 5), ([(7, 0, 12)], 5), (three, 0), (three, 33)):
        with pytest.raises(ValueError):
            host.table_grad_layout_nch(bad, n_ch)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_kernels_keep_registers_and_add_with_f64_atomics():
    import isa_round_trips as irt
    asm = irt.compile_to_asm(os.path.join(ROOT, "mitsuba_customization_amd", "csrc", "merl_table_grad_nch.hip"))
    kernels = _kernels(asm)
    accumulate = {f"k_grad_bricks_nch<{lookup}, {queue}>" for lookup in (0, 1) for queue in ("false", "true")}
    # the clear of the workspace is k_grad_clear of merl_grad_scatter.hip (test_table_grad_cpu.py checks it there)
    assert set(kernels) == accumulate | {"k_grad_fold_nch"}, sorted(kernels)
    assert "cmpswap" not in asm
    for name, (scratch, text) in kernels.items():
        assert scratch == 0, (name, scratch)
    for name in accumulate:
        atomics = set(re.findall(r"\b((?:global|flat|buffer)_atomic_\w+)", kernels[name][1]))
        assert atomics == {"global_atomic_add_f64"}, (name, atomics)
    assert not re.search(r"_atomic_", kernels["k_grad_fold_nch"][1])


# ---- the inputs of the GPU tests, on the reference alone ----
@pytest.mark.parametrize("center", (False, True))
def test_sequences_are_interior_reach_texels_and_hold_some_dead_units(center):
    wi, wo = ref.sequence(*inp.pool(), (7, 5, 12), ref.HALF_DIFF, center, inp.BASE)
    live = ref.guard(wi, wo)
    assert ref.interior(wi, wo, (7, 5, 12), ref.HALF_DIFF, center)[live].all()
    assert 0 < (~live).sum() < len(live) // 4
    for n_ch in WIDTHS:
        g = nref.gradients(wi, wo, n_ch, n_ch)
        assert g.shape == (inp.BASE, n_ch) and np.isfinite(g[live]).all() and not np.isfinite(g[~live]).any()
        for trilinear in (True, False):
            R, S = nref.adjoint_nch(wi, wo, g, (7, 5, 12), trilinear=trilinear, center=center, scale=nref.scales(n_ch))
            assert np.isfinite(R).all() and all((S[c] > 0).sum() > 0 for c in range(n_ch))
    # mixed targets: lane by lane, every unit interior for its own target, every stray unit poisoned
    wi, wo, _, role = inp.interleaved(inp.MIXED, center, inp.BASE)
    g = nref.gradients(wi, wo, 5, 50, stray=role >= len(inp.MIXED))
    live = ref.guard(wi, wo)
    assert not np.isfinite(g[role >= len(inp.MIXED)]).any()
    for k, (dims, param) in enumerate(inp.MIXED):
        at = role == k
        assert ref.interior(wi[at], wo[at], dims, param, center)[live[at]].all()
        assert 0 < (~live[at]).sum() < at.sum() // 4
        assert np.isfinite(g[at & live]).all() and not np.isfinite(g[at & ~live]).any()
    for R, S in nref.reference(wi, wo, g, role, inp.MIXED, 1, center):
        assert np.isfinite(R).all() and all((S[c] > 0).sum() > 0 for c in range(5))
    # the thin set: the quiet target gets no unit, every texel of the others carries weight
    wi, wo, _, role = inp.interleaved(inp.THIN, center, 1536, quiet=(inp.THIN_QUIET,), others=False)
    g = nref.gradients(wi, wo, 5, 51)
    live = ref.guard(wi, wo)
    for k, (dims, param) in enumerate(inp.THIN):
        at = role == k
        if k != inp.THIN_QUIET:
            assert ref.interior(wi[at], wo[at], dims, param, center)[live[at]].all() and 0 < (~live[at]).sum() < at.sum() // 4
    for k, (R, S) in enumerate(nref.reference(wi, wo, g, role, inp.THIN, 1, center)):
        assert (S == 0).all() if k == inp.THIN_QUIET else (S > 0).all()
    # the wave layouts and the one-cell wave
    for name, (a, b) in ref.wave_layouts(*inp.pool(), (7, 5, 12), ref.HALF_DIFF, center).items():
        live = ref.guard(a, b)
        assert ref.interior(a, b, (7, 5, 12), ref.HALF_DIFF, center)[live].all() and (~live).sum() < len(live) // 4, name
        R, S = nref.adjoint_nch(a, b, nref.gradients(a, b, 5, 52), (7, 5, 12), center=center, scale=nref.scales(5))
        assert all((S[c] > 0).sum() > 0 for c in range(5))
    a, b = inp.one_cell_wave(center)
    assert ref.interior(a, b, *inp.SAME, center).all()


def test_host_array_inputs_are_interior():
    wi, wo = inp.pool()
    keep = np.nonzero(ref.interior(wi, wo, (7, 5, 12), ref.HALF_DIFF, False))[0]
    assert len(keep) >= 40009
