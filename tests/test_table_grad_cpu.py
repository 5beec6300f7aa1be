"""The adjoint of eval (mrl_table_grad_batch) without a GPU: the numpy reference of A^T (tests/table_grad_reference.py) is pinned to
the CPU oracle's eval, the header / library export the call, and the compiled kernels keep their values in registers and add with
the atomics DESIGN.md §5g names."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import table_grad_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

DIMS = ((90, 90, 180), (7, 5, 12))


def _table(rng, dims):
    """A random table with negative entries (NEGATIVE_KEEP blends them as stored)."""
    return rng.standard_normal((3,) + tuple(dims)) + 0.25


def _end_cells(S):
    """For each axis end, the azimuth wrap and the theta_h = 0 row: the cell the inputs weigh most (S: [3, n0, n1, n2])."""
    n0, n1, n2 = S.shape[1:]
    total = S.sum(0)
    h, d, p = np.meshgrid(np.arange(n0), np.arange(n1), np.arange(n2), indexing="ij")
    cells = []
    for mask in (h == 0, h == n0 - 1, d == 0, d == n1 - 1, p == 0, p == n2 - 1, (h == 0) & (p == 0), (h == 0) & (p == n2 - 1),
                 (d == 0) & (p == 0), (h > 0) & (h < n0 - 1) & (d > 0) & (p > 0) & (p < n2 - 1)):
        best = np.argmax(np.where(mask, total, -1.0))
        cells.append(np.unravel_index(best, total.shape))
    return cells


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("param", (ref.HALF_DIFF, ref.STANDARD, ref.STANDARD_FULL))
@pytest.mark.parametrize("cosine", (True, False))
@pytest.mark.parametrize("trilinear,center", ((False, False), (True, False), (True, True)))     # a nearest lookup has no node position
def test_reference_is_the_transpose_of_the_oracle(oracle, dims, param, cosine, trilinear, center):
    rng = np.random.default_rng(1000 * param + 10 * dims[0] + 2 * cosine + trilinear)
    n = 20000
    wi, wo, _ = oracle.generate_pairs(0xADD0 + param, 0, n)
    wi = np.array(wi, np.float32); wo = np.array(wo, np.float32)
    wo[::97, 2] *= -1.0                                      # some units below the horizon: masked on both sides
    if not trilinear:
        keep = ~ref.near_cell_boundary(wi, wo, dims, param)
        assert (~keep).sum() <= 16
        wi, wo = wi[keep], wo[keep]
    scale = (0.7, 1.3, 2.1)
    opts = oracle.make_opts(lookup=int(trilinear), node=int(center), cosine=0 if cosine else 1, negative=oracle.NEGATIVE_KEEP)
    kw = dict(param=param, trilinear=trilinear, center=center, cosine=cosine, scale=scale)
    # <eval(T), g> = <T, A^T g> for random T, g; the error scale is the sum of the magnitudes of all terms, <|T|, S>
    for _ in range(3):
        T = _table(rng, dims)
        g = rng.standard_normal((len(wi), 3)).astype(np.float32)
        R, S = ref.adjoint(wi, wo, g, dims, **kw)
        ev = oracle.OracleTable(T, scale, param).eval(wi, wo, opts).astype(np.float64)
        lhs, rhs = float((ev * g.astype(np.float64)).sum()), float((T * R).sum())
        terms = float((np.abs(T) * S).sum())
        assert terms > 0 and abs(lhs - rhs) <= 1e-6 * terms, (lhs, rhs, terms)
    # per cell, on one-hot tables
    g = rng.standard_normal((len(wi), 3)).astype(np.float32)
    R, S = ref.adjoint(wi, wo, g, dims, **kw)
    reached = 0
    for k, (h, d, p) in enumerate(_end_cells(S)):
        c = k % 3
        T = np.zeros((3,) + tuple(dims)); T[c, h, d, p] = 1.0
        ev = oracle.OracleTable(T, scale, param).eval(wi, wo, opts).astype(np.float64)
        lhs = float((ev * g.astype(np.float64)).sum())
        assert abs(lhs - R[c, h, d, p]) <= 1e-6 * S[c, h, d, p], ((h, d, p, c), lhs, R[c, h, d, p], S[c, h, d, p])
        reached += S[c, h, d, p] > 0
    # 20000 random pairs may miss an axis end of the (90, 90, 180) grid (a cell with S == 0 checks nothing); on the small grid every
    # end, the wrap and the theta_h = 0 row are reached, so every fold rule is checked with weight on it
    assert reached >= 6
    if dims == (7, 5, 12):
        assert reached == 10


def test_reference_masks_dead_units_whatever_their_gradient():
    dims = (7, 5, 12)
    wi = np.array([[0.3, 0.1, 0.9], [0.3, 0.1, -0.9], [np.nan, 0.0, 1.0], [0.0, 0.0, 0.0], [0.2, 0.2, 0.9]], np.float32)
    wo = np.array([[0.1, -0.4, 0.8], [0.1, -0.4, 0.8], [0.1, -0.4, 0.8], [0.1, -0.4, 0.8], [np.inf, 0.0, 1.0]], np.float32)
    g = np.array([[1, 2, 3], [np.nan] * 3, [np.inf] * 3, [np.nan] * 3, [np.inf] * 3], np.float32)
    R, S = ref.adjoint(wi, wo, g, dims)
    R1, S1 = ref.adjoint(wi[:1], wo[:1], g[:1], dims)
    assert np.isfinite(R).all() and np.array_equal(R, R1) and np.array_equal(S, S1) and S.sum() > 0


def test_header_declares_and_library_exports_table_grad():
    from mitsuba_customization_amd import build, host
    text = open(os.path.join(ROOT, "include", "merl_hip.h")).read()
    assert re.search(r"\bint\s+mrl_table_grad_batch\s*\(", text)
    assert "mrl_table_grad_batch" in host.ABI_SYMBOLS
    build.build_lib()
    lib = host.load_library()
    assert hasattr(lib, "mrl_table_grad_batch")
    assert lib.mrl_table_grad_batch(None, None, None, None, 0, 4, None) == -1       # no context: MRL_ERR_INVALID


def _kernels(asm):
    """{demangled kernel name: (scratch bytes per lane, kernel text)}"""
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    names = subprocess.run(["c++filt"] + [b[0] for b in blocks], capture_output=True, text=True).stdout.splitlines()
    out = {}
    for (mangled, body), d in zip(blocks, names):
        d = d.replace("mrl::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        text = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(mangled), asm, re.S | re.M).group(1)
        out[d] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)), text)
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_table_grad_kernels_keep_registers_and_add_with_f64_atomics():
    import isa_round_trips as irt
    src = os.path.join(ROOT, "mitsuba_customization_amd", "csrc", "merl_table_grad.hip")
    assert os.path.exists(src)
    asm = irt.compile_to_asm(src)
    kernels = _kernels(asm)
    want = {"k_grad_bricks<0>", "k_grad_bricks<1>", "k_grad_naive<0>", "k_grad_naive<1>", "k_grad_fold"}
    assert want <= set(kernels), sorted(kernels)
    assert "cmpswap" not in asm
    for name, (scratch, text) in kernels.items():
        assert scratch == 0, (name, scratch)
    # the accumulate kernels add with global_atomic_add_f64 and nothing narrower; the fold kernel has no atomics
    for name in ("k_grad_bricks<0>", "k_grad_bricks<1>", "k_grad_naive<0>", "k_grad_naive<1>"):
        atomics = set(re.findall(r"\b((?:global|flat|buffer)_atomic_\w+)", kernels[name][1]))
        assert atomics == {"global_atomic_add_f64"}, (name, atomics)
    assert not re.search(r"_atomic_", kernels["k_grad_fold"][1])


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_the_shared_clear_is_the_one_kernel_of_its_unit_and_stores_plainly():
    """merl_grad_scatter.hip: the host call the adjoints share and the kernel that clears their workspace (a kernel, so that a
    captured call replays; DESIGN.md, "What the adjoints share")."""
    import isa_round_trips as irt
    kernels = _kernels(irt.compile_to_asm(os.path.join(ROOT, "mitsuba_customization_amd", "csrc", "merl_grad_scatter.hip")))
    assert set(kernels) == {"k_grad_clear"}, sorted(kernels)
    scratch, text = kernels["k_grad_clear"]
    assert scratch == 0
    assert not re.search(r"_atomic_", text)
