"""The multi-material table adjoint (include/merl_hip_fit_table.h) without a GPU: the header declares exactly
host.FIT_TABLE_ABI_SYMBOLS and the library exports them, the compiled kernels of merl_table_grad.hip keep their values in
registers and add with f64 atomics, and the inputs of tests/test_gpu_table_grad_mat.py (tests/table_grad_mat_inputs.py) have the
make-up that file relies on — checked on the reference alone."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from tests import table_grad_mat_inputs as inp
from tests import table_grad_reference as ref
from tests.test_table_grad_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_header_declares_and_library_exports_the_calls():
    import ctypes as C
    from mitsuba_customization_amd import build, host
    text = open(os.path.join(ROOT, "include", "merl_hip_fit_table.h")).read()
    assert re.search(r'#include\s+"merl_hip.h"', text)
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = dict(re.findall(r"^[ \t]*int[ \t]+(mrl_\w+)[ \t]*\(([^()]*)\)[ \t]*;", code, flags=re.M))
    assert host.FIT_TABLE_ABI_SYMBOLS == ("mrl_table_grad_batch_mat", "mrl_table_grad_queue", "mrl_table_grad_layout")
    assert set(protos) == set(host.FIT_TABLE_ABI_SYMBOLS)
    others = (host.ABI_SYMBOLS, host.FIT_ABI_SYMBOLS, host.DIFF_ABI_SYMBOLS, host.DIFF_TABLE_ABI_SYMBOLS, host.DIFF_NCH_ABI_SYMBOLS)
    assert not set(host.FIT_TABLE_ABI_SYMBOLS) & set().union(*others)
    for other in ("merl_hip.h", "merl_hip_fit.h", "merl_hip_diff.h", "merl_hip_diff_table.h", "merl_hip_diff_nch.h"):
        plain = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not any(name in plain for name in host.FIT_TABLE_ABI_SYMBOLS), other
    assert int(re.search(r"#define\s+MRL_TABLE_GRAD_MAX_TARGETS\s+(\d+)", code).group(1)) == host.TABLE_GRAD_MAX_TARGETS
    for word in ("Not offered", "n-channel", "device groups", "RGL", "one-unit", "ACCUMULATED", "MRL_ERR_POINTER_MIX", "HIP graph"):
        assert word in text, word
    build.build_lib()
    lib = host.load_library()

    def c_class(decl):
        if "*" in decl or "[" in decl:
            return "pointer"
        return {"int": "i32", "int32_t": "i32", "size_t": "u64"}[[w for w in re.findall(r"\w+", decl) if w != "const"][0]]

    def ctypes_class(t):
        return {C.c_int32: "i32", C.c_int: "i32", C.c_uint64: "u64", C.c_size_t: "u64"}.get(t, "pointer")
    want = {"mrl_table_grad_batch_mat": ["pointer"] * 5 + ["i32", "u64", "pointer", "i32", "pointer"],
            "mrl_table_grad_queue": ["pointer"] * 5 + ["i32", "pointer", "pointer", "u64", "pointer", "i32", "pointer"],
            "mrl_table_grad_layout": ["pointer", "i32", "pointer"]}
    for name in host.FIT_TABLE_ABI_SYMBOLS:
        assert hasattr(lib, name)
        assert [c_class(p) for p in protos[name].split(",")] == want[name]
        assert [ctypes_class(t) for t in getattr(lib, name).argtypes] == want[name]
    # no context: MRL_ERR_INVALID
    assert lib.mrl_table_grad_batch_mat(None, None, None, None, None, 0, 4, None, 1, None) == -1
    assert lib.mrl_table_grad_queue(None, None, None, None, None, 0, None, None, 4, None, 1, None) == -1
    # both are rows of the host's call table
    assert {host._CALLS["batch", "table_grad_mat"][0], host._CALLS["queue", "table_grad_mat"][0]} == set(host.FIT_TABLE_ABI_SYMBOLS[:2])


def test_layout_refuses_what_the_int_cell_index_cannot_hold():
    """mrl_table_grad_layout is the arithmetic mrl_table_grad_batch_mat / mrl_table_grad_queue run on their targets' dims: the
    contract's row 'a cell total above 2^31 - 1: MRL_ERR_INVALID' is driven here, where it needs neither 16 tables of 17 GB each
    nor a GPU."""
    import ctypes as C
    from mitsuba_customization_amd import build, host
    build.build_lib()
    lib = host.load_library()
    big = (512, 512, 513)                                          # 134,479,872 cells: 15 of them fit, 16 do not
    assert 15 * np.prod(big, dtype=np.int64) + 90 * 90 * 180 < 2 ** 31 - 1 < 16 * np.prod(big, dtype=np.int64)

    def layout(dims_list, n=None, want_offsets=True):
        flat = (C.c_int * max(3 * len(dims_list), 1))(*[int(v) for d in dims_list for v in d])
        out = (C.c_size_t * (host.TABLE_GRAD_MAX_TARGETS + 1))(*([12345] * (host.TABLE_GRAD_MAX_TARGETS + 1)))
        rc = lib.mrl_table_grad_layout(flat, len(dims_list) if n is None else n, out if want_offsets else None)
        return rc, list(out[:len(dims_list) + 1])
    rc, offsets = layout([big] * 15 + [(90, 90, 180)])
    cells = [int(np.prod(big))] * 15 + [90 * 90 * 180]
    assert rc == 0 and offsets == [3 * sum(cells[:k]) for k in range(17)]
    assert layout([big] * 16)[0] == -1 and layout([big] * 16, want_offsets=False)[0] == -1
    # exactly 2^31 - 1 cells is the last total that fits; one more cell, in the last table or in another one, does not
    assert layout([(2 ** 31 - 1, 1, 1)]) == (0, [0, 3 * (2 ** 31 - 1)])
    assert layout([(2 ** 30, 2, 1)])[0] == -1 and layout([(2 ** 31 - 1, 1, 1), (1, 1, 1)])[0] == -1
    assert layout([(1, 1, 1), (2 ** 31 - 1, 1, 1)])[0] == -1
    # products that would wrap a 64-bit sum if they were formed carelessly
    assert layout([(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)])[0] == -1 and layout([(2 ** 16, 2 ** 16, 2 ** 16)] * 16)[0] == -1
    # the other rows: NULL dims, n_targets out of range, a dim below 1
    assert lib.mrl_table_grad_layout(None, 1, None) == -1
    assert layout([(7, 5, 12)], n=0)[0] == -1 and layout([(7, 5, 12)], n=-1)[0] == -1
    assert layout([(7, 5, 12)] * 17)[0] == -1
    assert layout([(7, 0, 12)])[0] == -1 and layout([(7, 5, 12), (-3, 5, 12)])[0] == -1
    assert layout([(7, 5, 12), (1, 1, 1), (5, 1, 2)]) == (0, [0, 1260, 1263, 1293])
    # the Python face of it
    assert host.table_grad_layout([(7, 5, 12), (1, 1, 1), (5, 1, 2)]) == [0, 1260, 1263, 1293]
    for bad in ([big] * 16, [], [(7, 5, 12)] * 17, [(7, 0, 12)]):
        with pytest.raises(ValueError):
            host.table_grad_layout(bad)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_kernels_with_targets_keep_registers_and_add_with_f64_atomics():
    import isa_round_trips as irt
    asm = irt.compile_to_asm(os.path.join(ROOT, "mitsuba_customization_amd", "csrc", "merl_table_grad.hip"))
    kernels = _kernels(asm)
    accumulate = {f"k_grad_{form}_mat<{lookup}, {queue}>" for form in ("bricks", "naive") for lookup in (0, 1) for queue in ("false", "true")}
    accumulate |= {"k_grad_bricks<0>", "k_grad_bricks<1>", "k_grad_naive<0>", "k_grad_naive<1>"}
    assert set(kernels) == accumulate | {"k_grad_fold"}, sorted(kernels)
    assert "cmpswap" not in asm
    for name, (scratch, text) in kernels.items():
        assert scratch == 0, (name, scratch)
    for name in accumulate:
        atomics = set(re.findall(r"\b((?:global|flat|buffer)_atomic_\w+)", kernels[name][1]))
        assert atomics == {"global_atomic_add_f64"}, (name, atomics)
    assert not re.search(r"_atomic_", kernels["k_grad_fold"][1])


# ---- the inputs of the GPU tests, on the reference alone ----
# (dims, param): the least number of cells with >= 64 interior units over both node conventions, as measured for this pool
FULL_CELLS = {((7, 5, 12), ref.HALF_DIFF): 160, ((9, 4, 6), ref.STANDARD): 177, ((5, 1, 2), ref.STANDARD): 10,
              ((33, 17, 64), ref.STANDARD_FULL): 0, ((2, 3, 1), ref.HALF_DIFF): 5}


@pytest.mark.parametrize("dims,param", sorted(FULL_CELLS))
@pytest.mark.parametrize("center", (False, True))
def test_pool_has_the_interior_units_the_targets_need(dims, param, center):
    wi, wo = inp.pool()
    inside = ref.interior(wi, wo, dims, param, center)
    cell = ref.cell_index(wi[inside], wo[inside], dims, param, center)
    full = int((np.bincount(cell, minlength=int(np.prod(dims))) >= 64).sum())
    print(f"dims {dims} param {param} center {center}: {int(inside.sum())} interior units, {full} cells with >= 64")
    assert inside.sum() >= 42000
    assert full >= FULL_CELLS[dims, param]


@pytest.mark.parametrize("center", (False, True))
def test_interleaved_units_are_interior_for_their_own_material(center):
    n = inp.BASE
    wi, wo, g, role = inp.interleaved(inp.MIXED, center, n)
    roles = len(inp.MIXED) + len(inp.OTHERS)
    assert np.array_equal(role, np.arange(n) % roles)          # lane by lane: a wave holds every target and every stray id
    live = ref.guard(wi, wo)
    for k, (dims, param) in enumerate(inp.MIXED):
        at = role == k
        assert ref.interior(wi[at], wo[at], dims, param, center)[live[at]].all()
        assert 0 < (~live[at]).sum() < at.sum() // 4           # some dead units in every target
        assert np.isfinite(g[at & live]).all() and not np.isfinite(g[at & ~live]).any()
    assert not np.isfinite(g[role >= len(inp.MIXED)]).any()    # every stray unit is poisoned
    refs = inp.reference(wi, wo, g, role, inp.MIXED, 1, center)
    for (R, S), cells in zip(refs, inp.cells(inp.MIXED)):
        assert np.isfinite(R).all() and (S > 0).sum() > 0 and R.size == 3 * cells
    # the thin set: the quiet target gets no unit, every texel of the others carries weight
    wi, wo, g, role = inp.interleaved(inp.THIN, center, 1536, quiet=(inp.THIN_QUIET,), others=False)
    assert set(role.tolist()) == {0, 2, 3}
    for k, (R, S) in enumerate(inp.reference(wi, wo, g, role, inp.THIN, 1, center)):
        assert (S == 0).all() if k == inp.THIN_QUIET else (S > 0).all()


@pytest.mark.parametrize("center", (False, True))
def test_one_cell_wave_and_its_patterns(center):
    wi, wo = inp.one_cell_wave(center)
    dims, param = inp.SAME
    assert wi.shape == (64, 3) and ref.guard(wi, wo).all() and ref.interior(wi, wo, dims, param, center).all()
    assert len(set(ref.cell_index(wi, wo, dims, param, center).tolist())) == 1
    want = {"alternating": (32, 32, 16), "halves": (32, 32, 32), "four": (4, 60, 4)}          # units of A, of B, of A in the low half
    for name in inp.SAME_PATTERNS:
        role = inp.same_pattern(name)
        assert ((role == 0).sum(), (role == 1).sum(), (role[:32] == 0).sum()) == want[name]


def test_queue_lists_one_slot_twice_and_skips_one():
    q = inp.queue_slots()
    assert len(q) == inp.BASE and q.min() >= 0 and q.max() < inp.BASE
    counts = np.bincount(q, minlength=inp.BASE)
    assert sorted(np.bincount(counts).tolist()) == [1, 1, inp.BASE - 2]      # one slot twice, one never, the rest once
    assert counts[q[3]] == 2 and (np.bincount(q[:600], minlength=inp.BASE) == 2).sum() == 1
    assert not np.array_equal(np.sort(q[:600]), q[:600])
