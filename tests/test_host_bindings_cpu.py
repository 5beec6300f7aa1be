"""The Python host against include/merl_hip.h, without a GPU: every symbol's ctypes signature agrees with its prototype, and
every batch / queue wrapper hands each array and scalar to the parameter the header names.  The header is the reference."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from mitsuba_customization_amd import build, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the header: {name: (return class, [(parameter name, class)])} ----
_CLASS_OF_C = {"int": "i32", "int32_t": "i32", "size_t": "u64", "uint64_t": "u64", "float": "float", "double": "double", "void": "void"}


def _c_class(decl: str) -> str:
    if "*" in decl or "[" in decl:                      # an array parameter is a pointer
        return "pointer"
    words = [w for w in re.findall(r"\w+", decl) if w != "const"]
    return _CLASS_OF_C[words[0]]                        # KeyError: a type this test does not know yet


def _prototypes():
    text = open(os.path.join(ROOT, "include", "merl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for ret, name, params in re.findall(r"^[ \t]*((?:const[ \t]+)?\w+[ \t]*\*?)[ \t]*(mrl_\w+)[ \t]*\(([^()]*)\)[ \t]*;", text, flags=re.M):
        assert name not in out, name
        plist = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        out[name] = (_c_class(ret), [(re.findall(r"\w+", re.sub(r"\[.*", "", p))[-1], _c_class(p)) for p in plist])
    return out


PROTOTYPES = _prototypes()


def _ctypes_class(t) -> str:
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    return {C.c_int32: "i32", C.c_uint64: "u64", C.c_float: "float", C.c_double: "double"}[t]      # c_int is c_int32, c_size_t is c_uint64 here


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return host.load_library()


def test_header_parses_to_the_binding_list():
    assert len(PROTOTYPES) == 127
    assert len(set(host.ABI_SYMBOLS)) == len(host.ABI_SYMBOLS)
    assert set(host.ABI_SYMBOLS) == set(PROTOTYPES)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_signature_matches_the_header(lib, name):
    ret, params = PROTOTYPES[name]
    fn = getattr(lib, name)
    assert fn.argtypes is not None, f"{name}: argtypes never set"
    assert [_ctypes_class(t) for t in fn.argtypes] == [c for _, c in params], name
    assert _ctypes_class(fn.restype) == ret, name


# ---- the wrappers under a recording library ----
N, MATERIAL, QUEUE_LEN, CAPACITY = 5, 2, 4, 3
CTX, GROUP = 0xC0DE, 0x6E0
WIDTH_RGB, WIDTH_NCH, WIDTH_SPECTRAL = 3, 4, 7


class RecordingLib:
    """Every mrl_* attribute is a callable that stores (name, args) and returns `status` once (then 0 again)."""

    def __init__(self):
        self.calls, self.status = [], 0

    def __getattr__(self, name):
        if name.endswith("last_error") or name == "mrl_strerror":
            return lambda *a: b""
        if not name.startswith("mrl_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            rc, self.status = self.status, 0
            return rc
        return call


def _owners(monkeypatch):
    lib = RecordingLib()
    gpu = object.__new__(host.MerlHip)
    gpu._lib, gpu._ctx, gpu.device = lib, CTX, 0
    group = object.__new__(host.MerlGroup)
    group._lib, group._g, group.device, group.size = lib, GROUP, 0, 1
    monkeypatch.setattr(host.MerlHip, "_prep", lambda self, first: None)     # the real one rightly refuses CPU tensors
    return lib, gpu, group


# (owner, wrapper, symbol, width, extra keyword arguments); the arrays follow from the wrapper's own parameter names
_RGB = [("eval", "eval"), ("pdf", "pdf"), ("eval_pdf", "eval_pdf"), ("sample", "sample"), ("eval_sample", "eval_sample")]
_NO_PDF = [m for m in _RGB if m[0] != "pdf"]
CASES = (
    [("gpu", m, f"mrl_{m}_batch", WIDTH_RGB, {}) for m, _ in _RGB]
    + [("gpu", f"{m}_queue", f"mrl_{m}_queue", WIDTH_RGB, {}) for m, _ in _RGB]
    + [("gpu", f"{m}_nch", f"mrl_{m}_batch_nch", WIDTH_NCH, {}) for m, _ in _NO_PDF]
    + [("gpu", f"{m}_queue_nch", f"mrl_{m}_queue_nch", WIDTH_NCH, {}) for m, _ in _NO_PDF]
    + [("gpu", "eval_spectral", "mrl_eval_spectral_batch", WIDTH_SPECTRAL, {}),
       ("gpu", "eval_spectral", "mrl_eval_pdf_spectral_batch", WIDTH_SPECTRAL, {"with_pdf": True}),
       ("gpu", "sample_spectral", "mrl_sample_spectral_batch", WIDTH_SPECTRAL, {}),
       ("gpu", "eval_sample_spectral", "mrl_eval_sample_spectral_batch", WIDTH_SPECTRAL, {})]
    + [("gpu", f"{m}_spectral_queue", f"mrl_{m}_spectral_queue", WIDTH_SPECTRAL, {}) for m, _ in _NO_PDF]
    + [("gpu", f"{m}_spectral_mat", f"mrl_{m}_spectral_batch_mat", WIDTH_SPECTRAL, {}) for m, _ in _NO_PDF]
    + [("group", f"{m}_host", f"mrl_group_{m}_batch", WIDTH_RGB, {}) for m, _ in _RGB]
)
CASE_IDS = [f"{c[1]}{'-with_pdf' if c[4] else ''}" for c in CASES]
assert len(CASES) == 35 and len({c[2] for c in CASES}) == 35


def _address(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def _arrays(symbol, width):
    """Distinct input arrays for the call, as torch CPU tensors for a queue call and numpy otherwise."""
    rng = np.random.default_rng(7)
    a = {"wi": rng.random((N, 3), np.float32), "wo": rng.random((N, 3), np.float32), "u": rng.random((N, 2), np.float32),
         "wavelengths": rng.random((N, width), np.float32), "mat": np.full(N, MATERIAL, np.int32),
         "queue": np.arange(QUEUE_LEN, dtype=np.int32), "count": np.array([CAPACITY], np.int32)}
    if "_queue" in symbol:
        import torch
        a = {k: torch.from_numpy(v) for k, v in a.items()}
    return a


def _shape_of(out_name, width):
    return {"out_rgb": (N, width), "out_values": (N, width), "out_weight": (N, width), "out_wo": (N, 3), "out_pdf": (N,), "out_pdf2": (N,)}[out_name]


def _fresh_outputs(symbol, width):
    names = [p for p, _ in PROTOTYPES[symbol][1] if p.startswith("out_")]
    if "_queue" in symbol:
        import torch
        outs = tuple(torch.full(_shape_of(p, width), 9.0, dtype=torch.float32) for p in names)
    else:
        outs = tuple(np.full(_shape_of(p, width), 9.0, np.float32) for p in names)
    return outs[0] if len(outs) == 1 else outs


def _call(owner, wrapper, symbol, width, extra, with_mat, out=None, **override):
    """Calls the wrapper with one value per parameter of its own signature; returns (result, the arrays passed by name)."""
    arrays = _arrays(symbol, width)
    arrays.update(override)
    kwargs = dict(extra)
    for p in inspect.signature(getattr(owner, wrapper)).parameters:
        if p in ("wi", "wo", "u", "wavelengths", "queue", "count"):
            kwargs[p] = arrays[p]
        elif p == "mat" and (with_mat or symbol.endswith("_mat")):
            kwargs[p] = arrays[p]
        elif p == "material":
            kwargs[p] = MATERIAL
        elif p == "n_channels":
            kwargs[p] = width
        elif p == "capacity":
            kwargs[p] = CAPACITY
    if out is not None:
        kwargs["out"] = out
    given = {k: kwargs.get(k) for k in ("wi", "wo", "u", "wavelengths", "mat", "queue")}
    given["queue_count"] = kwargs.get("count")
    return getattr(owner, wrapper)(**kwargs), given


def _check_recorded(lib, owner_name, symbol, width, given, result, out=None):
    assert len(lib.calls) == 1
    name, args = lib.calls[0]
    assert name == symbol
    params = [p for p, _ in PROTOTYPES[symbol][1]]
    assert len(args) == len(params)
    out_names = [p for p in params if p.startswith("out_")]
    results = (result,) if len(out_names) == 1 else result
    assert isinstance(results, tuple) and len(results) == len(out_names)
    if out is not None:
        for r, o in zip(results, (out,) if len(out_names) == 1 else out):
            assert r is o
    for p, a in zip(params, args):
        if p in ("ctx", "g"):
            assert a == (GROUP if owner_name == "group" else CTX) and (p == "g") == (owner_name == "group")
        elif p in given:
            assert a == (None if given[p] is None else _address(given[p])), p
        elif p in ("n", "capacity"):
            assert a == (N if p == "n" else CAPACITY), p
        elif p in ("single_id", "id"):
            assert a == MATERIAL, p
        elif p in ("n_channels", "n_wavelengths"):
            assert a == width, p
        else:
            r = results[out_names.index(p)]                # ValueError: a parameter this test does not know
            assert a == _address(r), p
            assert tuple(r.shape) == _shape_of(p, width), p
            assert str(r.dtype).endswith("float32"), p
            if "_queue" in symbol:
                assert hasattr(r, "data_ptr") and (out is not None or bool((r == 0).all())), p      # fresh queue outputs: torch zeros
            else:
                assert isinstance(r, np.ndarray), p


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_wrapper_allocates_and_passes_arguments_in_abi_order(monkeypatch, case):
    owner_name, wrapper, symbol, width, extra = case
    lib, gpu, group = _owners(monkeypatch)
    owner = group if owner_name == "group" else gpu
    result, given = _call(owner, wrapper, symbol, width, extra, with_mat=False)
    assert given["mat"] is None or symbol.endswith("_mat")
    _check_recorded(lib, owner_name, symbol, width, given, result)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_wrapper_writes_into_the_callers_out(monkeypatch, case):
    owner_name, wrapper, symbol, width, extra = case
    lib, gpu, group = _owners(monkeypatch)
    owner = group if owner_name == "group" else gpu
    out = _fresh_outputs(symbol, width)
    result, given = _call(owner, wrapper, symbol, width, extra, with_mat=True, out=out)
    assert given["mat"] is not None or "mat" not in [p for p, _ in PROTOTYPES[symbol][1]]
    _check_recorded(lib, owner_name, symbol, width, given, result, out=out)
    for o in (out if isinstance(out, tuple) else (out,)):
        assert bool((o == 9.0).all())                      # the wrapper itself writes nothing


@pytest.mark.parametrize("wrapper, symbol", [("eval_spectral", "mrl_eval_spectral_batch"), ("sample_spectral", "mrl_sample_spectral_batch"),
                                             ("eval_sample_spectral", "mrl_eval_sample_spectral_batch"),
                                             ("eval_sample_spectral_queue", "mrl_eval_sample_spectral_queue")])
def test_a_materials_own_nodes_need_no_wavelengths(monkeypatch, wrapper, symbol):
    lib, gpu, _ = _owners(monkeypatch)
    result, given = _call(gpu, wrapper, symbol, WIDTH_SPECTRAL, {"n_wavelengths": WIDTH_SPECTRAL}, with_mat=False, wavelengths=None)
    assert given["wavelengths"] is None
    _check_recorded(lib, "gpu", symbol, WIDTH_SPECTRAL, given, result)


def test_id_batches_of_spectral_materials_require_wavelengths(monkeypatch):
    lib, gpu, _ = _owners(monkeypatch)
    with pytest.raises((ValueError, TypeError, AttributeError)):
        _call(gpu, "eval_spectral_mat", "mrl_eval_spectral_batch_mat", WIDTH_SPECTRAL, {}, with_mat=True, wavelengths=None)
    assert lib.calls == []


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_failing_call_raises_with_the_symbols_name(monkeypatch, case):
    owner_name, wrapper, symbol, width, extra = case
    lib, gpu, group = _owners(monkeypatch)
    lib.status = -1
    with pytest.raises(host.MerlHipError) as e:
        _call(group if owner_name == "group" else gpu, wrapper, symbol, width, extra, with_mat=False)
    assert e.value.status == -1 and str(e.value).startswith(symbol + ": ")


@pytest.mark.parametrize("case", [c for c in CASES if "wo" in [p for p, _ in PROTOTYPES[c[2]][1]]],
                         ids=[i for c, i in zip(CASES, CASE_IDS) if "wo" in [p for p, _ in PROTOTYPES[c[2]][1]]])
def test_a_wrong_shape_is_refused_by_name(monkeypatch, case):
    owner_name, wrapper, symbol, width, extra = case
    lib, gpu, group = _owners(monkeypatch)
    bad = _arrays(symbol, width)["wo"][:N - 1]
    with pytest.raises(ValueError, match=r"^wo: shape"):
        _call(group if owner_name == "group" else gpu, wrapper, symbol, width, extra, with_mat=False, wo=bad)
    assert lib.calls == []


def test_queue_calls_refuse_host_arrays_and_long_capacities(monkeypatch):
    lib, gpu, _ = _owners(monkeypatch)
    a = _arrays("mrl_eval_batch", WIDTH_RGB)               # numpy
    with pytest.raises(ValueError, match="queue calls take GPU tensors"):
        gpu.eval_queue(a["wi"], a["wo"], a["queue"], a["count"])
    t = _arrays("mrl_eval_queue", WIDTH_RGB)
    with pytest.raises(ValueError, match="capacity exceeds the queue's length"):
        gpu.eval_queue(t["wi"], t["wo"], t["queue"], t["count"], capacity=QUEUE_LEN + 1)
    assert lib.calls == []
