"""ctypes bindings to the in-tree native libraries.

The HIP library must be loaded *after* ``torch`` so that it binds to the HIP runtime torch has
already mapped (same ``libamdhip64.so.7`` soname): kernels then run on torch's device/streams and
take ``torch.cuda.current_stream().cuda_stream`` as their ``hipStream_t``.

Device kernels fail loudly: if a CUDA tensor reaches an op and ``libtmog_hip.so`` cannot be built
or loaded, :func:`hip` raises instead of silently falling back to a slower path.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

import torch

from . import build

_lock = threading.Lock()
_host = None
_hip = None

P = C.c_void_p
I32 = C.c_int32
I64 = C.c_int64
F32 = C.c_float

# ---- the native ABI, read from the two headers that are its only declaration (csrc/common/tmog_abi.h,
# csrc/hip/tmog_hip_abi.h). The headers keep to a restricted style, so this is a reader, not a C parser.
_SCALARS = {"int": I32, "int32_t": I32, "unsigned": I32, "uint32_t": I32, "int64_t": I64, "uint64_t": I64,
            "size_t": C.c_size_t, "long": C.c_long, "float": F32, "double": C.c_double}


def _ctype(decl: str, named: bool = True):
    """ctypes type of one C declarator: ``const float* y`` / ``int64_t N``, or a bare return type."""
    if "*" in decl or decl.split()[0] == "hipStream_t":
        return P
    words = [w for w in decl.split() if w != "const"]
    base = " ".join(words[:-1] if named else words)
    if base == "void" and not named:
        return None
    if base not in _SCALARS:
        raise ValueError(f"native ABI header: unknown type in {decl.strip()!r}")
    return _SCALARS[base]


def parse_abi(text: str):
    """``(functions, structs, defines)`` of an ABI header: ``{name: (restype, [argtypes])}``,
    ``{struct: [(field, ctype)]}`` and ``{NAME: int}``."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"\(\s*\*\s*(\w+)\s*\)\s*\([^()]*\)", r"* \1", text)     # a function pointer is a pointer
    structs = {}
    for m in re.finditer(r"struct\s+(\w+)\s*\{([^{}]*)\}", text):
        fields = structs[m[1]] = []
        for decl in filter(str.strip, m[2].split(";")):
            names = [n.split()[-1] for n in decl.split(",")]        # `int32_t F, mode, kind`: one type, many names
            if "*" in decl and len(names) > 1:
                raise ValueError(f"native ABI header: one pointer per declaration, got {decl.strip()!r}")
            fields += [(n, _ctype(decl.split(",")[0])) for n in names]
    text = re.sub(r"struct\s+\w+\s*\{[^{}]*\}", "", text)
    funcs = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(tmog_\w+)\s*\(([^();]*)\)\s*;", text):
        if m[2] in funcs:
            raise ValueError(f"native ABI header: {m[2]} declared twice")
        funcs[m[2]] = (_ctype(m[1], named=False), [_ctype(a) for a in m[3].split(",") if a.strip() not in ("", "void")])
    return funcs, structs, defines


_HOST_ABI, _STRUCT_FIELDS, ABI_CONSTS = parse_abi((build.CSRC / "common" / "tmog_abi.h").read_text())
_HIP_ABI = parse_abi((build.CSRC / "hip" / "tmog_hip_abi.h").read_text())[0]
_HOST_SIGS = {name: args for name, (_, args) in _HOST_ABI.items()}
_HIP_SIGS = {name: args for name, (_, args) in _HIP_ABI.items()}
_RESTYPES = {name: res for name, (res, _) in {**_HOST_ABI, **_HIP_ABI}.items()}


class _Struct(C.Structure):
    """A mirror of a struct of ``tmog_abi.h``; built by keyword, every field named exactly once."""

    def __init__(self, **kw):
        names = {f for f, _ in self._fields_}
        if names != set(kw):
            raise TypeError(f"{type(self).__name__}: missing {sorted(names - set(kw))}, "
                            f"unknown {sorted(set(kw) - names)}")
        super().__init__(**kw)


STRUCTS = {name: type(name, (_Struct,), {"_fields_": fields}) for name, fields in _STRUCT_FIELDS.items()}
_SIZEOF_ORDER = ("GrowArgs", "ResidentIO", "HistItem", "PartItem", "LeafItem")     # tmog_abi_sizeof(which)


def _declare(lib, sigs):
    for name, args in sigs.items():
        fn = getattr(lib, name, None)
        if fn is None:
            continue
        fn.argtypes = args
        fn.restype = _RESTYPES[name]


def _check_loaded_hash(lib, kind: str) -> None:
    """The mapped library reports the sources it was built from (``build._provenance_source``)."""
    fn = getattr(lib, f"tmog_{kind}_source_hash")
    fn.argtypes = []
    fn.restype = C.c_char_p
    got = fn().decode()
    if got != build.source_hash(kind):
        raise RuntimeError(f"loaded {kind} library reports source hash {got}, the tree has {build.source_hash(kind)}")


def host():
    global _host
    if _host is None:
        with _lock:
            if _host is None:
                path = build.build_host()
                build.verify(path, "host")
                lib = C.CDLL(str(path))
                _declare(lib, _HOST_SIGS)
                _check_loaded_hash(lib, "host")
                for which, name in enumerate(_SIZEOF_ORDER):       # the compiler's layout against the derived mirrors
                    if lib.tmog_abi_sizeof(which) != C.sizeof(STRUCTS[name]):
                        raise RuntimeError(f"{name}: the host library has sizeof {lib.tmog_abi_sizeof(which)}, the "
                                           f"ctypes mirror read from tmog_abi.h {C.sizeof(STRUCTS[name])}")
                _host = lib
    return _host


_pyhost = None


def pyhost():
    """The host library's CPython-API entry points (``csrc/host/utf8_pack.cpp``), through ``ctypes.PyDLL``: the
    GIL stays held during the call."""
    global _pyhost
    if _pyhost is None:
        host()                      # built and loaded first (host() takes _lock itself)
        with _lock:
            if _pyhost is None:
                lib = C.PyDLL(str(build.HOST_SO))
                lib.tmog_utf8_offsets.argtypes = [C.py_object, P]
                lib.tmog_utf8_offsets.restype = C.c_int64
                lib.tmog_utf8_copy.argtypes = [C.py_object, P, P]
                lib.tmog_utf8_copy.restype = C.c_int
                _pyhost = lib
    return _pyhost


def _release_torch_cache():
    """Native out-of-memory handler (called from a grower thread, GIL taken by ctypes)."""
    try:
        torch.cuda.empty_cache()
    except Exception:  # noqa: BLE001 - a handler must not unwind into native code
        pass


_OOM_HANDLER_T = C.CFUNCTYPE(None)
_OOM_HANDLER = _OOM_HANDLER_T(_release_torch_cache)      # module-level: must outlive the library's use of it


def hip():
    global _hip
    if _hip is None:
        with _lock:
            if _hip is None:
                if os.environ.get("TMOG_DISABLE_HIP") == "1":
                    raise RuntimeError("HIP kernels disabled by TMOG_DISABLE_HIP=1 but a device tensor was passed")
                path = build.build_hip()
                build.verify(path, "hip")       # never load a library built from other sources
                torch.cuda.init()
                lib = C.CDLL(str(path), mode=C.RTLD_GLOBAL)
                _declare(lib, _HIP_SIGS)
                _check_loaded_hash(lib, "hip")
                dbg = int(os.environ.get("TMOG_HIST_DEBUG", "0"))
                if dbg:
                    lib.tmog_hip_debug_flags(dbg)
                # one device-memory budget: a native buffer growth that runs out of memory first returns
                # torch's cached-but-unused blocks to the device, then retries (ops/csrc/hip/dev_alloc.hpp)
                lib.tmog_hip_set_oom_handler.argtypes = [_OOM_HANDLER_T]
                lib.tmog_hip_set_oom_handler(_OOM_HANDLER)
                _hip = lib
    return _hip


def hip_loaded() -> bool:
    return _hip is not None


def ptr(t) -> int:
    if t is None:
        return None
    return t.data_ptr()


def stream(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def check(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"native kernel {name} failed with code {rc}")
