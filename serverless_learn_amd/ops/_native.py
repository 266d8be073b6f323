"""ctypes binding of ``libslkernels.so`` (the gfx950 HIP kernels).

Every launcher takes raw device pointers plus the HIP stream and returns 0 on
success (non-zero = hipError_t or an argument error).  Launchers are cheap to
call and are captured into hipGraphs by ``torch.cuda.graph`` because they
launch on the caller's current stream.

The signatures are not written here.  ``csrc/kernels/sl_api.h`` declares every
exported ``sl_*`` function once; the compiler holds each definition to it, and
:func:`parse_api` reads the same text at import to derive ``_SIGS`` (name ->
argtypes) and ``_RESTYPE`` (name -> restype), so every export has its argtypes
and a Python signature cannot drift from the C one.

There is deliberately NO silent fallback: on a machine with a GPU the ops
raise if the extension is missing or fails, so a test can never pass on an
eager PyTorch path while claiming to exercise the HIP kernels.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

import torch

from ..build import API_HEADER, KERNELS_DET_SO, KERNELS_SO

_lock = threading.Lock()
_lib = None
_lib_is_default = True  # False: an A/B build loaded through SL_KERNELS_SO, which may lack newer kernels

# the header's whole type vocabulary (plus: anything with a '*' is a pointer)
_CTYPES = {
    "int": ctypes.c_int, "unsigned": ctypes.c_uint, "long": ctypes.c_long, "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "double": ctypes.c_double,
    "hipStream_t": ctypes.c_void_p,
}
_TYPE_WORDS = {"int", "unsigned", "long", "float", "double", "void", "hipStream_t"}
_DECL = re.compile(r"([\w\s:*]+?)\b(\w+)\s*\(([^()]*)\)")


def _ctype(text: str, decl: str, named: bool):
    """ctypes type of one parameter (``named``: a trailing parameter name is dropped) or return type."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return ctypes.c_void_p
    if named and len(words) > 1 and words[-1] not in _TYPE_WORDS:
        words.pop()
    try:
        return _CTYPES[" ".join(words)]
    except KeyError:
        raise ValueError(f"sl_api.h: type {text.strip()!r} is outside the ABI's vocabulary in: {decl}") from None


def parse_api(text: str) -> dict[str, tuple]:
    """``{name: (restype, argtypes)}`` for every ``RET NAME(PARAMS);`` in the extern "C" block of
    a header's text.  Anything in the block that is not such a declaration raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    block = re.search(r'extern\s+"C"\s*\{(.*)\}', text, re.S)
    if not block:
        raise ValueError('sl_api.h: no extern "C" { ... } block')
    *decls, rest = block.group(1).split(";")
    if rest.strip():
        raise ValueError("sl_api.h: declaration without ';': " + " ".join(rest.split()))
    api = {}
    for decl in decls:
        decl = " ".join(decl.split())
        m = _DECL.fullmatch(decl)
        if not m:
            raise ValueError("sl_api.h: not a 'RET NAME(PARAMS);' declaration: " + decl)
        ret, name, params = m.groups()
        if name in api:
            raise ValueError("sl_api.h: declared twice: " + name)
        restype = None if ret.split() == ["void"] else _ctype(ret, decl, named=False)
        params = [] if params.split() in ([], ["void"]) else params.split(",")
        api[name] = (restype, [_ctype(p, decl, named=True) for p in params])
    return api


with open(API_HEADER) as _f:
    _API = parse_api(_f.read())
_SIGS: dict[str, list] = {name: argtypes for name, (_, argtypes) in _API.items()}
_RESTYPE = {name: restype for name, (restype, _) in _API.items()}


def _bind(lib, name):
    fn = getattr(lib, name)
    fn.argtypes = _SIGS[name]
    fn.restype = _RESTYPE[name]


def available() -> bool:
    return os.path.exists(KERNELS_SO)


def lib():
    """Load (building first if needed) the kernel library."""
    global _lib, _lib_is_default
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            det = os.environ.get("SL_DETERMINISTIC", "0") == "1"  # bit-reproducible kernel build
            path = os.environ.get("SL_KERNELS_SO") or (KERNELS_DET_SO if det else KERNELS_SO)  # override: A/B builds
            if not os.path.exists(path):
                from ..build import build_kernels

                build_kernels(deterministic=det)
            handle = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            _lib_is_default = path in (KERNELS_SO, KERNELS_DET_SO)
            for name in _SIGS:
                if not _lib_is_default and not hasattr(handle, name):
                    continue  # an A/B build of older kernels: only what it exports
                _bind(handle, name)
            _lib = handle
    return _lib


def stream_ptr(stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def ptr(t) -> int | None:
    """Device pointer of a tensor (None passes a NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def call(name: str, *args) -> None:
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc}")


class Launch:
    """A kernel launch with its arguments converted to ctypes ONCE.

    Engines with static buffers (the fused MLP/CNN steps) build these at setup
    and call them every step: the per-launch host cost drops to one ctypes
    call plus the current-stream lookup, which matters for the eager (non
    hipGraph) multi-GPU path where the host must stay ahead of ~30 us steps.

    ``entry`` names another launcher of the same signature that does ``name``'s work from
    differently laid-out inputs (``sl_mlp_rows`` / ``sl_mlp_rows_xt``): ``name`` stays the
    launch's identity in the step, ``entry`` is the symbol called.
    """

    __slots__ = ("name", "entry", "fn", "args")

    def __init__(self, name: str, *args, entry: str | None = None):
        self.name = name
        self.entry = entry or name
        if _SIGS[self.entry] != _SIGS[name]:
            raise ValueError(f"{self.entry} does not have {name}'s signature")
        fn = getattr(lib(), self.entry)
        self.fn = fn
        conv = []
        for a, t in zip(args, _SIGS[name]):
            conv.append(a if a is None else t(a))
        self.args = tuple(conv)

    def __call__(self, stream=None) -> None:
        rc = self.fn(*self.args, ctypes.c_void_p(stream_ptr(stream)))
        if rc != 0:
            raise RuntimeError(f"{self.entry} failed with code {rc}")
