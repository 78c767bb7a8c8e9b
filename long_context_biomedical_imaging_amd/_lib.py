"""ctypes binding of liblci.so (the C-ABI declared in include/lci.h).

There is no fallback: if the library is missing, or a tensor is not on a ROCm device, the op raises.
`import torch` happens first so that liblci's libamdhip64.so.7 dependency binds to the HIP runtime torch
already loaded (one runtime, one set of streams).
"""
from __future__ import annotations

import ctypes
import functools
import os
import re

import torch

from . import build_lib

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "liblci.so")
LIB_PATH = os.environ.get("LCI_LIB_PATH", DEFAULT_LIB)   # override: kernel-variant A/B runs (no staleness check)

# The type map of include/lci.h. An argument with `*` or `[` is a pointer; nothing else is guessed.
_RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}
# dtype codes of the ABI (include/lci.h "Conventions")
DTYPE = {torch.float32: 0, torch.bfloat16: 1}

_lib = None


class LciError(RuntimeError):
    pass


def signatures(text: str) -> dict:
    """name -> (restype, argtypes) of every function a C header text declares (include/lci.h's: `lci_*` functions
    of pointers, int, float, double and long long). A declaration it cannot type raises LciError naming it."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'^\s*(#.*|extern\s+"C"\s*\{|\})\s*$', "", text, flags=re.M)
    sigs = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(.+?) ?\b(lci_\w+) ?\((.*)\)", decl)
        ret = m and m.group(1).replace(" *", "*")
        if not m or ret not in _RETURNS:
            raise LciError(f"include/lci.h: cannot type the declaration `{decl}`")
        args = [a.strip() for a in m.group(3).split(",")]
        argtypes = []
        for a in ([] if args in ([""], ["void"]) else args):
            ctype = ctypes.c_void_p if "*" in a or "[" in a else _SCALARS.get(a.rpartition(" ")[0])
            if ctype is None:
                raise LciError(f"include/lci.h: cannot type the argument `{a}` of `{decl}`")
            argtypes.append(ctype)
        sigs[m.group(2)] = (_RETURNS[ret], argtypes)
    return sigs


@functools.lru_cache(maxsize=None)
def header():
    """(LCI_ABI_VERSION, signatures) of include/lci.h, read once per process."""
    try:
        with open(build_lib.HEADER) as f:
            text = f.read()
    except OSError as e:
        raise LciError(f"{build_lib.HEADER} not readable ({e}): the binding takes every signature from it") from e
    m = re.search(r"^#define\s+LCI_ABI_VERSION\s+(\d+)", text, flags=re.M)
    if not m:
        raise LciError(f"{build_lib.HEADER} defines no LCI_ABI_VERSION")
    return int(m.group(1)), signatures(text)


def __getattr__(name):
    if name == "ABI_VERSION":   # include/lci.h LCI_ABI_VERSION
        return header()[0]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def bind(lib, names=None):
    """Set restype and argtypes of a ctypes.CDLL's functions as include/lci.h declares them: all of them, or `names`."""
    sigs = header()[1]
    for name in sigs if names is None else names:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise LciError(f"{lib._name} does not export {name}, which include/lci.h declares; rebuild with "
                           "`python -m long_context_biomedical_imaging_amd.build_lib`") from None
        fn.restype, fn.argtypes = sigs[name]
    return lib


def load(path: str = LIB_PATH):
    """Load liblci.so and bind every function include/lci.h declares (raises if anything is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise LciError(f"{path} not found: build it with `python -m long_context_biomedical_imaging_amd.build_lib`"
                       " (the HIP path has no CPU fallback)")
    abi_version = header()[0]
    lib = ctypes.CDLL(path)
    if lib.lci_abi_version() != abi_version:   # (before bind: another ABI's library may lack declared symbols)
        raise LciError(f"{path}: ABI version {lib.lci_abi_version()} != {abi_version} expected by this binding; "
                       "rebuild with `python -m long_context_biomedical_imaging_amd.build_lib`")
    bind(lib)
    if path == DEFAULT_LIB and os.path.isdir(os.path.join(HERE, "csrc")):
        want, got = build_lib.source_hash(), lib.lci_build_hash().decode()
        if want != got:
            raise LciError(f"{path} is stale: built from sources {got}, the sources beside it hash to {want}; "
                           "rebuild with `python -m long_context_biomedical_imaging_amd.build_lib`")
    _lib = lib
    return lib


def call(name: str, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise LciError(f"{name} failed (rc={rc}): {lib.lci_last_error().decode()}")


def plain_tensors():
    """Context for building a cached constant tensor. Under torch.inference_mode() (trainer.EvalStep) it leaves that
    mode, so the tensor is a plain one that a later training step may save for its backward; anywhere else it does
    nothing at all (torch.inference_mode(False) would also switch grad mode on inside a no_grad region)."""
    import contextlib
    return torch.inference_mode(False) if torch.is_inference_mode_enabled() else contextlib.nullcontext()


def stream_of(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def c_array(ctype, vals, size=None, pad=0):
    """Host array argument (`const int* geo`, `const long long* strides`, ...): `vals` as a ctypes array of `ctype`,
    padded with `pad` to `size` elements when given (the ABI's int[3] extents are padded with 1)."""
    conv = float if ctype in (ctypes.c_float, ctypes.c_double) else int
    vals = [conv(v) for v in vals]
    return (ctype * (len(vals) if size is None else size))(*vals, *[pad] * ((size or 0) - len(vals)))


def require_gpu(*ts: torch.Tensor):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise LciError("liblci ops run on the GPU only (tensor on %s); there is no CPU path" % t.device)
        if not t.is_contiguous():
            raise LciError("liblci ops need contiguous tensors")
