"""ctypes binding of libmlagg_hip.so (C ABI: include/mlagg_hip.h).

The ctypes signatures and the integer constants are read from the header itself at import, so the binding cannot drift from the
ABI the library is compiled against.  There is no fallback: if the shared library is absent or a symbol is missing the import of
any op raises, and every non-zero return code of an entry point becomes RuntimeError (the exception type nnU-Net's trainers handle,
reference nnUNetTrainerBenchmark_5epochs.py:25-29)."""
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.path.join(CSRC, "libmlagg_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "mlagg_hip.h")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}


def _ctype(decl, name, is_return=False):
    """ctypes type of a C type `decl` (a parameter without its name, or a return type) of entry point `name`: every pointer is
    c_void_p (device buffers, host arrays and the stream alike), a `const char *` return is c_char_p."""
    t = " ".join(decl.replace("*", " * ").split())
    if t.endswith("*"):
        if not is_return:
            return ctypes.c_void_p
        if t == "const char *":
            return ctypes.c_char_p
    elif t in _SCALARS:
        return _SCALARS[t]
    raise RuntimeError(f"include/mlagg_hip.h: {name}: no ctypes mapping for the type {decl.strip()!r}")


def _parse_header(path):
    """(signatures, constants) of the header: name -> (restype, argtypes) for every mlagg_* declaration, and the value of every
    integer #define MLAGG_*."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    constants = {k: int(v) for k, v in re.findall(r"^#define\s+(MLAGG_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    signatures = {}
    for ret, name, params in re.findall(r"^([\w \t*]+?)\s*\b(mlagg_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        args = []
        for p in params.split(","):
            p = p.strip()
            if p == "void":
                continue
            m = re.fullmatch(r"(.*?[\s*])\s*[A-Za-z_]\w*", p)
            if m is None:
                raise RuntimeError(f"include/mlagg_hip.h: {name}: cannot read the parameter {p!r}")
            args.append(_ctype(m.group(1), name))
        signatures[name] = (_ctype(ret, name, is_return=True), args)
    missed = set(re.findall(r"\b(mlagg_\w+)\s*\(", text)) - set(signatures)
    if missed:
        raise RuntimeError(f"include/mlagg_hip.h: cannot read the declarations of {sorted(missed)}")
    return signatures, constants


# name -> (restype, argtypes), and MLAGG_* -> int
SIGNATURES, CONSTANTS = _parse_header(HEADER)

_handle = None


def build(verbose=False):
    """Compile every HIP source for gfx950 into csrc/libmlagg_hip.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"] + ([] if verbose else ["-s"])
    subprocess.check_call(cmd)


def lib():
    global _handle
    if _handle is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the MI355X ops have no CPU or eager fallback)")
        handle = ctypes.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError if the ABI is incomplete
            fn.restype = res
            fn.argtypes = args
        _handle = handle
    return _handle


def check(code, what):
    if code != 0:
        msg = lib().mlagg_error_string(int(code)).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {code})")


def stream():
    """Raw handle of torch's current HIP stream on the current device.  Every kernel launch asks for it: the two C calls below cost
    0.3 us, `torch.cuda.current_stream().cuda_stream` 9 us (tools/host_profile.py: 2.6 ms of host time per direction and step, and
    the 224 x 224 configurations are bound by the host's enqueue rate)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def launch(name, *args):
    """Call the stream-taking entry point `name` with `args` on torch's current stream (the last parameter of every such entry
    point); a non-zero return raises.  On the host-bound path: one attribute lookup on the library handle, no other work."""
    code = getattr(_handle or lib(), name)(*args, stream())
    if code:
        check(code, name)
