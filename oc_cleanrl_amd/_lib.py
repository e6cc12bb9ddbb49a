"""ctypes binding of libocppo_hip.so (the C-ABI declared in include/ocppo.h).

torch is imported first on purpose: torch ships libamdhip64.so with soname libamdhip64.so.7, and
libocppo_hip.so's NEEDED entry is that soname, so loading ours after torch reuses torch's HIP
runtime (one runtime per process, shared streams and graph capture).

There is no CPU fallback: if the library is missing, importing this module raises.

include/ocppo.h is the only copy of the C-ABI: SIGNATURES (name -> (restype, [argtypes])) and
every OCPPO_* constant of this module are parsed from it at import. A new entry point is declared
in the header and defined in a .hip file, with OCPPO_ABI_VERSION bumped in the header; nothing
is edited here. A declaration whose types the parser cannot map fails the import.
"""
from __future__ import annotations

import ctypes
import os
import re
from pathlib import Path

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

PKG = Path(__file__).resolve().parent
# OCPPO_LIB: load another build of the same C-ABI (experiments, e.g. a probe variant); default
# is the in-tree build
LIB_PATH = Path(os.environ.get("OCPPO_LIB", PKG / "lib" / "libocppo_hip.so"))
HEADER = PKG.parent / "include" / "ocppo.h"

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
            "float": ctypes.c_float, "ocppo_stream_t": ctypes.c_void_p}


def _ctype(ctype: str, ret: bool = False) -> type | None:
    """ctypes type of one C type as the header spells it, None when it has none here: nothing is
    guessed."""
    words = ctype.replace("*", " * ").split()
    if not re.fullmatch(r"[\w\s*]+", ctype):
        return None
    if "*" in words:
        return ctypes.c_char_p if ret and words == ["const", "char", "*"] else ctypes.c_void_p
    scalar = [w for w in words if w != "const"]
    return _SCALARS.get(scalar[0]) if len(scalar) == 1 else None


def parse_header(text: str) -> tuple[dict[str, tuple[type, list]], dict[str, int]]:
    """(signatures, constants) of a C-ABI header: `name -> (restype, [argtypes])` for every
    `OCPPO_API <return type> <name>(<params>);` and `OCPPO_<NAME> -> value` for every #define of
    a decimal integer. A type outside the mapping of _ctype raises ImportError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {n: int(v) for n, v in
                 re.findall(r"^[ \t]*#[ \t]*define[ \t]+(OCPPO_\w+)[ \t]+(\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    signatures = {}
    for ret, name, params in re.findall(r"\bOCPPO_API\b([\w\s*]*?)\b(\w+)\s*\(([^;]*)\)\s*;", text):
        restype = _ctype(ret, ret=True)
        if restype is None:
            raise ImportError(f"include/ocppo.h: {name}: no ctypes mapping for the return type "
                              f"`{' '.join(ret.split())}`")
        argtypes = []
        for param in [] if params.split() == ["void"] else params.split(","):
            m = re.fullmatch(r"(.*)\b(\w+)", param.strip(), re.S)  # type, then the name
            argtype = _ctype(m.group(1)) if m else None
            if argtype is None:
                raise ImportError(f"include/ocppo.h: {name}: no ctypes mapping for parameter "
                                  f"`{' '.join(param.split())}`")
            argtypes.append(argtype)
        signatures[name] = (restype, argtypes)
    if len(signatures) != len(re.findall(r"\bOCPPO_API\b", text)):
        raise ImportError("include/ocppo.h: an OCPPO_API declaration did not parse (or a name is "
                          "declared twice)")
    return signatures, constants


# the header is the only copy: every OCPPO_* constant below is one of its #defines
SIGNATURES, _CONSTANTS = parse_header(HEADER.read_text())
globals().update(_CONSTANTS)
STAT_NAMES = tuple(n[len("OCPPO_STAT_"):].lower() for n in
                   sorted((n for n in _CONSTANTS if n.startswith("OCPPO_STAT_")),
                          key=_CONSTANTS.get))
if len(STAT_NAMES) != _CONSTANTS["OCPPO_NUM_STATS"]:
    raise ImportError(f"include/ocppo.h: {len(STAT_NAMES)} OCPPO_STAT_* defines, "
                      f"OCPPO_NUM_STATS {_CONSTANTS['OCPPO_NUM_STATS']}")


class OcppoError(RuntimeError):
    """A C-ABI call returned a non-zero status."""


def header_functions() -> list[str]:
    """Names of every function the header declares (the ABI contract)."""
    text = HEADER.read_text()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\s\*]*?\b(ocppo_\w+)\s*\(", text, re.M)))


def _load() -> ctypes.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m oc_cleanrl_amd.build`.")
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    ver = lib.ocppo_abi_version()
    if ver != OCPPO_ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {ver}, expected {OCPPO_ABI_VERSION}; rebuild")
    return lib


LIB = _load()


def call(name: str, *args) -> None:
    """Invoke a status-returning entry point and raise OcppoError on failure."""
    rc = getattr(LIB, name)(*args)
    if rc != OCPPO_OK:
        msg = LIB.ocppo_last_error().decode(errors="replace")
        raise OcppoError(f"{name} failed (status {rc}): {msg}")
