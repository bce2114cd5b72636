"""ctypes binding of ``libphendiff_hip.so``, derived from the C ABI's one definition, ``include/phendiff_hip.h``.

The header is read once, at import (:mod:`phendiff_amd._abi`): every ``typedef struct { ... } pd_foo_bar_args;`` becomes the
``ctypes.Structure`` class ``FooBarArgs`` of this module, every prototype an entry of ``SYMBOLS``, every enumerator and integer
``#define`` a constant.  A new entry point needs its declaration in the header and nothing here, unless it hands a scalar back to the
host through a pointer (``OUT_PARAMS``).

The product path has no CPU fallback: if the shared library is missing or fails to load, importing
:func:`lib` raises.  Build it with ``phendiff_amd/csrc/build.sh`` (``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# PD_LIB: diagnostic override (same-box A/B of two builds of the library, kept OUTSIDE the package under build_ab/); the default
# -- and the only thing the driver ever loads -- is the in-tree build
LIB_PATH = os.environ.get("PD_LIB") or os.path.join(_HERE, "libphendiff_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "phendiff_hip.h")      # the path csrc/source_hash.py hashes


class PhenDiffHipError(RuntimeError):
    pass


def source_hash() -> str:
    """sha256 over the library's sources (csrc/*.hip, csrc/*.h, include/phendiff_hip.h, the build script): identifies the code
    a build / a committed profile belongs to.  The definition lives in csrc/source_hash.py (standalone: build.sh runs it too)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_pd_source_hash", os.path.join(_HERE, "csrc", "source_hash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.source_hash()


def library_is_current() -> bool:
    """True when the loaded library's manifest names the sources in the tree (an in-tree build of this checkout)."""
    import json
    try:
        with open(LIB_PATH + ".manifest.json") as f:
            return json.load(f).get("sources_sha256") == source_hash()
    except (OSError, ValueError):
        return False


vp = C.c_void_p

# The only hand-kept part of the binding: scalars a host caller receives through byref().  Every other pointer parameter is a
# c_void_p (device pointers are passed as integers) or a POINTER of the args struct.
OUT_PARAMS = {("pd_event_elapsed_ms", "ms"): C.POINTER(C.c_float),
              ("pd_comm_query", "rank_out"): C.POINTER(C.c_int), ("pd_comm_query", "world_out"): C.POINTER(C.c_int)}


def read_header(path):
    try:
        with open(path) as f:
            return _abi.read(f.read(), OUT_PARAMS)
    except OSError as e:
        raise PhenDiffHipError(f"cannot read the C ABI's header {path}: {e}") from e


# STRUCTS: C struct name -> class; SYMBOLS: every symbol the header declares, name -> (restype, argtypes); CONSTANTS: name -> int
STRUCTS, SYMBOLS, CONSTANTS = read_header(HEADER_PATH)

globals().update((cls.__name__, cls) for cls in STRUCTS.values())
# the three names the derivation rule does not give
AdamWEmaArgs, LayerNormArgs, LayerNormBwdArgs = AdamwEmaArgs, LayernormArgs, LayernormBwdArgs     # noqa: F821

ABI_VERSION = CONSTANTS["PD_ABI_VERSION"]
PD_F32, PD_BF16, PD_F16 = (CONSTANTS[n] for n in ("PD_F32", "PD_BF16", "PD_F16"))
PD_ERR_SHAPE = CONSTANTS["PD_ERR_SHAPE"]      # pd_status: a shape the entry point refuses before it launches anything
PD_PRED = {"epsilon": CONSTANTS["PD_PRED_EPSILON"], "sample": CONSTANTS["PD_PRED_SAMPLE"], "v_prediction": CONSTANTS["PD_PRED_V"]}
PD_OUT_NHWC, PD_OUT_NCHW_F32, PD_OUT_QKV_HEADS = (CONSTANTS[n] for n in ("PD_OUT_NHWC", "PD_OUT_NCHW_F32", "PD_OUT_QKV_HEADS"))
# pd_sample_stats: the stats row (PD_SS_*), the chunk a workgroup takes and the LDS histogram's limit
SAMPLE_STATS_FIELDS = tuple(n[len("PD_SS_"):].lower() for n in sorted((n for n in CONSTANTS if n.startswith("PD_SS_")), key=CONSTANTS.get))
SAMPLE_STATS_CHUNK = CONSTANTS["PD_SAMPLE_STATS_CHUNK"]
SAMPLE_STATS_MAX_BINS = CONSTANTS["PD_SAMPLE_STATS_MAX_BINS"]
# pd_kid_mmd / pd_feature_moments: the tile of a Gram product and the rows per column-sum chunk
METRIC_STATS_TILE = CONSTANTS["PD_METRIC_STATS_TILE"]
FEATURE_MOMENTS_CHUNK = CONSTANTS["PD_FEATURE_MOMENTS_CHUNK"]
if len(SAMPLE_STATS_FIELDS) != CONSTANTS["PD_SAMPLE_STATS_FIELDS"]:
    raise PhenDiffHipError(f"{HEADER_PATH}: {len(SAMPLE_STATS_FIELDS)} PD_SS_* rows, PD_SAMPLE_STATS_FIELDS = {CONSTANTS['PD_SAMPLE_STATS_FIELDS']}")

_lib = None


def lib():
    """Load (once) and return the HIP library; raises if it is absent -- there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PhenDiffHipError(
            f"{LIB_PATH} not found: build it with phendiff_amd/csrc/build.sh (hipcc --offload-arch=gfx950). "
            "phendiff_amd has no CPU fallback.")
    try:
        l = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise PhenDiffHipError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(l, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if l.pd_abi_version() != ABI_VERSION:
        # same-box A/B against a library built from an older revision (scripts/build_rev.sh, scripts/ab_forward.py): the caller
        # vouches that the structs it exercises did not change between the two
        if not (os.environ.get("PD_ALLOW_ABI_MISMATCH") and LIB_PATH != os.path.join(_HERE, "libphendiff_hip.so")):
            raise PhenDiffHipError(f"ABI mismatch: library {l.pd_abi_version()} != binding {ABI_VERSION}")
    _lib = l
    return l


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().pd_last_error()
        raise PhenDiffHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()
