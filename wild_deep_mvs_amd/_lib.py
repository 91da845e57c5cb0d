"""ctypes binding of libpscv.so (the C ABI declared in include/pscv.h).

The library is built in-tree by ``wild_deep_mvs_amd/csrc/Makefile`` (``__graft_entry__.build()``)
and must be present: there is no PyTorch / CPU fallback for the hot path.  ``lib()`` raises
``PscvMissingError`` when the shared object cannot be loaded.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PSCV_LIB") or os.path.join(_HERE, "libpscv.so")     # (PSCV_LIB: A/B builds of scripts/dev)
CSRC = os.path.join(_HERE, "csrc")

HEADER = os.path.join(os.path.dirname(_HERE), "include", "pscv.h")

_RET = {"const char*": C.c_char_p, "int": C.c_int, "long": C.c_long}
_SCALAR = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double}
_PROTO = re.compile(r"(const char\*|int|long) (pscv_\w+)\(([^()]*)\)")


def _param_type(param: str):
    """`const char*` -> c_char_p, a pointer to pointers (a host array of device pointers) -> POINTER(c_void_p), any other pointer ->
    c_void_p, int / long / float / double by name; anything else raises."""
    if "*" in param:
        if param.count("*") >= 2:
            return C.POINTER(C.c_void_p)
        return C.c_char_p if re.fullmatch(r"const char\s*\*\s*\w*", param) else C.c_void_p
    ctype = re.sub(r"\s*\b\w+$", "", param)          # drop the parameter's name
    if ctype not in _SCALAR:
        raise ValueError(f"pscv.h: no ctypes type for parameter '{param}'")
    return _SCALAR[ctype]


def parse_header(text: str):
    """(prototypes, constants) of the C ABI: {name: (restype, [argtypes])} for every `pscv_x(...);` declaration and {NAME: int} for
    every `#define PSCV_NAME <int>`.  Whatever is left of the header after comments, preprocessor lines and the extern "C" braces is
    a sequence of prototypes; a statement that is not one, or a parameter type the tables above do not know, raises ValueError."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^#define PSCV_(\w+) (-?\d+)\s*$", text, flags=re.M)}
    text = re.sub(r'^\s*(#.*|extern "C" \{|\})$', "", text, flags=re.M)
    protos = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = _PROTO.fullmatch(stmt)
        if m is None:
            raise ValueError(f"pscv.h: not a prototype: '{stmt[:80]}'")
        params = [] if m[3].strip() in ("", "void") else [p.strip() for p in m[3].split(",")]
        protos[m[2]] = (_RET[m[1]], [_param_type(p) for p in params])
    return protos, consts


with open(HEADER) as _fh:
    PROTOTYPES, _CONSTS = parse_header(_fh.read())
EXPORTS = tuple(PROTOTYPES)
# The constants the package and its users read (a #define that is not a plain integer would be missing here: fail at import)
CONSTANTS = ("ABI_VERSION", "F32", "BF16", "F16", "GEOM_PROJ", "GEOM_HOMOG", "COST_VARIANCE", "COST_VARIANCE_CVP", "COST_SOFTMIN",
             "COST_GROUPCORR", "COST_WARP_ONLY", "COST_VARIANCE_PARTIAL", "CONV_S1", "CONV_S2", "CONV_T2", "CONV_S1P8", "CONV_S1C1",
             "CONV_T2P8", "EPI_RELU_PRE", "EPI_RELU_POST", "MAX_SRC", "CAM_FLOATS", "GEO_MAX_SRC", "GEO_CAM_FLOATS", "FUSE_MAX_VIEWS",
             "PM_MAX_SRC", "PM_MAX_RADIUS", "PM_MAX_TOPK", "LOSS_GT_PLAIN", "LOSS_GT_BAYES", "LOSS_L_PLAIN", "LOSS_L_BAYES",
             "LOSS_MAX_TERMS", "METRIC_MAX_THRESH", "METRIC_SUMS", "AUG_NONE", "AUG_BRIGHTNESS", "AUG_CONTRAST", "AUG_MAX_VIEWS")
_missing = [n for n in CONSTANTS if n not in _CONSTS]
if _missing:
    raise ImportError(f"include/pscv.h does not define PSCV_{_missing[0]} as an integer")
globals().update(_CONSTS)


class PscvMissingError(RuntimeError):
    pass


class PscvError(RuntimeError):
    pass


_lock = threading.Lock()
_lib = None


STAMP_PATH = os.path.join(CSRC, ".build_stamp")


def source_hash() -> str:
    """sha256 over every file the library is compiled from (csrc/*.hip|h|cpp, the Makefile, include/pscv.h)."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp")) or f == "Makefile")
    for path in [os.path.join(CSRC, f) for f in files] + [HEADER]:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def build(verbose: bool = False, force: bool = False) -> str:
    """Compile libpscv.so for gfx950 with hipcc (cross-compiles without a GPU).  File times do not survive a copy of the tree, so
    the decision is by CONTENT: the sources' hash is stored next to the objects (csrc/.build_stamp); a library built from other
    sources (or none) is rebuilt from scratch with `make -B`, otherwise `make` only links what is missing.  Prints which happened."""
    want = source_hash()
    have = open(STAMP_PATH).read().strip() if os.path.exists(STAMP_PATH) else ""
    fresh = force or have != want or not os.path.exists(LIB_PATH)
    cmd = ["make", "-C", CSRC, "-j8"] + (["-B"] if fresh else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise RuntimeError("building libpscv.so failed")
    with open(STAMP_PATH, "w") as fh:
        fh.write(want + "\n")
    print(f"[pscv build] {'full rebuild (make -B): sources changed or no stamp' if fresh else 'up to date: sources match the stamp of the built library'}"
          f" [{want[:12]}]", flush=True)
    return LIB_PATH


def _declare(lib):
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes


def lib():
    """The loaded library (loads on first use; import torch first so that its HIP runtime is the one
    both sides share -- both carry SONAME libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise PscvMissingError(
                    f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(or make -C wild_deep_mvs_amd/csrc). The plane-sweep engine has no CPU / PyTorch fallback.")
            try:
                import torch  # noqa: F401  (loads torch's libamdhip64 first)
            except Exception:  # pragma: no cover
                pass
            try:
                handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
            except OSError as e:
                raise PscvMissingError(f"cannot load {LIB_PATH}: {e}") from e
            _declare(handle)
            ver = handle.pscv_abi_version()
            if ver != ABI_VERSION:
                raise PscvMissingError(f"libpscv.so ABI {ver} != binding ABI {ABI_VERSION}: rebuild")
            _lib = handle
    return _lib


TUNING_GEN = 0      # bumped by every knob change: captured hipGraphs (graph.replayable) froze the kernel selection of their capture


def set_tuning(key: str, value: int) -> None:
    """Process-wide: also seen by launches from other host threads (autograd's backward thread, DataParallel replicas)."""
    global TUNING_GEN
    TUNING_GEN += 1
    check(lib().pscv_set_tuning(key.encode(), int(value)), "pscv_set_tuning")


def get_tuning(key: str) -> int:
    """The value the calling thread's next launch would use."""
    v = C.c_int(0)
    check(lib().pscv_get_tuning(key.encode(), C.byref(v)), "pscv_get_tuning")
    return int(v.value)


_thread_overrides = threading.local()     # .keys: the knobs the calling thread overrides (set_tuning_thread)


def set_tuning_thread(key: str, value: int, enable: bool = True) -> None:
    """Override (or, enable=False, stop overriding) a knob for the calling host thread only."""
    global TUNING_GEN
    TUNING_GEN += 1
    check(lib().pscv_set_tuning_thread(key.encode(), int(value), 1 if enable else 0), "pscv_set_tuning_thread")
    keys = _thread_overrides.__dict__.setdefault("keys", set())
    keys.add(key) if enable else keys.discard(key)


@contextlib.contextmanager
def tuning(**knobs: int):
    """`with tuning(warp_tiled=0, conv_wide=2): ...` sets process-wide knobs and puts back what they held before, also when the
    body raises.  Blocks nest.  get_tuning reports the calling thread's override where one is set, which is not the value to put
    back: entering with such a knob raises."""
    mine = getattr(_thread_overrides, "keys", ())
    for key in knobs:
        if key in mine:
            raise PscvError(f"tuning({key}=...): this thread overrides '{key}' (set_tuning_thread); the process-wide value cannot be read")
    saved = {key: get_tuning(key) for key in knobs}
    try:
        for key, value in knobs.items():
            set_tuning(key, value)
        yield
    finally:
        for key, value in saved.items():
            set_tuning(key, value)


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().pscv_last_error().decode("utf-8", "replace")
        raise PscvError(f"{what} failed (rc={rc}): {msg}")
