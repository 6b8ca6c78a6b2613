"""ctypes binding of libprd_hip.so (include/prd_hip.h).  The product path is HIP only: importing an
operator without the built library, or calling it on a CPU tensor, raises -- there is no fallback."""
from __future__ import annotations

import collections
import ctypes as C
import os
import re

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRD_LIB", os.path.join(HERE, "libprd_hip.so"))   # PRD_LIB: experiment builds

vp, ci, cf, cz, cll = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_longlong


# ---- the binding is read from include/prd_hip.h: the header is the only statement of the C ABI ----------------------------------
_SCALARS = {"int": ci, "float": cf, "size_t": cz, "long long": cll, "hipStream_t": vp}
Entry = collections.namedtuple("Entry", "argtypes restype inject at")     # inject: "arith" / "tune" / None, at: its parameter index


class PrdGemm(C.Structure):
    pass                                    # _fields_: the header's struct, below


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def _declarator(decl, where, header="include/prd_hip.h"):
    """(ctypes type, name) of one C parameter or struct member such as ``const float* bias``.  A type outside the map raises."""
    m = re.fullmatch(r"(.*?)\s*(\w+)", " ".join(decl.split()))
    ctype = m.group(1).replace(" *", "*") if m else ""
    if ctype == "const char*":
        return C.c_char_p, m.group(2)
    if ctype == "const PrdGemm*":
        return C.POINTER(PrdGemm), m.group(2)
    if "*" in ctype:
        return vp, m.group(2)
    if ctype not in _SCALARS:
        raise TypeError(f"{header}, {where}: no ctypes type for {decl.strip()!r}")
    return _SCALARS[ctype], m.group(2)


def parse_struct(text, name):
    """ctypes ``_fields_`` of ``typedef struct name { ... } name;`` (members such as ``int M, N, K;`` share their type)."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _strip_comments(text), flags=re.S).group(1)
    fields = []
    for decl in filter(str.strip, body.split(";")):
        first, *more = decl.split(",")
        ctype, member = _declarator(first, "struct " + name)
        fields += [(member, ctype)] + [(m.strip(), ctype) for m in more]
    return fields


def parse_header(text, header="include/prd_hip.h"):
    """{entry point: Entry} for every ``int`` / ``size_t prd_*(...);`` prototype of the header text.  The injection rule is the
    header's own: a parameter named ``arith`` or ``tune`` is the last one, or the last before ``stream``; elsewhere it raises.
    ``header``: the name the text goes by in those messages."""
    entries = {}
    for ret, name, params in re.findall(r"^(int|size_t)\s+(prd_\w+)\s*\(([^)]*)\)\s*;", _strip_comments(text), flags=re.M):
        decls = [] if params.strip() in ("", "void") else [_declarator(p, name, header) for p in params.split(",")]
        names = [n for _, n in decls]
        hits = [i for i, n in enumerate(names) if n in ("arith", "tune")]
        if len(hits) > 1 or (hits and hits[0] != len(names) - 1 and not (hits[0] == len(names) - 2 and names[-1] == "stream")):
            raise ValueError(f"{header}, {name}: `arith` / `tune` must be the last parameter or the last before `stream`")
        entries[name] = Entry([t for t, _ in decls], _SCALARS[ret], names[hits[0]] if hits else None, hits[0] if hits else None)
    return entries


def parse_defines(text, prefix):
    """{macro without ``prefix``: value} of the header's ``#define <prefix>NAME <integer>`` lines (``(-3)`` is an integer too)."""
    return {n: int(v) for n, v in re.findall(r"^[ \t]*#define[ \t]+%s(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$" % re.escape(prefix), _strip_comments(text), flags=re.M)}


def parse_tune(text):
    """({macro without PRD_TUNE_: bits}, shift of PRD_TUNE(), (mask, shift) of PRD_TUNE_TA2_FLAGS()) from the header's #defines."""
    text = _strip_comments(text)
    bits = {n: int(a) << int(b) for n, a, b in re.findall(r"#define\s+PRD_TUNE_(\w+)\s+\((\d+)\s*<<\s*(\d+)\)", text)}
    bits["TA_VARIANT_MASK"] = int(re.search(r"#define\s+PRD_TUNE_TA_VARIANT_MASK\s+(\d+)", text).group(1))
    shift = int(re.search(r"#define\s+PRD_TUNE\(switches\)\s+\(\(switches\)\s*<<\s*(\d+)\)", text).group(1))
    flags = re.search(r"#define\s+PRD_TUNE_TA2_FLAGS\(f\)\s+\(PRD_TUNE_TA2_FLAGS_SET\s*\|\s*\(\(\(f\)\s*&\s*(\d+)\)\s*<<\s*(\d+)\)\)", text)
    return bits, shift, (int(flags.group(1)), int(flags.group(2)))


with open(os.path.join(os.path.dirname(HERE), "include", "prd_hip.h")) as _f:
    _HEADER = _f.read()
PrdGemm._fields_ = parse_struct(_HEADER, "PrdGemm")
ENTRIES = parse_header(_HEADER)
SIGNATURES = {name: e.argtypes for name, e in ENTRIES.items()}          # name -> argtypes
_TUNE, _TUNE_SHIFT, (_FLAGS_MASK, _FLAGS_SHIFT) = parse_tune(_HEADER)

GEMM_MODES = {"fp32": 0, "split16": 1, "bf16x3": 1}      # "bf16x3": earlier name of the split-operand mode
DEFAULT_GEMM_MODE = "split16"       # process default of the Python host side (env PRD_GEMM_MODE overrides)

# A/B environment variable, its default, {value: PRD_TUNE_* switch that value sets}
_TUNE_ENV = (
    ("PRD_TA2_V3", 1, {0: "TA2_NO_V3"}),
    ("PRD_TA2_LONG", 1, {0: "TA2_NO_LONG"}),
    ("PRD_OL_VARIANT", 0, {1: "OL_GEN2"}),
    ("PRD_TMS_NW", 8, {12: "TMS_NW12", 16: "TMS_NW16"}),
    ("PRD_GEMM_KG", 1, {0: "GEMM_NO_KG"}),
    ("PRD_GEMM_SLAB", 1, {0: "GEMM_NO_SLAB"}),
    ("PRD_GEMM_BRING", 1, {0: "GEMM_NO_BATCHED_RING"}),
    ("PRD_GEMM_XCDCOLS", 0, {1: "GEMM_XCD_COLS"}),
    ("PRD_TA2_TAIL", 1, {0: "TA2_NO_TAIL_SPLIT"}),
    ("PRD_TA2_XCD8", 1, {0: "TA2_NO_XCD8"}),
    ("PRD_TA2_GV", 1, {0: "TA2_NO_GV"}),
    ("PRD_TMP_NW", 12, {16: "TMP_NW16"}),
)


def tune_from_env(env=None) -> int:
    """The PRD_TUNE_* switch word (prd_hip.h) from the A/B environment variables -- read HERE, on the host side: the library
    itself never looks at the environment."""
    env = os.environ if env is None else env

    def geti(name, default):
        v = env.get(name)
        return default if v is None or v == "" else int(v)

    t = geti("PRD_TA_VARIANT", 0) & _TUNE["TA_VARIANT_MASK"]
    for name, default, switches in _TUNE_ENV:
        switch = switches.get(geti(name, default))
        if switch:
            t |= _TUNE[switch]
    f = geti("PRD_TA2_FLAGS", -1)
    if f >= 0:
        t |= _TUNE["TA2_FLAGS_SET"] | ((f & _FLAGS_MASK) << _FLAGS_SHIFT)
    if geti("PRD_TMS_DEPTH", 2) == 3 and geti("PRD_TMS_NW", 8) == 8:         # three chunks in flight: the 8-wave contraction only
        t |= _TUNE["TMS_DEPTH3"]
    return t


ABI_VERSION = 101          # include/prd_hip.h PRD_VERSION this binding is written against (101: prd_step_boundary's sync = 2 int32)


class _Library:
    """The loaded C library plus the ONE piece of state of the host side: the arithmetic (prd_hip.h: PRD_ARITH_*) that the
    Python operators pass to every call.  The C ABI itself is stateless; ``prd_set_gemm_mode`` / ``prd_get_gemm_mode`` live
    here, in the host language, with the names round 2 used so that callers and tests read the same."""

    def __init__(self, cdll, mode: int, tune: int = 0):
        self._cdll = cdll
        self._mode = mode
        self._tune = tune               # PRD_TUNE_* switches (A/B measurements), injected with the arithmetic
        self._wrapped = {}

    def prd_set_tune(self, tune: int) -> int:
        if tune < 0 or tune >= (1 << 23):
            return -1
        self._tune = int(tune)
        return 0

    def prd_get_tune(self) -> int:
        return self._tune

    def prd_set_gemm_mode(self, mode: int) -> int:
        if mode not in (0, 1):
            return -1
        self._mode = int(mode)
        return 0

    def prd_get_gemm_mode(self) -> int:
        return self._mode

    def __getattr__(self, name):
        fn = self._wrapped.get(name)
        if fn is None:
            raw = getattr(self._cdll, name)
            e = ENTRIES.get(name)
            kind = (e.inject, e.at == len(e.argtypes) - 2) if e else (None, False)          # (what, before the stream?)
            if kind == ("arith", True):
                def fn(*args, _raw=raw):
                    return _raw(*args[:-1], self._mode | (self._tune << _TUNE_SHIFT), args[-1])
            elif kind == ("arith", False):
                def fn(*args, _raw=raw):
                    return _raw(*args, self._mode | (self._tune << _TUNE_SHIFT))
            elif kind == ("tune", True):
                def fn(*args, _raw=raw):
                    return _raw(*args[:-1], self._tune, args[-1])
            elif kind == ("tune", False):
                def fn(*args, _raw=raw):
                    return _raw(*args, self._tune)
            else:
                fn = raw
            self._wrapped[name] = fn
        return fn


def load_library(path, entries, version_export, version, flag=""):
    """The C library at ``path`` with the argtypes / restype of ``entries`` (a parsed header) set on its entry points.  Raises
    RuntimeError (never falls back) when it has not been built, or when ``version_export()`` is not the ``version`` the binding
    was written against.  ``flag``: what ``python -m protein_redesign_amd.build`` takes to build it."""
    how = " ".join(["python -m protein_redesign_amd.build"] + [flag] * bool(flag))
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `{how}` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    cdll = C.CDLL(path)
    for name, e in entries.items():
        fn = getattr(cdll, name)
        fn.argtypes, fn.restype = e.argtypes, e.restype
    got = getattr(cdll, version_export)()
    if got != version:
        raise RuntimeError(f"{path} reports {version_export.upper()} {got}, this binding was written against {version} "
                           f"(the header lists what changed): rebuild with `{how}`")
    return cdll


_lib = None


def lib():
    """The loaded library; raises RuntimeError (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        cdll = load_library(LIB_PATH, ENTRIES, "prd_version", ABI_VERSION)
        mode = os.environ.get("PRD_GEMM_MODE", DEFAULT_GEMM_MODE)
        if os.environ.get("PRD_BF16X3"):                               # older spelling of PRD_GEMM_MODE=bf16x3
            mode = "bf16x3"
        if mode not in GEMM_MODES:
            raise RuntimeError(f"PRD_GEMM_MODE must be one of {sorted(GEMM_MODES)}, got {mode!r}")
        _lib = _Library(cdll, GEMM_MODES[mode], tune_from_env())
    return _lib


def arith() -> int:
    """The arithmetic the operators pass to the library (PRD_ARITH_FP32 = 0 / PRD_ARITH_SPLIT16 = 1)."""
    return lib().prd_get_gemm_mode()


ARITH_NAMES = {0: "fp32 (PRD_ARITH_FP32)", 1: "split16 (PRD_ARITH_SPLIT16)"}


class arithmetic:
    """``with arithmetic("fp32"): ...`` -- the operators called inside pass that arithmetic to the library; the previous default
    comes back on exit (also on an exception).  ``None`` leaves the default alone.  The library itself is stateless (prd_hip.h):
    this only changes what the Python binding injects, so it is a fresh CALL in another arithmetic, never a re-exec."""

    def __init__(self, mode):
        if isinstance(mode, str):
            if mode not in GEMM_MODES:
                raise ValueError(f"arithmetic must be one of {sorted(GEMM_MODES)}, got {mode!r}")
            mode = GEMM_MODES[mode]
        self.mode = mode
        self.prev = None

    def __enter__(self):
        if self.mode is not None:
            self.prev = lib().prd_get_gemm_mode()
            if lib().prd_set_gemm_mode(self.mode) != 0:
                raise ValueError(f"invalid arithmetic {self.mode!r}")
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            lib().prd_set_gemm_mode(self.prev)
        return False


class NonFiniteError(RuntimeError):
    """A sampling loop or an optimisation step produced inf / NaN (see ProteinReDiffModel.nonfinite_policy)."""


def row_gemm_description(b3: bool) -> str:
    """What the GEMMs of the pair kernels compute in, for bench.py's JSON line (stated truthfully, not as a precision claim)."""
    if b3:
        return ("split16: fp32 operands split into fp16 hi + lo (both rounded to nearest: 24 bits; 3 products hi*hi + hi*lo + lo*hi) "
                "and multiplied on the fp16 MFMA pipe with fp32 accumulation -- the row GEMMs of the pair track, the node-row "
                "linears of the single track (incl. SPAttention's logits / P*V), the coordinate head, the triangle-multiplication contraction, "
                "Q*K^T and P*V of the triangle attention; "
                "the single-track attention core and pair_bias run fp32 MFMA / FMA.  "
                "Parity tolerances are the same as in fp32 mode (PRD_GEMM_MODE=fp32)")
    return "fp32-mfma"


_DEFINES = parse_defines(_HEADER, "PRD_")


def check(code: int, what: str, defines=_DEFINES, prefix: str = "PRD_", unsupported: str = None):
    """Raise for the non-zero return ``code`` of the entry point ``what``: a RuntimeError that names the ``ERR_*`` macro of the header
    (``defines``: its parsed #defines, ``prefix``: what parse_defines took off their names) or the hipError_t.  ``unsupported``, if
    given: ERR_UNSUPPORTED is a limit the caller can act on, and becomes a ValueError that states it."""
    if code != 0:
        name = next((n for n, v in defines.items() if n.startswith("ERR_") and v == code), None)
        if unsupported and name == "ERR_UNSUPPORTED":
            raise ValueError(f"{what}: {unsupported}")
        raise RuntimeError(f"{what} failed: {prefix + name if name else 'hipError_t ' + str(code)}")


def dptr(t, dtype=torch.float32):
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("protein_redesign_amd operators run on the GPU only (got a CPU tensor); "
                           "there is no CPU fallback")
    if t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("expected a contiguous tensor")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the side libraries (the rows of build.SIDE_LIBS and build.MORE_SIDE_LIBS): one binding, one statement of their argument checks ----
class SideLibrary:
    """The binding of ``libprd_<name>.so`` beside the package, derived from the name: ``include/prd_<name>.h`` is read and parsed here
    (``entries``, and ``defines`` without their ``PRD_<NAME>_`` prefix), the library itself is loaded on the first ``lib()``.  ``version``:
    the ``PRD_<NAME>_VERSION`` the calling module is written against; ``limit``: what ERR_UNSUPPORTED means to a caller, a sentence in
    which ``{MAX_N}`` and the like stand for the header's defines."""

    def __init__(self, name: str, version: int, limit: str):
        self.name, self.version, self.prefix = name, version, f"PRD_{name.upper()}_"
        with open(os.path.join(os.path.dirname(HERE), "include", f"prd_{name}.h")) as f:
            text = f.read()                     # the header is the only statement of the C ABI and of its constants
        self.entries = parse_header(text, f"include/prd_{name}.h")
        self.defines = parse_defines(text, self.prefix)
        self.limit = limit.format(**self.defines)
        self._cdll = None

    def lib(self):
        """The loaded library; raises RuntimeError (never falls back) when it has not been built."""
        if self._cdll is None:
            self._cdll = load_library(os.path.join(HERE, f"libprd_{self.name}.so"), self.entries, f"prd_{self.name}_version", self.version,
                                      f"--{self.name}")
        return self._cdll

    def check(self, code: int, what: str):
        check(code, what, self.defines, self.prefix, self.limit)


def structures(t, name, *, runs, letter, N=None, bounds=None):
    """[K,N,3] fp32 device tensor whose last stride is 1 (made so if it is not); returns (tensor, structure stride, row stride).
    ``letter``: what the messages call the first dimension; ``runs``: the subject and verb of the "GPU only" message; ``N``: the
    positions expected; ``bounds``: the SideLibrary whose ``MAX_S`` / ``MAX_N`` are refused here already, or None."""
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name} must be a [{letter},N,3] tensor, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if N is not None and t.shape[1] != N:
        raise ValueError(f"{name} has {t.shape[1]} positions, expected {N}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: {runs} on the GPU only (got a CPU tensor); there is no CPU fallback")
    if bounds is not None and (t.shape[1] > bounds.defines["MAX_N"] or t.shape[0] > bounds.defines["MAX_S"]):
        raise ValueError(f"{name}: {t.shape[0]} structures of {t.shape[1]} positions, at most {bounds.defines['MAX_S']} structures "
                         f"({bounds.prefix}MAX_S) of {bounds.defines['MAX_N']} positions ({bounds.prefix}MAX_N) are supported")
    if t.stride(2) != 1 or t.stride(1) < 3 or t.stride(0) < 0:
        t = t.contiguous()
    return t, t.stride(0), t.stride(1)


def position_mask(mask, name, N, device):
    """``mask`` as a contiguous [N] fp32 (0 / 1) tensor on ``device``, or ValueError"""
    if not torch.is_tensor(mask) or mask.shape != (N,):
        raise ValueError(f"{name} must be a [{N}] tensor, got {tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__}")
    if mask.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (0 / 1), got {mask.dtype}")
    if mask.device != device:
        raise ValueError(f"{name} is on {mask.device}, the structures on {device}")
    return mask.contiguous()
