"""Build libprd_hip.so in-tree with hipcc for gfx950 (no CMake / JIT cache: the .so travels with the repo)."""
import collections
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libprd_hip.so")
SOURCES = ["prd_gemm.hip", "prd_pair.hip", "prd_tri.hip", "prd_tri2.hip", "prd_bwd.hip", "prd_spa.hip", "prd_tri_heads.hip", "prd_tri_heads_bwd.hip", "prd_mask.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]
# per-source extras.  prd_tri2: the softmax arithmetic is placed by hand between the MFMAs of the key loop; the SLP vectoriser
# would pack its scalar fp32 adds into v_pk_add_f32 (slower beside MFMAs on gfx950) and move them out of their slots
EXTRA_FLAGS = {"prd_tri2.hip": ["-fno-slp-vectorize"]}
PRD_HIP_H = os.path.join(os.path.dirname(HERE), "include", "prd_hip.h")
# every object depends on these (prd_launch.h: the host half of every launch -- the checked launch, the pair_dim dispatch, the geometry)
HEADERS = [os.path.join(CSRC, "prd_common.h"), os.path.join(CSRC, "prd_launch.h"), os.path.join(CSRC, "prd_tri2_v3_body.inc"), PRD_HIP_H]
# The side libraries: what samples pass through around the denoiser, not part of its ABI, hence each a library of its own
# (libprd_<name>.so) with a header of its own (include/prd_<name>.h) and one source (csrc/prd_<name>.hip), so that libprd_hip.so,
# prd_hip.h and their recorded command lines stay what they are.  Same flags, same compile routine (build_side); a row states the three
# things in which they differ: the name, an extra header, and whether the recorded side-launch trace walks the library.
# Per library: what it is (the module that binds it); when the sampling loop calls it.
#   align      superposition and TM-score of samples (align.py); after the loop, generate_samples(align_to=...)
#   tmalign    structural alignment of samples to a reference of another length (tmalign.py); after the loop
#   quality    lDDT and pair censuses of samples, no superposition (quality.py); after the loop, generate_samples(assess=...)
#   condition  the kept rows of structure-conditioned sampling (conditioning.py); inside the loop, only when a scaffold is given
#   sequence   sequence rules, device decoding and census (sequence.py); inside the loop when rules are given, decode=... after it
#   solver     the step boundary of few-step sampling, strided ancestral and DDIM (solver.py); ends every step under a solver
#   guide      the gradient of a clash and restraint energy on the predicted noise (guidance.py); before the boundary, under guidance
#   chirality  the handedness census of samples, a verdict each, the reflection of mirrored ones (chirality.py); after the loop
#   multistep  the order-2 and order-3 correction of multistep sampling and its history (solver.py); after the boundary, at those orders
#   backbone   N, C, O and CB of every residue from the C-alpha trace (backbone.py); the last device stage, generate_samples(backbone=...)
#   dssp       hydrogen bonds and the eight DSSP classes of the built atoms (dssp.py); after backbone, generate_samples(secondary=...)
#   sasa       Shrake-Rupley point counts of every atom: burial and the ligand interface (sasa.py); after backbone, generate_samples(accessibility=...)
# csrc/prd_superpose.h is the fit that align and tmalign share: touching it makes both stale and no object of the denoiser.
# csrc/prd_launch.h is the host half of every launch, theirs as the denoiser's: touching it makes every object stale.  Each has a
# trace form as well (build_side(name, variant="trace"): objects under csrc/trace, libprd_<name>_trace.so); build_trace_side links
# tests/native/side_launch_trace.c against those of the ``traced`` rows, the five that existed when its output was recorded.
SideLib = collections.namedtuple("SideLib", "sources headers lib flag traced")
_INCLUDE, PRD_SUPERPOSE_H, PRD_LAUNCH_H = os.path.join(os.path.dirname(HERE), "include"), os.path.join(CSRC, "prd_superpose.h"), os.path.join(CSRC, "prd_launch.h")


def _side(name, *headers, traced=False):
    return SideLib([f"prd_{name}.hip"], [os.path.join(_INCLUDE, f"prd_{name}.h"), PRD_LAUNCH_H, *headers], os.path.join(HERE, f"libprd_{name}.so"), f"--{name}", traced)


SIDE_LIBS = {"align": _side("align", PRD_SUPERPOSE_H, traced=True), "tmalign": _side("tmalign", PRD_SUPERPOSE_H, traced=True),
             "quality": _side("quality", traced=True), "condition": _side("condition", traced=True), "sequence": _side("sequence", traced=True),
             "solver": _side("solver"), "guide": _side("guide"), "chirality": _side("chirality"), "multistep": _side("multistep"),
             "backbone": _side("backbone")}
# The second table: side libraries added after the first one was closed.  SIDE_LIBS, the top level of csrc/ and the command lines of its
# ten rows are pinned as they stand by the tests that were written with them, so a later library is a row HERE -- the same row type, the
# same flags, the same compile routine -- with its source and its private headers under csrc/side/ and its objects beside them
# (csrc/side/prd_<name>.o; <variant objdir>/side/ for a variant).  csrc/side/prd_dssp_energy.h is the one statement of the hydrogen-bond
# energy, shared by both roles of the sweep.  ``side_lib(name)`` finds a row in either table.
MORE_SIDE_LIBS = {"dssp": SideLib(["side/prd_dssp.hip"], [os.path.join(_INCLUDE, "prd_dssp.h"), PRD_LAUNCH_H, os.path.join(CSRC, "side", "prd_dssp_energy.h")],
                                  os.path.join(HERE, "libprd_dssp.so"), "--dssp", False)}


# The third table, and the LAST one: the contents of the first two, the listing of csrc/side/ and what ``all_side_libs()`` returns are
# pinned by the tests written with them, so neither can take a row.  A library added from now on is a row HERE -- the same row type, the
# same flags, the same compile routine -- and a directory csrc/<name>/ of its own, its object beside its source (<variant objdir>/<name>/
# for a variant).  No fourth table is needed for the next one: the tests of a row of this table speak of that row alone, never of the
# table's whole contents or of a directory listing.


def _later(name, *headers):
    return SideLib([f"{name}/prd_{name}.hip"], [os.path.join(_INCLUDE, f"prd_{name}.h"), PRD_LAUNCH_H, *headers], os.path.join(HERE, f"libprd_{name}.so"),
                   f"--{name}", False)


LATER_SIDE_LIBS = {"sasa": _later("sasa")}


def side_lib(name):
    """the row of the side library ``name``, from any of the three tables"""
    return every_side_lib()[name]


def all_side_libs():
    """{name: row} of the first two tables, the first table first (what it returned when the second was closed)"""
    return {**SIDE_LIBS, **MORE_SIDE_LIBS}


def every_side_lib():
    """{name: row} of all three tables, in the order of the tables"""
    return {**SIDE_LIBS, **MORE_SIDE_LIBS, **LATER_SIDE_LIBS}

# A variant of the library: flags added to every compile, flags added to the link, object directory, library, and -- for a variant
# that differs from the shipped one by a macro alone -- that macro: a source that never tests it shares the shipped object.
Variant = collections.namedtuple("Variant", "cflags ldflags objdir lib macro")
_ASAN = ["-fsanitize=address", "-fno-gpu-sanitize"]         # host code only: GPU ASan is not available on this pool
VARIANTS = {
    # (-Rpass-analysis: the per-kernel resource remarks of THIS compilation are kept in csrc/resource_usage.json)
    "shipped": Variant(["-Rpass-analysis=kernel-resource-usage", "-fno-caret-diagnostics"], [], CSRC, LIB, None),
    "ab": Variant(["-DPRD_AB"], [], os.path.join(CSRC, "ab"), os.path.join(HERE, "libprd_hip_ab.so"), "PRD_AB"),
    "timing": Variant(["-DPRD_TIMING"], [], os.path.join(CSRC, "timing"), os.path.join(HERE, "libprd_hip_timing.so"), None),
    # every launch replaced by a printed line (csrc/prd_launch.h): host code is what it is about, so the device code, which no call of
    # this library reaches, is compiled without optimisation (a tenth of the time)
    "trace": Variant(["-DPRD_LAUNCH_TRACE", "-Xarch_device", "-O0"], [], os.path.join(CSRC, "trace"), os.path.join(HERE, "libprd_hip_trace.so"), None),
    "asan": Variant(["-g"] + _ASAN + ["-fno-omit-frame-pointer"], _ASAN, os.path.join(CSRC, "asan"), os.path.join(HERE, "libprd_hip_asan.so"), None),
}

RESOURCE_JSON = os.path.join(CSRC, "resource_usage.json")     # per kernel: VGPRs, AGPRs, SGPRs, scratch bytes / lane, occupancy, LDS


def _demangle(names):
    """c++filt on the mangled kernel names; template arguments kept, the anonymous namespace and the parameter list dropped."""
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return list(names)
    res = []
    for n in out[:len(names)]:
        n = n.replace("(anonymous namespace)::", "")
        if n.startswith("void "):
            n = n[5:]
        depth, cut = 0, len(n)
        for i, ch in enumerate(n):          # the first '(' outside the template brackets starts the parameter list
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = i
                break
        res.append(n[:cut].strip())
    return res


def parse_resource_usage(stderr_text):
    """{kernel name: {vgprs, agprs, sgprs, scratch, occupancy, lds}} from hipcc -Rpass-analysis=kernel-resource-usage remarks."""
    import re
    blocks = re.split(r"remark: Function Name: ", stderr_text)[1:]
    mangled, rows = [], []
    for b in blocks:
        def g(key, b=b):
            m = re.search(key + r": (\d+)", b)
            return int(m.group(1)) if m else None
        mangled.append(b.split()[0])
        rows.append({"vgprs": g("VGPRs"), "agprs": g("AGPRs"), "sgprs": g("SGPRs"), "scratch": g(r"ScratchSize \[bytes/lane\]"),
                     "occupancy": g(r"Occupancy \[waves/SIMD\]"), "lds": g(r"LDS Size \[bytes/block\]")})
    return dict(zip(_demangle(mangled), rows))


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _headers(src):
    """the headers an object of ``src`` depends on"""
    return next((s.headers for s in every_side_lib().values() if src in s.sources), HEADERS)


def _stamp(src):
    return max(os.path.getmtime(d) for d in [os.path.join(CSRC, src)] + _headers(src))


def _resources(update=None):
    """csrc/resource_usage.json as a dict ({} when missing or unreadable); ``update``, if any, is merged in and stored first."""
    have = {}
    try:
        with open(RESOURCE_JSON) as f:
            have = json.load(f)
    except (OSError, ValueError):
        pass
    if update:
        have.update(update)
        try:
            with open(RESOURCE_JSON, "w") as f:
                json.dump(have, f, indent=1, sort_keys=True)
        except OSError:
            pass
    return have


def resource_usage(verbose: bool = False, sources=None):
    """Register / scratch / occupancy figures of every kernel of the library, as the compiler reports them for the committed flags
    (hipcc cross-compiles without a GPU).  ``build()`` writes them next to the objects; a source whose figures are missing is
    analysed here (device code only, nothing linked).  tests/test_build_resources.py holds the default-dispatch kernels of the
    sampling step to ScratchSize == 0.  ``sources``: another list than the denoiser library's (that of a side library)."""
    sources = SOURCES if sources is None else sources
    have, new = _resources(), {}
    for src in sources:
        if src in have and have[src].get("stamp") == _stamp(src):
            continue
        cmd = [_hipcc()] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(CSRC, src), "-o", os.devnull]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"resource analysis of {src} failed:\n{r.stderr[-2000:]}")
        new[src] = {"stamp": _stamp(src), "kernels": parse_resource_usage(r.stderr)}
    have = _resources(new)
    return {k: v for src in sources for k, v in have[src]["kernels"].items()}


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _build(v: Variant, sources, force: bool = False, verbose: bool = True) -> str:
    """Compile ``sources`` into the variant's object directory and link its library; only what is stale, unless ``force``."""
    os.makedirs(v.objdir, exist_ok=True)
    objs = []
    for src in sources:
        spath = os.path.join(CSRC, src)
        if not os.path.exists(spath):
            raise FileNotFoundError(f"HIP source listed in build.py is missing: {spath}")
        if v.macro:
            with open(spath) as f:
                if v.macro not in f.read():
                    objs.append(os.path.join(CSRC, src.replace(".hip", ".o")))
                    continue
        obj = os.path.join(v.objdir, src.replace(".hip", ".o"))
        objs.append(obj)
        os.makedirs(os.path.dirname(obj), exist_ok=True)          # a source of the later tables lies in a subdirectory, and so does its object
        if not (force or _stale(obj, [spath] + _headers(src))):
            continue
        cmd = [_hipcc()] + FLAGS + EXTRA_FLAGS.get(src, []) + v.cflags + ["-c", spath, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise subprocess.CalledProcessError(r.returncode, cmd)
        for line in r.stderr.splitlines():                      # warnings stay visible, the remarks do not
            if "remark:" not in line and line.strip():
                sys.stderr.write(line + "\n")
        kernels = parse_resource_usage(r.stderr)                  # only the shipped variant asks for the remarks
        if kernels:
            _resources({src: {"stamp": _stamp(src), "kernels": kernels}})
    if force or _stale(v.lib, objs):
        _run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + v.ldflags + ["-o", v.lib] + objs, verbose)
    return v.lib


def build(force: bool = False, verbose: bool = True) -> str:
    return _build(VARIANTS["shipped"], SOURCES, force, verbose)


def build_side(name: str, force: bool = False, verbose: bool = True, variant: str = "shipped") -> str:
    """The side library ``name`` of SIDE_LIBS, MORE_SIDE_LIBS or LATER_SIDE_LIBS: its source with the committed FLAGS and the shipped variant's extras, its object beside
    the denoiser's.  Not a variant of libprd_hip.so: ``build()`` compiles none of it, and no side library compiles another.
    Another ``variant`` ("trace", "asan"): that variant's flags and object directory, the library libprd_<name>_<variant>.so."""
    s, v = side_lib(name), VARIANTS[variant]
    lib = s.lib if variant == "shipped" else s.lib.replace(".so", f"_{variant}.so")
    return _build(Variant(v.cflags, v.ldflags, v.objdir, lib, None), s.sources, force, verbose)


def _link_driver(variant, name, libs, headers, flags, verbose):
    """The stand-alone C program tests/native/<name>.c, linked against ``libs`` (found at run time beside this file) into the variant's
    object directory; only when it is older than its source, a library or a header.  Returns the path of the binary."""
    exe = os.path.join(VARIANTS[variant].objdir, name)
    driver = os.path.join(os.path.dirname(HERE), "tests", "native", name + ".c")
    if _stale(exe, [driver] + libs + headers):
        _run([_hipcc(), "-x", "c", driver, "-x", "none"] + flags + ["-o", exe] + libs + ["-Wl,-rpath," + HERE], verbose)
    return exe


def build_asan(verbose: bool = True) -> str:
    """Host-side AddressSanitizer build: libprd_hip_asan.so with the HOST code of every source instrumented
    (-fsanitize=address; device code is compiled as usual: -fno-gpu-sanitize) and the argument-validation driver
    tests/native/host_abi_check.c linked against it.  Runs on a machine without a GPU: every call of
    the driver is rejected by the argument checks before any HIP API is used.  Returns the path of the driver binary."""
    lib = _build(VARIANTS["asan"], SOURCES, verbose=verbose)
    return _link_driver("asan", "host_abi_check", [lib], [PRD_HIP_H], ["-g"] + _ASAN, verbose)


def build_side_check(name: str, verbose: bool = True) -> str:
    """The same for the side library ``name``: libprd_<name>_asan.so and the argument-validation driver
    tests/native/<name>_abi_check.c linked against it.  Runs on a machine without a GPU: every call of the driver is refused before
    any HIP API is used.  Returns the path of the driver binary."""
    lib = build_side(name, verbose=verbose, variant="asan")
    return _link_driver("asan", f"{name}_abi_check", [lib], side_lib(name).headers[:1], ["-g"] + _ASAN, verbose)


def build_trace(verbose: bool = True) -> str:
    """The launch trace (csrc/prd_launch.h under -DPRD_LAUNCH_TRACE): libprd_hip_trace.so, whose launches print a line each instead of
    reaching HIP, and the driver tests/native/launch_trace.c linked against it, which walks the entry points over a sweep of shapes,
    arithmetics and switches.  Host code only; tests/test_launch_trace_cpu.py compares the driver's output with the recorded one.
    Returns the path of the driver binary."""
    lib = _build(VARIANTS["trace"], SOURCES, verbose=verbose)
    return _link_driver("trace", "launch_trace", [lib], [PRD_HIP_H], ["-O1", "-Wno-format-extra-args"], verbose)


def build_gemm_dispatch(verbose: bool = True) -> str:
    """The launch trace of single calls of the GEMM family: the same libprd_hip_trace.so and the driver tests/native/gemm_dispatch_trace.c
    linked against it, which reads one case per line from stdin (tests/gemm_cases.py), calls prd_gemm / prd_ln_rows / prd_softmax_rows /
    prd_single_fc1_folded or one of their host queries with dummy addresses and prints the library's launch lines and the return code.
    Host code only; tests/test_gemm_dispatch_cpu.py reads its output.  Returns the path of the driver binary."""
    lib = _build(VARIANTS["trace"], SOURCES, verbose=verbose)
    return _link_driver("trace", "gemm_dispatch_trace", [lib], [PRD_HIP_H], ["-O1"], verbose)


def build_trace_side(verbose: bool = True) -> str:
    """The launch trace of the side libraries: libprd_<name>_trace.so of the five ``traced`` rows and the driver
    tests/native/side_launch_trace.c linked against them, which walks every entry point of their headers over the shapes at which a
    host decision changes.  Host code only; tests/test_launch_trace_cpu.py compares the driver's output with the recorded one.
    Returns the path of the driver binary."""
    traced = [name for name, s in SIDE_LIBS.items() if s.traced]
    libs = [build_side(name, verbose=verbose, variant="trace") for name in traced]
    return _link_driver("trace", "side_launch_trace", libs, [SIDE_LIBS[name].headers[0] for name in traced], ["-O1", "-Wno-format-extra-args"], verbose)


def build_ab(verbose: bool = True) -> str:
    """libprd_hip_ab.so: the library with -DPRD_AB, i.e. INCLUDING the superseded kernels the shipped library leaves out (the
    first-generation split-16 attention cores of csrc/prd_tri.hip, in their three wave-count forms, and the fused form built on
    them).  For A/B measurements (PRD_LIB=<path> PRD_TA_VARIANT=10 ...) and for the parity tests of those kernels, which
    tests/test_ab_build.py runs against this library in a child process."""
    build(verbose=verbose)                                   # sources that never test PRD_AB share the shipped objects
    return _build(VARIANTS["ab"], SOURCES, verbose=verbose)


def build_timing(verbose: bool = True) -> str:
    """Diagnostic build with in-kernel cycle stamps (-DPRD_TIMING: tools/ta_timing.py, tools/phase_timing.py read them through
    prd_debug_read); load it with PRD_LIB=<path>.  Never the shipped library: the stamps cost ~10 % of a wave's cycles."""
    return _build(VARIANTS["timing"], SOURCES, verbose=verbose)


if __name__ == "__main__":
    if "--ab" in sys.argv:
        print(build_ab())
        sys.exit(0)
    if "--timing" in sys.argv:
        print(build_timing())
        sys.exit(0)
    if "--trace" in sys.argv:
        sys.exit(subprocess.call([build_trace()]))
    if "--trace-side" in sys.argv:
        sys.exit(subprocess.call([build_trace_side()]))
    for side, s in every_side_lib().items():
        if s.flag in sys.argv:
            print(build_side(side, force="--force" in sys.argv))
            sys.exit(0)
    if "--resources" in sys.argv:                   # the denoiser's kernels, then those of each side library
        for sources in [SOURCES] + [s.sources for s in every_side_lib().values()]:
            for name, u in sorted(resource_usage(verbose=True, sources=sources).items()):
                print(f"{u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}")
        sys.exit(0)
    if "--asan" in sys.argv:
        exe = build_asan()
        sys.exit(subprocess.call([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")))
    build(force="--force" in sys.argv)
