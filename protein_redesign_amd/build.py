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
# The side libraries: post-processing of samples, not part of the denoiser ABI, hence each a library of its own with its own header, so
# that libprd_hip.so, prd_hip.h and their recorded command lines stay what they are; same flags, same compile routine.  Per library:
# its sources, the headers every object of it depends on, the library, and the flag of this module's command line that builds it.
#   align    libprd_align.so (include/prd_align.h): superposition and TM-score of generated samples
#   tmalign  libprd_tmalign.so (include/prd_tmalign.h): structural alignment of samples to a reference of another length
#   quality  libprd_quality.so (include/prd_quality.h): lDDT and pair censuses of samples, no superposition
#   condition  libprd_condition.so (include/prd_condition.h): the kept rows of structure-conditioned sampling (conditioning.py); the one
#            side library the sampling loop itself calls, and only when a scaffold is given
#   sequence  libprd_sequence.so (include/prd_sequence.h): the sequence rules of sampling (sequence.py) -- the ruled rows of seq_t inside
#            the loop, only when rules are given, and the decoding and census of generate_samples(decode=...)
# csrc/prd_superpose.h is the fit that align and tmalign share: touching it makes both stale and no object of the denoiser.
# csrc/prd_launch.h is the host half of every launch, theirs as the denoiser's: touching it makes every object stale.  Each has a
# trace form as well (build_side(name, variant="trace"): objects under csrc/trace, libprd_<name>_trace.so), which build_trace_side links
# tests/native/side_launch_trace.c against.
SideLib = collections.namedtuple("SideLib", "sources headers lib flag")
_INCLUDE, PRD_SUPERPOSE_H, PRD_LAUNCH_H = os.path.join(os.path.dirname(HERE), "include"), os.path.join(CSRC, "prd_superpose.h"), os.path.join(CSRC, "prd_launch.h")


def _side(name, *headers):
    return SideLib([f"prd_{name}.hip"], [os.path.join(_INCLUDE, f"prd_{name}.h"), PRD_LAUNCH_H, *headers], os.path.join(HERE, f"libprd_{name}.so"), f"--{name}")


SIDE_LIBS = {"align": _side("align", PRD_SUPERPOSE_H), "tmalign": _side("tmalign", PRD_SUPERPOSE_H), "quality": _side("quality"),
             "condition": _side("condition"), "sequence": _side("sequence")}
LIB_ALIGN, ALIGN_SOURCES = SIDE_LIBS["align"].lib, SIDE_LIBS["align"].sources
LIB_TMALIGN, TMALIGN_SOURCES = SIDE_LIBS["tmalign"].lib, SIDE_LIBS["tmalign"].sources
LIB_QUALITY, QUALITY_SOURCES = SIDE_LIBS["quality"].lib, SIDE_LIBS["quality"].sources
LIB_CONDITION, CONDITION_SOURCES = SIDE_LIBS["condition"].lib, SIDE_LIBS["condition"].sources
LIB_SEQUENCE, SEQUENCE_SOURCES = SIDE_LIBS["sequence"].lib, SIDE_LIBS["sequence"].sources
# The loop libraries: the same SideLib tuples, the same flags and compile routine (build_side serves both maps), for what runs INSIDE the
# sampling loop without being part of the denoiser ABI.  They are kept apart from SIDE_LIBS because that map is what the side-library
# launch trace (build_trace_side, tests/native/side_launch_trace.c) walks; each source sits in a directory of its own under csrc/.
#   solver   libprd_solver.so (include/prd_solver.h): the step boundary of few-step sampling (solver.py) -- strided ancestral and DDIM
#            loops over K visited levels; called by the sampling loop only when a solver is given
LOOP_LIBS = {"solver": SideLib([os.path.join("solver", "prd_solver.hip")], [os.path.join(_INCLUDE, "prd_solver.h"), PRD_LAUNCH_H],
                               os.path.join(HERE, "libprd_solver.so"), "--solver")}
LIB_SOLVER, SOLVER_SOURCES = LOOP_LIBS["solver"].lib, LOOP_LIBS["solver"].sources
# The step libraries: again the same SideLib tuples, flags and compile routine, for what runs inside a sampling STEP, between the network
# and the boundary, when the caller asks for it.  They are kept apart from both maps above: SIDE_LIBS is what the side-library launch trace
# walks, and LOOP_LIBS is the set of step boundaries (a loop has exactly one of them; its tests pin the map to the solver's).
#   guide    libprd_guide.so (include/prd_guide.h): guided sampling (guidance.py) -- the gradient of a clash and restraint energy on the
#            step's clean-structure estimate, added to the predicted noise; called by the sampling loop only when guidance is given
STEP_LIBS = {"guide": SideLib([os.path.join("guide", "prd_guide.hip")], [os.path.join(_INCLUDE, "prd_guide.h"), PRD_LAUNCH_H],
                              os.path.join(HERE, "libprd_guide.so"), "--guide")}
LIB_GUIDE, GUIDE_SOURCES = STEP_LIBS["guide"].lib, STEP_LIBS["guide"].sources
# The sample libraries: once more the same SideLib tuples, flags and compile routine, for post-processing of samples that was added after
# the side-library launch trace was recorded.  They are kept apart from SIDE_LIBS because that map is what the trace and its recorded
# output walk, and from the two maps above because nothing here runs inside the sampling loop.
#   chirality  libprd_chirality.so (include/prd_chirality.h): the handedness census of samples (chirality.py) -- C-alpha virtual
#            dihedrals and the signed volumes of the ligand's stereocentres, a verdict per sample, the reflection of mirrored samples
SAMPLE_LIBS = {"chirality": SideLib([os.path.join("chirality", "prd_chirality.hip")], [os.path.join(_INCLUDE, "prd_chirality.h"), PRD_LAUNCH_H],
                                    os.path.join(HERE, "libprd_chirality.so"), "--chirality")}
LIB_CHIRALITY, CHIRALITY_SOURCES = SAMPLE_LIBS["chirality"].lib, SAMPLE_LIBS["chirality"].sources
# The history libraries: the same SideLib tuples, flags and compile routine a fifth time, for what runs inside a sampling step AFTER its
# boundary and keeps a history across steps.  They are kept apart from LOOP_LIBS (the step boundaries: a loop has exactly one) and from
# STEP_LIBS (what runs before the boundary), each of which its tests pin to its present contents.
#   multistep  libprd_multistep.so (include/prd_multistep.h): the second- and third-order correction of multistep few-step sampling
#            (solver.py) and the history of clean-structure estimates it reads; called by the sampling loop only under a multistep
#            solver of order 2 or 3
HISTORY_LIBS = {"multistep": SideLib([os.path.join("multistep", "prd_multistep.hip")], [os.path.join(_INCLUDE, "prd_multistep.h"), PRD_LAUNCH_H],
                                     os.path.join(HERE, "libprd_multistep.so"), "--multistep")}
LIB_MULTISTEP, MULTISTEP_SOURCES = HISTORY_LIBS["multistep"].lib, HISTORY_LIBS["multistep"].sources
# The output libraries: the same SideLib tuples, flags and compile routine a sixth time, for what turns finished samples into what
# leaves the project.  They are kept apart from SAMPLE_LIBS and from every map above because each of those is held to its present
# contents by its own tests.
#   backbone  libprd_backbone.so (include/prd_backbone.h): N, C, O and CB of every residue from the C-alpha trace (backbone.py) --
#            the last device stage of generate_samples(backbone=...)
OUTPUT_LIBS = {"backbone": SideLib([os.path.join("backbone", "prd_backbone.hip")], [os.path.join(_INCLUDE, "prd_backbone.h"), PRD_LAUNCH_H],
                                  os.path.join(HERE, "libprd_backbone.so"), "--backbone")}
LIB_BACKBONE, BACKBONE_SOURCES = OUTPUT_LIBS["backbone"].lib, OUTPUT_LIBS["backbone"].sources


def _own_libs():
    """every library with a header of its own: the side libraries, then the loop libraries, the step libraries and the sample libraries"""
    return list(SIDE_LIBS.items()) + list(LOOP_LIBS.items()) + list(STEP_LIBS.items()) + list(SAMPLE_LIBS.items())


def _all_libs():
    """``_own_libs()`` and the history libraries after them.  (The first four maps keep a function of their own because tests of
    theirs hold its value to exactly those four; this one is held to its five in the same way, see ``_every_lib``.)"""
    return _own_libs() + list(HISTORY_LIBS.items())


def _every_lib():
    """``_all_libs()`` and the output libraries after them: what build_side, the header lookup and the command line serve.  (The
    two functions above keep their values because tests hold each to exactly its maps.)"""
    return _all_libs() + list(OUTPUT_LIBS.items())

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
    return next((s.headers for _, s in _every_lib() if src in s.sources), HEADERS)


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
        if not (force or _stale(obj, [spath] + _headers(src))):
            continue
        os.makedirs(os.path.dirname(obj), exist_ok=True)        # a source in a directory of its own keeps its object there
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
    """The side library ``name`` of SIDE_LIBS (or the loop library ``name`` of LOOP_LIBS, or the step library ``name`` of STEP_LIBS, or the sample library ``name`` of SAMPLE_LIBS, or the history library ``name`` of HISTORY_LIBS, or the output library ``name`` of OUTPUT_LIBS): its sources with the committed FLAGS and the shipped variant's extras, objects beside
    the denoiser's.  Not a variant of libprd_hip.so: ``build()`` compiles none of it, and no side library compiles another.
    ``variant="trace"``: the trace variant's flags and object directory, the library libprd_<name>_trace.so."""
    s, v = dict(_every_lib())[name], VARIANTS[variant]
    lib = s.lib if variant == "shipped" else s.lib.replace(".so", f"_{variant}.so")
    return _build(Variant(v.cflags, v.ldflags, v.objdir, lib, None), s.sources, force, verbose)


def build_align(force: bool = False, verbose: bool = True) -> str:
    """libprd_align.so (include/prd_align.h, protein_redesign_amd/align.py)"""
    return build_side("align", force, verbose)


def build_tmalign(force: bool = False, verbose: bool = True) -> str:
    """libprd_tmalign.so (include/prd_tmalign.h, protein_redesign_amd/tmalign.py)"""
    return build_side("tmalign", force, verbose)


def build_quality(force: bool = False, verbose: bool = True) -> str:
    """libprd_quality.so (include/prd_quality.h, protein_redesign_amd/quality.py)"""
    return build_side("quality", force, verbose)


def build_condition(force: bool = False, verbose: bool = True) -> str:
    """libprd_condition.so (include/prd_condition.h, protein_redesign_amd/conditioning.py)"""
    return build_side("condition", force, verbose)


def build_sequence(force: bool = False, verbose: bool = True) -> str:
    """libprd_sequence.so (include/prd_sequence.h, protein_redesign_amd/sequence.py)"""
    return build_side("sequence", force, verbose)


def build_solver(force: bool = False, verbose: bool = True) -> str:
    """libprd_solver.so (include/prd_solver.h, protein_redesign_amd/solver.py)"""
    return build_side("solver", force, verbose)


def build_guide(force: bool = False, verbose: bool = True) -> str:
    """libprd_guide.so (include/prd_guide.h, protein_redesign_amd/guidance.py)"""
    return build_side("guide", force, verbose)


def build_chirality(force: bool = False, verbose: bool = True) -> str:
    """libprd_chirality.so (include/prd_chirality.h, protein_redesign_amd/chirality.py)"""
    return build_side("chirality", force, verbose)


def build_multistep(force: bool = False, verbose: bool = True) -> str:
    """libprd_multistep.so (include/prd_multistep.h, protein_redesign_amd/solver.py)"""
    return build_side("multistep", force, verbose)


def build_backbone(force: bool = False, verbose: bool = True) -> str:
    """libprd_backbone.so (include/prd_backbone.h, protein_redesign_amd/backbone.py)"""
    return build_side("backbone", force, verbose)


def build_asan(verbose: bool = True) -> str:
    """Host-side AddressSanitizer build: libprd_hip_asan.so with the HOST code of every source instrumented
    (-fsanitize=address; device code is compiled as usual: -fno-gpu-sanitize) and the argument-validation driver
    tests/native/host_abi_check.c linked against it.  Runs on a machine without a GPU: every call of
    the driver is rejected by the argument checks before any HIP API is used.  Returns the path of the driver binary."""
    lib = _build(VARIANTS["asan"], SOURCES, verbose=verbose)
    exe = os.path.join(VARIANTS["asan"].objdir, "host_abi_check")
    driver = os.path.join(os.path.dirname(HERE), "tests", "native", "host_abi_check.c")
    if _stale(exe, [driver, lib, PRD_HIP_H]):
        _run([_hipcc(), "-x", "c", driver, "-x", "none", "-g"] + _ASAN + ["-o", exe, lib, "-Wl,-rpath," + HERE], verbose)
    return exe


def build_chirality_check(verbose: bool = True) -> str:
    """Host-side AddressSanitizer build of libprd_chirality.so (the asan variant's flags: host code instrumented, device code as usual)
    and the argument-validation driver tests/native/chirality_abi_check.c linked against it.  Runs on a machine without a GPU: every
    call of the driver is refused before any HIP API is used.  Returns the path of the driver binary."""
    lib = build_side("chirality", verbose=verbose, variant="asan")
    exe = os.path.join(VARIANTS["asan"].objdir, "chirality_abi_check")
    driver = os.path.join(os.path.dirname(HERE), "tests", "native", "chirality_abi_check.c")
    if _stale(exe, [driver, lib, SAMPLE_LIBS["chirality"].headers[0]]):
        _run([_hipcc(), "-x", "c", driver, "-x", "none", "-g"] + _ASAN + ["-o", exe, lib, "-Wl,-rpath," + HERE], verbose)
    return exe


def build_backbone_check(verbose: bool = True) -> str:
    """Host-side AddressSanitizer build of libprd_backbone.so (the asan variant's flags: host code instrumented, device code as usual)
    and the argument-validation driver tests/native/backbone_abi_check.c linked against it.  Runs on a machine without a GPU: every
    call of the driver is refused before any HIP API is used.  Returns the path of the driver binary."""
    lib = build_side("backbone", verbose=verbose, variant="asan")
    exe = os.path.join(VARIANTS["asan"].objdir, "backbone_abi_check")
    driver = os.path.join(os.path.dirname(HERE), "tests", "native", "backbone_abi_check.c")
    if _stale(exe, [driver, lib, OUTPUT_LIBS["backbone"].headers[0]]):
        _run([_hipcc(), "-x", "c", driver, "-x", "none", "-g"] + _ASAN + ["-o", exe, lib, "-Wl,-rpath," + HERE], verbose)
    return exe


def build_trace(verbose: bool = True) -> str:
    """The launch trace (csrc/prd_launch.h under -DPRD_LAUNCH_TRACE): libprd_hip_trace.so, whose launches print a line each instead of
    reaching HIP, and the driver tests/native/launch_trace.c linked against it, which walks the entry points over a sweep of shapes,
    arithmetics and switches.  Host code only; tests/test_launch_trace_cpu.py compares the driver's output with the recorded one.
    Returns the path of the driver binary."""
    lib = _build(VARIANTS["trace"], SOURCES, verbose=verbose)
    exe = os.path.join(VARIANTS["trace"].objdir, "launch_trace")
    driver = os.path.join(os.path.dirname(HERE), "tests", "native", "launch_trace.c")
    if _stale(exe, [driver, lib, PRD_HIP_H]):
        _run([_hipcc(), "-x", "c", driver, "-x", "none", "-O1", "-Wno-format-extra-args", "-o", exe, lib, "-Wl,-rpath," + HERE], verbose)
    return exe


def build_trace_side(verbose: bool = True) -> str:
    """The launch trace of the side libraries: the five libprd_<name>_trace.so and the driver tests/native/side_launch_trace.c linked
    against them, which walks every entry point of their headers over the shapes at which a host decision changes.  Host code only;
    tests/test_launch_trace_cpu.py compares the driver's output with the recorded one.  Returns the path of the driver binary."""
    libs = [build_side(name, verbose=verbose, variant="trace") for name in SIDE_LIBS]
    exe = os.path.join(VARIANTS["trace"].objdir, "side_launch_trace")
    driver = os.path.join(os.path.dirname(HERE), "tests", "native", "side_launch_trace.c")
    if _stale(exe, [driver] + libs + [s.headers[0] for s in SIDE_LIBS.values()]):
        _run([_hipcc(), "-x", "c", driver, "-x", "none", "-O1", "-Wno-format-extra-args", "-o", exe] + libs + ["-Wl,-rpath," + HERE], verbose)
    return exe


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
    for side, s in _every_lib():
        if s.flag in sys.argv:
            print(build_side(side, force="--force" in sys.argv))
            sys.exit(0)
    if "--resources" in sys.argv:                   # the denoiser's kernels, then those of each side, loop and step library
        for sources in [SOURCES] + [s.sources for _, s in _every_lib()]:
            for name, u in sorted(resource_usage(verbose=True, sources=sources).items()):
                print(f"{u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}")
        sys.exit(0)
    if "--asan" in sys.argv:
        exe = build_asan()
        sys.exit(subprocess.call([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")))
    build(force="--force" in sys.argv)
