"""Serial memory round trips in the prologues of the split-16 row kernels, read off the compiled code (no GPU).

A prologue that stages its operands one after another -- loads, wait, convert, LDS write, then the next operand's loads -- pays one
L2-cold round trip per operand while nothing else runs on the chip.  The issue / commit staging of csrc/prd_common.h
requests every operand before the first wait.  This test compiles the three sources device-only with the committed flags and, in each
kernel's text up to its first ``s_barrier``, marks ``global_load*`` / ``buffer_load*`` as L, ``s_waitcnt ... vmcnt`` as W and
``ds_write*`` as D.  A *load run* is a maximal run of L that a W separates from the next L (D does not end a run: only a wait is a round
trip).  Nothing but those four kinds of mnemonics is read.

Counts of the parent of this change, same method, same instantiations:
    pair_tail_h2_kernel<64, 12>              LWD x 13           13   (the bias-head rows sat in a runtime loop: more at run time)
    pair_head_h2_kernel<64, 8>               ...LWDLWDWD...     > 20
    tri_mul_out_proj_kernel<64, 12>          LWD x 9             9
    tri_mul_proj_kernel<64, 12, true>        LWD x 6 + fetch     7
    coord_head_kernel<64, true>              LWD x 4             4
    tri_mul_out_kernel<64, 8, true>          LWD x 3             3
    tri_attn_core_v3_kernel<64, 12, 0, true> LWDWDLWD            3
    tri_attn_out_kernel<64, 12, true>        LWD x 2             2   (still: the conversion gained nothing there and was taken back)
    outer_linear_ks_kernel<64, 4>            LW                  1   (already requests everything up front; not changed)
"""
import os
import re
import subprocess

import pytest

from protein_redesign_amd import build

# at most two runs: the operands, and the first task's rows where the kernel requests them ahead of the barrier
FIXED = {
    "prd_pair.hip": ["pair_tail_h2_kernel<64, 12>", "coord_head_kernel<64, true>", "outer_linear_ks_kernel<64, 4>"],
    "prd_tri.hip": ["tri_mul_out_proj_kernel<64, 12>", "tri_mul_proj_kernel<64, 12, true>", "tri_mul_out_kernel<64, 8, true>",
                    "tri_attn_out_kernel<64, 12, true>"],
    "prd_tri2.hip": ["tri_attn_core_v3_kernel<64, 12, 0, true>"],
}
# pair_head_h2_kernel has runtime-sized operands (dist_dim, C).  Its runs in the text:
#   1  the first chunk of both matrices, the centers and every vector -- at dist_dim 256, C = 128 that is the whole prologue;
#   2  the body of the loop over further chunks (operands larger than the in-flight budget, e.g. dist_dim 632): one run per chunk;
#   3  inside that body hipcc puts a wait before a load whose destination registers the previous chunk's load of the same piece still
#      names (write after write).  It splits the body's loads in the text; at run time the awaited load was consumed by the previous
#      chunk's commit, so the wait falls through.
# 3 is inside the 4 the design allows.
PAIR_HEAD = ("prd_pair.hip", "pair_head_h2_kernel<64, 8>", 3)


def _assembly(src):
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


_CACHE = {}


def kernel_texts(src):
    """{demangled kernel name: its instruction lines} of one source"""
    if src not in _CACHE:
        text = _assembly(src)
        mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        bodies = {}
        for m, name in zip(mangled, build._demangle(mangled)):
            start = text.index("\n" + m + ":")
            end = text.index(".Lfunc_end", start)
            bodies[name] = text[start:end].split("\n")
        _CACHE[src] = bodies
    return _CACHE[src]


def events(lines):
    """the L / W / D string of a kernel's text up to its first barrier, repeats collapsed"""
    ev = []
    for line in lines:
        parts = line.split(None, 1)
        if not parts:
            continue
        op = parts[0]
        if op.startswith("s_barrier"):
            break
        if op.startswith("global_load") or op.startswith("buffer_load"):
            k = "L"
        elif op == "s_waitcnt" and len(parts) > 1 and "vmcnt" in parts[1]:
            k = "W"
        elif op.startswith("ds_write"):
            k = "D"
        else:
            continue
        if not ev or ev[-1] != k:
            ev.append(k)
    else:
        raise AssertionError("kernel has no s_barrier")
    return "".join(ev)


def load_runs(ev):
    return len(re.findall(r"L+", re.sub(r"W+", "W", ev.replace("D", ""))))


def test_counting_method():
    assert load_runs("LWD" * 13) == 13
    assert load_runs("LWDWDWD") == 1
    assert load_runs("LWDWDLWD") == 2
    assert load_runs("LW") == 1
    assert load_runs("LDLWD") == 1          # no wait between the two requests: one round trip


@pytest.mark.parametrize("src,kernel", [(s, k) for s, ks in FIXED.items() for k in ks])
def test_fixed_size_prologue_is_at_most_two_round_trips(src, kernel):
    bodies = kernel_texts(src)
    assert kernel in bodies, (kernel, sorted(k for k in bodies if k.split("<")[0] == kernel.split("<")[0]))
    ev = events(bodies[kernel])
    print(kernel, ev, load_runs(ev))
    # a prologue without a global or buffer load would mean the loads compiled to something this method does not see (flat loads)
    assert ev.startswith("L"), ev
    assert "D" in ev or kernel.startswith("outer_linear_ks"), ev
    assert load_runs(ev) <= 2, (kernel, ev)


def test_pair_head_prologue():
    src, kernel, bound = PAIR_HEAD
    ev = events(kernel_texts(src)[kernel])
    print(kernel, ev, load_runs(ev))
    assert ev.startswith("L"), ev
    assert bound <= 4 and load_runs(ev) <= bound, (kernel, ev)
