"""Times ``backbone.build`` (libprd_backbone.so) at S = 64 samples of N = 384 rows: 64 ligand atoms and 320 residues.  Not gated by any
test; no speed claim rests on it and no target is set.

    python tools/backbone_bench.py [--out profiles/backbone_bench.txt] [--reps 9] [--calls 2000]

The samples are the chains of tests/backbone_ref.py (ideal chains through the anchors in runs of 40 residues, every other sample with
sigma = 0.3 Angstrom of noise).  A window is ``--calls`` back-to-back calls on the same buffers between two device synchronises, timed
with the host clock; the call and an empty-kernel-sized control (``torch.Tensor.zero_`` on S ints) are timed in alternation, ``--reps``
windows each, after 50 warm-up calls.  The figure is the median window in us per call with the smallest and largest beside it.  A call
is the Python binding (argument checks, two ``torch.empty``) plus one launch: back to back the launches overlap the host work, so the
figure is the larger of the two, which is what a caller of the binding sees."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

S, NA, NR, RUN = 64, 64, 320, 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone_bench.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("backbone_bench needs the GPU: a CPU run says nothing about the device path")
    import backbone_ref as BR
    from protein_redesign_amd import backbone as BB
    from protein_redesign_amd import build
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    N = NA + NR
    x = np.zeros((S, N, 3))
    for s in range(S):
        x[s, :NA] = rng.normal(size=(NA, 3)) * 4.0
        for r0 in range(NA, N, RUN):
            ca = BR.chain(rng, RUN)[:, BR.CA_]
            x[s, r0: r0 + RUN] = ca - ca.mean(0) + rng.integers(-2, 3, 3) * 15.0
        if s % 2:
            x[s] += BR.SIGMA * rng.normal(size=(N, 3))
    mask = np.r_[np.zeros(NA), np.ones(NR)].astype(np.float32)
    link = mask.copy()
    link[NA + RUN - 1:: RUN] = 0.0
    x, mask, link = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev) for t in (x, mask, link))
    up = BB.upload("build", dev)
    small = torch.zeros(S, dtype=torch.int32, device=dev)
    work = [(f"build (S {S}, N {N})", lambda: BB.build(x, mask, link, up)), (f"control: Tensor.zero_ on {S} ints", lambda: small.zero_())]
    got = work[0][1]()
    for _, fn in work:
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in work}
    for _ in range(a.reps):
        for name, fn in work:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / a.calls * 1e6)
    whole = (got.built == 31).sum(1)
    lines = [f"backbone_bench: us per call of the Python binding, S {S} samples of N {N} rows ({NA} ligand atoms, {NR} residues in runs of {RUN})",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {a.reps} alternating windows of {a.calls} back-to-back calls "
             f"(host clock between two device synchronises), after 50 warm-up calls",
             f"inputs: residues built whole per sample, ideal chains {int(whole[0::2].min())} .. {int(whole[0::2].max())}, with sigma {BR.SIGMA} Angstrom of "
             f"noise {int(whole[1::2].min())} .. {int(whole[1::2].max())}, of {NR}",
             f"{'call':<52} | {'us/call':>9} {'(min':>8} {'max)':>8}"]
    for name, _ in work:
        lines.append(f"{name:<52} | {np.median(us[name]):9.2f} {min(us[name]):8.2f} {max(us[name]):8.2f}")
    read, written = N * 20 * S, N * 64 * S
    lines.append(f"the launch reads {read} bytes and writes {written} ({(read + written) / 1e6:.2f} MB in all): it is bound by launch and binding "
                 "overhead at this size, not by memory")
    res = build.resource_usage(sources=build.SIDE_LIBS["backbone"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
