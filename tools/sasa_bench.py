"""Times ``sasa.count`` and ``sasa.measure`` (libprd_sasa.so) beside ``backbone.build`` on the same inputs, at N = 320 and 769 residues
(A = 5 N + 24 ligand atoms), S = 8 and 64 samples, P = 256 points.  Not gated by any test; no speed claim rests on it and no target is
set: the stage runs once per call of generate_samples, after the sampling loop.

    python tools/sasa_bench.py [--out profiles/sasa_bench.txt] [--reps 5] [--calls 20]

The samples are the chains of tests/backbone_ref.py (ideal chains through the anchors in runs of 40 residues, the runs laid side by
side 10 Angstrom apart so that they bury one another, every other sample with sigma = 0.3 Angstrom of noise on the trace); the atoms are
what ``backbone.build`` makes of them, the ligand a random coil of 24 carbons beside the first run.  A window is ``--calls`` back-to-back
calls on the same buffers between two device synchronises, timed with the host clock; the calls are timed in alternation, ``--reps``
windows each, after 3 warm-up calls.  The figure is the median window in us per call with the smallest and largest beside it.  A call
is the Python binding (argument checks, its ``torch.empty``) plus its launch."""
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

SHAPES = ((8, 320), (64, 320), (8, 769), (64, 769))
RUN, NA, P = 40, 24, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sasa_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sasa_bench needs the GPU: a CPU run says nothing about the device path")
    import backbone_ref as BR
    from protein_redesign_amd import backbone as BB
    from protein_redesign_amd import build
    from protein_redesign_amd import sasa as SA
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = [f"sasa_bench: us per call of the Python binding, P = {P}; the atoms are backbone.build's on ideal chains in runs of {RUN}, {NA} ligand atoms",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {a.reps} alternating windows of {a.calls} back-to-back calls "
             f"(host clock between two device synchronises), after 3 warm-up calls"]
    up = SA.upload(SA.Accessibility(points=P), dev)
    for S, N in SHAPES:
        x = np.zeros((S, N, 3))
        for s in range(S):
            for k, r0 in enumerate(range(0, N, RUN)):
                L = min(RUN, N - r0)
                ca = BR.chain(rng, max(L, 4))[:L, BR.CA_]
                x[s, r0: r0 + L] = ca - ca.mean(0) + np.array([k % 5, k // 5, 0.0]) * 10.0
            if s % 2:
                x[s] += BR.SIGMA * rng.normal(size=(N, 3))
        mask = np.ones(N, np.float32)
        link = mask.copy()
        link[RUN - 1:: RUN] = 0.0
        ligand = np.cumsum(rng.normal(size=(S, NA, 3)) * 0.9, 1) + [0.0, 0.0, 6.0]
        x, mask, link, ligand = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev) for t in (x, mask, link, ligand))
        elements = torch.full((NA,), 5, dtype=torch.long, device=dev)
        built = BB.build(x, mask, link, BB.upload("build", dev))
        pos, reach, present, group = SA.flatten(built.atoms, built.built, ligand, elements, mask, up)
        A = pos.shape[1]
        work = [("backbone.build (1 launch)", lambda: BB.build(x, mask, link)),
                ("sasa.count ALL (1 launch)", lambda: SA.count(pos, reach, present, None, SA.ALL, up.sphere)),
                ("sasa.count SAME_GROUP (1 launch)", lambda: SA.count(pos, reach, present, group, SA.SAME_GROUP, up.sphere)),
                ("sasa.measure (2 launches and torch)", lambda: SA.measure(built.atoms, built.built, ligand, elements, mask, up))]
        got = work[3][1]()
        counts = work[1][1]()
        for _, fn in work:
            for _ in range(3):
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
        atoms = int(present.sum())
        lines.append(f"S {S} samples of N {N} residues, A {A} atoms ({atoms // S} present per sample); mean exposed fraction "
                     f"{float(counts.sum()) / (atoms * P):.3f}, buried atoms {float((counts == 0).sum() - (present == 0).sum()) / atoms:.3f}; "
                     f"mean relative area {float(got['relative'].mean()):.3f}, interface {float(got['interface_area'].mean()):.1f} A^2")
        lines.append(f"  {'call':<40} | {'us/call':>10} {'(min':>10} {'max)':>10}")
        for name, _ in work:
            lines.append(f"  {name:<40} | {np.median(us[name]):10.1f} {min(us[name]):10.1f} {max(us[name]):10.1f}")
        lines.append(f"  atom pairs met by the centre test over the whole call time of sasa.count ALL (binding included): "
                     f"{S * float(A) * A / np.median(us[work[1][0]]) / 1e3:.1f} G/s")
    res = build.resource_usage(sources=build.LATER_SIDE_LIBS["sasa"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
