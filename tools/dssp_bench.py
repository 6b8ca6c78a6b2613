"""Times ``dssp.hbonds`` and ``dssp.assign`` (libprd_dssp.so) beside ``backbone.build`` on the same inputs, at S = 64 samples of
N = 320 residues and at S = 8 of N = 769.  Not gated by any test; no speed claim rests on it and no target is set: the stage runs once
per call of generate_samples, after the sampling loop.

    python tools/dssp_bench.py [--out profiles/dssp_bench.txt] [--reps 9] [--calls 2000]

The samples are the chains of tests/backbone_ref.py (ideal chains through the anchors in runs of 40 residues, every other sample with
sigma = 0.3 Angstrom of noise on the trace); the atoms are what ``backbone.build`` makes of them.  A window is ``--calls`` back-to-back
calls on the same buffers between two device synchronises, timed with the host clock; the calls and an empty-kernel-sized control
(``torch.Tensor.zero_`` on S ints) are timed in alternation, ``--reps`` windows each, after 50 warm-up calls.  The figure is the median
window in us per call with the smallest and largest beside it.  A call is the Python binding (argument checks, its ``torch.empty``)
plus its launches: back to back the launches overlap the host work, so the figure is the larger of the two, which is what a caller of
the binding sees."""
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

SHAPES = ((64, 320), (8, 769))
RUN = 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dssp_bench.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dssp_bench needs the GPU: a CPU run says nothing about the device path")
    import backbone_ref as BR
    from protein_redesign_amd import backbone as BB
    from protein_redesign_amd import build
    from protein_redesign_amd import dssp as DS
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = ["dssp_bench: us per call of the Python binding; the atoms are backbone.build's on ideal chains in runs of " + str(RUN),
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {a.reps} alternating windows of {a.calls} back-to-back calls "
             f"(host clock between two device synchronises), after 50 warm-up calls"]
    for S, N in SHAPES:
        x = np.zeros((S, N, 3))
        for s in range(S):
            for r0 in range(0, N, RUN):
                L = min(RUN, N - r0)
                ca = BR.chain(rng, max(L, 4))[:L, BR.CA_]
                x[s, r0: r0 + L] = ca - ca.mean(0) + rng.integers(-2, 3, 3) * 15.0
            if s % 2:
                x[s] += BR.SIGMA * rng.normal(size=(N, 3))
        mask = np.ones(N, np.float32)
        link = mask.copy()
        link[RUN - 1:: RUN] = 0.0
        x, mask, link = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(dev) for t in (x, mask, link))
        up = BB.upload("build", dev)
        built = BB.build(x, mask, link, up)
        small = torch.zeros(S, dtype=torch.int32, device=dev)
        work = [("backbone.build (1 launch)", lambda: BB.build(x, mask, link, up)),
                ("dssp.hbonds (1 launch)", lambda: DS.hbonds(built.atoms, built.built, link)),
                ("dssp.assign (3 launches: hbonds, flags, classes)", lambda: DS.assign(built.atoms, built.built, link)),
                (f"control: Tensor.zero_ on {S} ints", lambda: small.zero_())]
        got = work[2][1]()
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
        counts = DS.census(got, mask)["counts"].sum(0).tolist()
        lines.append(f"S {S} samples of N {N} residues; {S * N * N * 2 / 1e6:.1f} M pair energies per hbonds launch; classes of the inputs: "
                     + " ".join(f"{DS.ALPHABET[k]}={c}" for k, c in enumerate(counts)))
        lines.append(f"  {'call':<52} | {'us/call':>9} {'(min':>8} {'max)':>8}")
        for name, _ in work:
            lines.append(f"  {name:<52} | {np.median(us[name]):9.2f} {min(us[name]):8.2f} {max(us[name]):8.2f}")
        rate = S * N * N * 2 / np.median(us[work[1][0]]) / 1e3
        lines.append(f"  pair energies over the whole call time of dssp.hbonds (binding included, not a kernel time): {rate:.1f} G/s")
    res = build.resource_usage(sources=build.MORE_SIDE_LIBS["dssp"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
