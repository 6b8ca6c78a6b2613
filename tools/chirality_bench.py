"""Times ``chirality.census`` and ``chirality.reflect`` (libprd_chirality.so) at S = 64 samples of N = 384 rows: 64 ligand atoms with 8
stereocentres and 320 residues.  Not gated by any test; no speed claim rests on it.

    python tools/chirality_bench.py [--out profiles/chirality_bench.txt] [--reps 9] [--calls 2000]

The samples are the chains of tests/chirality_ref.py (helical, extended and mixed segments), so every class and both hands occur.  A
window is ``--calls`` back-to-back calls of one function on the same buffers between two device synchronises, timed with the host clock;
the two functions and an empty-kernel-sized control (``torch.Tensor.zero_`` on S ints) are timed in alternation, ``--reps`` windows
each, after 50 warm-up calls.  The figure is the median window in us per call with the smallest and largest beside it.  A call is the
Python binding (argument checks, six ``torch.empty``) plus one launch: back to back the launches overlap the host work, so the figure is
the larger of the two, which is what a caller of the binding sees.  The control says what that floor is for one small launch."""
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

S, NA, NR, C = 64, 64, 320, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chirality_bench.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chirality_bench needs the GPU: a CPU run says nothing about the device path")
    import chirality_ref as CR
    from protein_redesign_amd import build
    from protein_redesign_amd import chirality as CH
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    N = NA + NR
    xs, link = [], None
    for s in range(S):
        prot, lk = CR.structure(rng, NR, CR.ALL if s % 2 else (CR.KINDS[s % 4],), ideal=s % 2 == 0)
        xs.append(np.concatenate([rng.normal(size=(NA, 3)) * 4.0, prot]))
        link = lk if link is None else link
    x = torch.from_numpy(np.stack(xs).astype(np.float32)).to(dev)
    mask = torch.cat([torch.zeros(NA), torch.ones(NR)]).to(dev)
    links = torch.cat([torch.zeros(NA), torch.from_numpy(link).float()]).to(dev)
    base = np.arange(C) * 7
    centres = CH.upload(np.stack([base, base + 1, base + 2, base + 3], 1), dev)
    cref = torch.from_numpy(CR.signed_volume(np.stack(xs)[0], centres.host.numpy()).astype(np.float32)).to(dev)
    flip = (torch.arange(S, device=dev) % 2).to(torch.int32)
    small = torch.zeros(S, dtype=torch.int32, device=dev)
    work = [("census (S 64, N 384, C 8, with a centre reference)", lambda: CH.census(x, mask, links, centres=centres, centre_ref=cref)),
            ("reflect (half of the samples flagged)", lambda: CH.reflect(x, flip)),
            ("control: Tensor.zero_ on 64 ints", lambda: small.zero_())]
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
    counts = got.counts.sum(0).tolist()
    lines = [f"chirality_bench: us per call of the Python binding, S {S} samples of N {N} rows ({NA} ligand atoms, {NR} residues), {C} centres",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {a.reps} alternating windows of {a.calls} back-to-back calls "
             f"(host clock between two device synchronises), after 50 warm-up calls",
             f"inputs: quads {counts[4]}, helical right / left {counts[0]} / {counts[1]}, extended native / mirror {counts[2]} / {counts[3]}; "
             f"verdicts +1 / -1 / 0: {int((got.verdict > 0).sum())} / {int((got.verdict < 0).sum())} / {int((got.verdict == 0).sum())}",
             f"{'call':<52} | {'us/call':>9} {'(min':>8} {'max)':>8}"]
    for name, _ in work:
        lines.append(f"{name:<52} | {np.median(us[name]):9.2f} {min(us[name]):8.2f} {max(us[name]):8.2f}")
    moved = N * 28 * S + N * 8 * S
    lines.append(f"the census reads {N * 28 * S} bytes and writes {N * 8 * S + S * 40 + S * C * 4} ({moved / 1e6:.2f} MB in all): it is bound by launch and "
                 "binding overhead at this size, not by memory")
    res = build.resource_usage(sources=build.SIDE_LIBS["chirality"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
