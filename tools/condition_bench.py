"""Times one replayed step of the reverse-diffusion loop without a scaffold, with ``Scaffold("outside")`` (one more launch per step:
prd_condition_rows) and with ``Scaffold("outside", sequence=True)`` (two more: prd_single_init after it), at the shape and model of
bench.py.  Not gated by any test.

    python tools/condition_bench.py [--out profiles/condition_bench.txt] [--reps 7] [--steps 200]

Shapes: 64 atoms + 256 residues (N = 320, bench.py's default) and 64 + 705 (N = 769), one sample.  The three loops live in ONE process
and are timed in alternation -- a window of ``--steps`` replayed steps of each, ``--reps`` times round-robin -- so that drift of the box
falls on all three alike; a window is a host clock around work that ends in a device synchronise, after the eager step, the graph
capture and 10 warm-up steps of every loop.  The figure is the median window in ms/step, with the smallest and largest beside it: the
spread of the unconditioned series is the yardstick for the differences."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(64, 256), (64, 705)]
VARIANTS = [("unconditioned", None), ("Scaffold('outside')", dict()), ("Scaffold('outside', sequence=True)", dict(sequence=True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "condition_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("condition_bench needs the GPU: a CPU run says nothing about the device path")
    import bench
    from protein_redesign_amd import build
    from protein_redesign_amd.conditioning import Scaffold
    from protein_redesign_amd.diffusion_model import ReverseDiffusion
    from protein_redesign_amd.synthetic import NoiseSource, batch_to, synthetic_batch
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_model(dev)
    lines = [f"condition_bench: ms per replayed step, model of bench.py (S {bench.S}, P {bench.P}, {bench.NB} blocks, T {bench.T}), one sample, "
             f"mask_prob 0.3 (the kept rows: the 70 % of the residues outside the design region)",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {a.reps} alternating windows of {a.steps} steps "
             f"(host clock to a device synchronise), after capture and 10 warm-up steps",
             f"{'N':>5} {'loop':<36} | {'ms/step':>9} {'(min':>8} {'max)':>8} | {'vs unconditioned':>17}"]
    for atoms, residues in SHAPES:
        loops = []
        for name, kw in VARIANTS:
            batch = batch_to(synthetic_batch([(atoms, residues)], seed=0), dev)
            loop = ReverseDiffusion(model, batch, [NoiseSource(0, 0)], **({} if kw is None else {"scaffold": Scaffold("outside", **kw)}))
            for _ in range(12):                 # eager step, capture, warm-up
                loop.step()
            loops.append((name, loop))
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in loops}
        for _ in range(a.reps):
            for name, loop in loops:
                if loop.steps_done + a.steps > loop.T:
                    loop.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loop.step()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
        base = float(np.median(ms[loops[0][0]]))
        for name, loop in loops:
            assert loop.finite(), name
            med = float(np.median(ms[name]))
            lines.append(f"{atoms + residues:5d} {name:<36} | {med:9.4f} {min(ms[name]):8.4f} {max(ms[name]):8.4f} | {med - base:+13.4f} ms")
        del loops
    res = build.resource_usage(sources=build.SIDE_LIBS["condition"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
