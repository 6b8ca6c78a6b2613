"""Times the reverse-diffusion loop under a multistep solver against the ddim loop on the same levels, at the shapes and model of
bench.py.  Not gated by any test.

    python tools/multistep_bench.py [--out profiles/multistep_bench.txt] [--reps 7] [--steps 18]

Shapes: 64 atoms + 256 residues (N = 320, bench.py's default) and 64 + 705 (N = 769), one sample, T = 1000, K = 20 levels spaced in
log-SNR.

ms per replayed step: ``Solver(timesteps=<the levels>, kind="ddim")`` (one boundary launch per step), ``Solver.multistep(K, order=2)`` and
``order=3`` (the boundary and one launch of prd_multistep_correct).  The three loops live in ONE process and are timed in alternation -- a
window of ``--steps`` replayed steps of each, ``--reps`` times round-robin -- so that drift of the box falls on all three alike; a window is
a host clock around work that ends in a device synchronise, after the eager step and the graph capture of every loop (every loop is
reset before a window: it has only K - 2 replayed steps).  The figure is the median window, with the smallest and largest beside it;
whether the windows of a multistep loop overlap those of the ddim loop is stated per line."""
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
K = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistep_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=K - 2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multistep_bench needs the GPU: a CPU run says nothing about the device path")
    if not 1 <= a.steps <= K - 2:
        raise SystemExit(f"--steps must lie in [1, {K - 2}]: a K = {K} loop replays K - 2 steps after its eager step and its capture")
    import bench
    from protein_redesign_amd import build
    from protein_redesign_amd.diffusion_model import ReverseDiffusion
    from protein_redesign_amd.solver import Solver
    from protein_redesign_amd.synthetic import NoiseSource, batch_to, synthetic_batch
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_model(dev)
    levels = Solver.multistep(K).levels(bench.T, schedule=model.diffusion_schedule)
    variants = [(f"ddim on the same {K} levels", Solver(timesteps=levels[::-1], kind="ddim")),
                (f"Solver.multistep({K}, order=2)", Solver.multistep(K, order=2)), (f"Solver.multistep({K}, order=3)", Solver.multistep(K, order=3))]
    lines = [f"multistep_bench: model of bench.py (S {bench.S}, P {bench.P}, {bench.NB} blocks, T {bench.T}), one sample, mask_prob 0.3",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"levels (log-SNR spacing): {levels}",
             f"ms per replayed step: median of {a.reps} alternating windows of {a.steps} steps (host clock to a device synchronise), after "
             "the eager step and the capture",
             f"{'N':>5} {'loop':<30} | {'ms/step':>9} {'(min':>8} {'max)':>8} | {'vs ddim':>12} | windows overlap the ddim loop's"]
    for atoms, residues in SHAPES:
        loops = []
        for name, spec in variants:
            batch = batch_to(synthetic_batch([(atoms, residues)], seed=0), dev)
            loop = ReverseDiffusion(model, batch, [NoiseSource(0, 0)], solver=spec)
            for _ in range(2):                  # eager step, capture
                loop.step()
            loops.append((name, loop))
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in loops}
        for _ in range(a.reps):
            for name, loop in loops:
                loop.reset()
                loop.step()                     # a window starts where the first replayed step does: at steps_done = 1
                loop.step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loop.step()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
        base = ms[loops[0][0]]
        for i, (name, loop) in enumerate(loops):
            assert loop.finite(), name
            med = float(np.median(ms[name]))
            overlap = "-" if i == 0 else ("yes" if min(ms[name]) <= max(base) and min(base) <= max(ms[name]) else "NO")
            lines.append(f"{atoms + residues:5d} {name:<30} | {med:9.4f} {min(ms[name]):8.4f} {max(ms[name]):8.4f} | "
                         f"{med - float(np.median(base)):+9.4f} ms | {overlap}")
        del loops
    res = build.resource_usage(sources=build.SIDE_LIBS["multistep"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
