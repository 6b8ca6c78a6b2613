"""Times the reverse-diffusion loop under a solver against the loop without one, at the shapes and model of bench.py.  Not gated by any
test.

    python tools/solver_bench.py [--out profiles/solver_bench.txt] [--reps 7] [--steps 48] [--samples 3]

Shapes: 64 atoms + 256 residues (N = 320, bench.py's default) and 64 + 705 (N = 769), one sample, T = 1000, K = 50.

1. ms per replayed step: the default loop (prd_step_boundary), ``Solver.ddim(50)`` and ``Solver.ancestral(50)`` (prd_solver_boundary;
   one boundary launch per step in all three).  The three loops live in ONE process and are timed in alternation -- a window of
   ``--steps`` replayed steps of each, ``--reps`` times round-robin -- so that drift of the box falls on all three alike; a window is a
   host clock around work that ends in a device synchronise, after the eager step and the graph capture of every loop (a solver
   loop is reset before a window: it has only K - 2 replayed steps).  The figure is the median window, with the smallest and largest
   beside it; whether the windows of a solver loop overlap those of the default loop is stated per line.
2. Seconds per sample, set-up included (prepare_batch, the draws, the uploads, the static embeddings, the eager step, the capture):
   ``model.sample`` with ``Solver.ddim(50)`` and with ``Solver.ancestral(50)`` against ``model.sample`` over all 1000 levels, host
   clock to a device synchronise, median of ``--samples`` calls after one warm-up call of each."""
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
K = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=K - 2)
    ap.add_argument("--samples", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("solver_bench needs the GPU: a CPU run says nothing about the device path")
    if not 1 <= a.steps <= K - 2:
        raise SystemExit(f"--steps must lie in [1, {K - 2}]: a K = {K} loop replays K - 2 steps after its eager step and its capture")
    import bench
    from protein_redesign_amd import build
    from protein_redesign_amd.diffusion_model import ReverseDiffusion
    from protein_redesign_amd.solver import Solver
    from protein_redesign_amd.synthetic import NoiseSource, batch_to, synthetic_batch
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_model(dev)
    variants = [("default loop (T = 1000)", None), (f"Solver.ddim({K})", Solver.ddim(K)), (f"Solver.ancestral({K})", Solver.ancestral(K))]
    lines = [f"solver_bench: model of bench.py (S {bench.S}, P {bench.P}, {bench.NB} blocks, T {bench.T}), one sample, mask_prob 0.3",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"1. ms per replayed step: median of {a.reps} alternating windows of {a.steps} steps (host clock to a device synchronise), after "
             "the eager step and the capture",
             f"{'N':>5} {'loop':<26} | {'ms/step':>9} {'(min':>8} {'max)':>8} | {'vs default':>12} | windows overlap the default loop's"]
    for atoms, residues in SHAPES:
        loops = []
        for name, spec in variants:
            batch = batch_to(synthetic_batch([(atoms, residues)], seed=0), dev)
            loop = ReverseDiffusion(model, batch, [NoiseSource(0, 0)], **({} if spec is None else {"solver": spec}))
            for _ in range(2):                  # eager step, capture
                loop.step()
            loops.append((name, loop))
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in loops}
        for _ in range(a.reps):
            for name, loop in loops:
                if loop.solver is not None or loop.steps_done + a.steps > loop.K:
                    loop.reset()
                    if loop.solver is not None:
                        loop.step()             # a window of a solver loop starts where its first replayed step does: at steps_done = 1
                        loop.step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loop.step()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
        base = ms[loops[0][0]]
        for name, loop in loops:
            assert loop.finite(), name
            med = float(np.median(ms[name]))
            overlap = "-" if loop.solver is None else ("yes" if min(ms[name]) <= max(base) and min(base) <= max(ms[name]) else "NO")
            lines.append(f"{atoms + residues:5d} {name:<26} | {med:9.4f} {min(ms[name]):8.4f} {max(ms[name]):8.4f} | "
                         f"{med - float(np.median(base)):+9.4f} ms | {overlap}")
        del loops
    lines += [f"2. seconds per sample, set-up included: median of {a.samples} calls of model.sample (host clock to a device synchronise), "
              "after one warm-up call",
              f"{'N':>5} {'loop':<26} | {'s/sample':>9} {'(min':>8} {'max)':>8} | {'speed-up':>9}"]
    for atoms, residues in SHAPES:
        base = None
        for name, spec in variants:
            sec = []
            for call in range(a.samples + 1):
                batch = batch_to(synthetic_batch([(atoms, residues)], seed=0), dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.sample(batch, sources=[NoiseSource(0, call)], **({} if spec is None else {"solver": spec}))
                torch.cuda.synchronize()
                if call:
                    sec.append(time.perf_counter() - t0)
            med = float(np.median(sec))
            base = med if base is None else base
            lines.append(f"{atoms + residues:5d} {name:<26} | {med:9.4f} {min(sec):8.4f} {max(sec):8.4f} | {base / med:8.1f}x")
    res = build.resource_usage(sources=build.SIDE_LIBS["solver"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
