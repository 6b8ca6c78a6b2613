"""Times one replayed step of the reverse-diffusion loop without guidance (73 launches) and with ``Guidance`` (74: prd_guide_eps between
the network and the boundary), at the shape and model of bench.py.  Not gated by any test.

    python tools/guidance_bench.py [--out profiles/guidance_bench.txt] [--reps 7] [--steps 200]
    rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/guidance_bench.py --trace [--steps 50]      # then --kernels DB

Shapes: 64 atoms + 256 residues (N = 320, bench.py's default) and 64 + 705 (N = 769), one sample.  The three loops -- unguided, guided,
and a second unguided one with buffers of its own as the control -- live in ONE process and are timed in alternation: a window of
``--steps`` replayed steps of each, ``--reps`` times round-robin, so that drift of the box falls on all of them alike; a window is a
host clock around work that ends in a device synchronise, after the eager step, the graph capture and 10 warm-up steps of every loop.
The figure is the median window in ms/step, with the smallest and largest beside it; the control's distance from the first loop says
what two loops of one process differ by for no reason at all.  The guidance is the clash term with its default floors, the chain
restraints of ``guidance.chain`` and the bond restraints of ``guidance.bonds``, guided at every level.

``--trace``: the unguided and the guided loop at N = 320, three alternating rounds of ``--steps`` steps each, nothing timed: the run
rocprofv3 traces.  ``--kernels DB``: the per-launch durations of step_boundary_kernel and guide_eps_kernel from that run's database,
appended to ``--out``."""
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
VARIANTS = [("no guidance", False), ("Guidance(clash, chain, bonds)", True), ("no guidance, a second loop (control)", False)]


def spec_for(batch):
    from protein_redesign_amd import guidance as GD
    return GD.Guidance(restraints=GD.chain(batch) + GD.bonds(batch), clash=True, scale=1.0, cap=0.5)


def kernels(db_path, out):
    """per-launch durations (us) of the two kernels from a rocprofv3 --kernel-trace database"""
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = list(db.execute("select name, end - start from kernels"))
    lines = ["kernels per launch (rocprofv3 --kernel-trace --stats, a run of its own: the unguided and the guided loop at N = 320, three "
             "alternating rounds)"]
    for key in ("step_boundary_kernel", "guide_eps_kernel"):
        us = np.array([d for n, d in rows if key in n], dtype=np.float64) / 1e3
        if us.size:
            lines.append(f"  {key:<22}: {us.size} launches, us: median {np.median(us):.2f} mean {us.mean():.2f} min {us.min():.2f} "
                         f"p10 {np.percentile(us, 10):.2f} p90 {np.percentile(us, 90):.2f} max {us.max():.2f} std {us.std():.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "a") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernels", default=None, metavar="DB")
    a = ap.parse_args()
    if a.kernels:
        return kernels(a.kernels, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("guidance_bench needs the GPU: a CPU run says nothing about the device path")
    import bench
    from protein_redesign_amd import build
    from protein_redesign_amd.diffusion_model import ReverseDiffusion
    from protein_redesign_amd.synthetic import NoiseSource, batch_to, synthetic_batch
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_model(dev)

    def loops_for(atoms, residues, variants):
        loops = []
        for name, guided in variants:
            host = synthetic_batch([(atoms, residues)], seed=0)
            kw = dict(guidance=spec_for(host)) if guided else {}
            loop = ReverseDiffusion(model, batch_to(host, dev), [NoiseSource(0, 0)], **kw)
            for _ in range(12):                 # eager step, capture, warm-up
                loop.step()
            loops.append((name, loop))
        torch.cuda.synchronize()
        return loops

    if a.trace:
        loops = loops_for(*SHAPES[0], VARIANTS[:2])
        for _ in range(3):
            for _, loop in loops:
                for _ in range(a.steps):
                    loop.step()
        torch.cuda.synchronize()
        return
    lines = [f"guidance_bench: ms per replayed step, model of bench.py (S {bench.S}, P {bench.P}, {bench.NB} blocks, T {bench.T}), one sample, "
             f"mask_prob 0.3; guidance: clash floors 3.0 / 2.5 / 2.0 A, chain and bond restraints, every level",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {a.reps} alternating windows of {a.steps} steps "
             f"(host clock to a device synchronise), after capture and 10 warm-up steps",
             f"{'N':>5} {'loop':<40} | {'ms/step':>9} {'(min':>8} {'max)':>8} | {'vs no guidance':>17}"]
    for atoms, residues in SHAPES:
        loops = loops_for(atoms, residues, VARIANTS)
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
            lines.append(f"{atoms + residues:5d} {name:<40} | {med:9.4f} {min(ms[name]):8.4f} {max(ms[name]):8.4f} | {med - base:+13.4f} ms")
        guided = loops[1][1]
        lines.append(f"      ({len(guided.guidance.restraints)} restraints; clash / restraint energy at the last estimate: "
                     + " / ".join(f"{v:.3f}" for v in guided.guidance_energy.double().sum(dim=(0, 1)).tolist()) + ")")
        del loops
    res = build.resource_usage(sources=build.SIDE_LIBS["guide"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
