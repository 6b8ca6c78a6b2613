"""Times the structural alignment of generated samples (protein_redesign_amd.tmalign) with HIP events: 64 samples of L = 320 against
one reference of 300 residues, and the float64 numpy yardstick tests/tmalign_ref.py on ONE CPU core on the first ``--cpu-samples`` of
the same inputs for scale.  Not gated by any test.

    python tools/tmalign_bench.py [--out profiles/tmalign_bench.txt] [--samples 64] [--length 320] [--ref-length 300]

Warm-up calls come first; the timed figure is the median over ``--iters`` calls, each bracketed by device events."""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import align_ref as AR  # noqa: E402
import tmalign_ref as TR  # noqa: E402
from align_bench import device_time  # noqa: E402


def inputs(S, L, Lr, seed=0):
    """a reference of Lr residues and S noisy variants of length L of the fold it was cut from (an N-terminal and an internal deletion
    make up L - Lr); every fourth variant mirrored; float32"""
    rng = np.random.default_rng(seed)
    base = TR.ss_chain(rng, L)
    a = (L - Lr) // 2
    keep = np.r_[a:L // 2, L // 2 + (L - Lr - a):L]
    ref = base[keep]
    xs = []
    for k in range(S):
        v = base @ AR.MIRROR if k % 4 == 3 else base.copy()
        xs.append(rng.uniform(-8.0, 8.0, 3) + v @ AR.random_rotation(rng) + rng.uniform(0.3, 2.0) * rng.normal(size=(L, 3)))
    return np.stack(xs).astype(np.float32), ref.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tmalign_bench.txt"))
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--length", type=int, default=320)
    ap.add_argument("--ref-length", type=int, default=300)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu-samples", type=int, default=4)
    a = ap.parse_args()
    S, L, Lr = a.samples, a.length, a.ref_length
    xs, ref = inputs(S, L, Lr)
    t0 = time.perf_counter()
    cpu = [TR.align(xs[k], ref)["tm"] for k in range(min(S, a.cpu_samples))]
    cpu_s = (time.perf_counter() - t0) / len(cpu)
    if not torch.cuda.is_available():
        raise SystemExit("tmalign_bench needs the GPU: a CPU run says nothing about the device path")
    from protein_redesign_amd import build, tmalign
    x, y = torch.from_numpy(xs).cuda(), torch.from_numpy(ref).cuda()
    mx, my = torch.ones(L, device="cuda"), torch.ones(Lr, device="cuda")
    t = device_time(lambda: tmalign.align(x, y, mx, my), a.iters, 3)
    out = tmalign.align(x, y, mx, my)
    gpu_tm = out.tm.cpu().numpy()
    res = build.resource_usage(sources=build.SIDE_LIBS["tmalign"].sources)
    lines = [
        f"tmalign_bench: {S} samples of L = {L} against one reference of {Lr} residues, mirror on: {S * 2 * 3} refine workgroups",
        f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; host {platform.processor() or platform.machine()}",
        f"tmalign.align {S} x 1 : {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}; {a.iters} calls, HIP events)  4 launches per call",
        f"tmalign_ref   per pair on one CPU core : {cpu_s * 1e3:9.1f} ms (mean of {len(cpu)})  -> {cpu_s * S:.1f} s for {S} samples, EXTRAPOLATED",
        f"agreement on the first {len(cpu)} samples: tm(GPU) - tm(tmalign_ref) min {float((gpu_tm[:len(cpu)] - cpu).min()):+.2e}, max {float((gpu_tm[:len(cpu)] - cpu).max()):+.2e}",
        f"tm to the reference: mean {gpu_tm.mean():.4f}; aligned pairs: mean {float(out.n_aligned.float().mean()):.1f}; mirrored: {int(out.mirrored.sum())} of {S}",
        "resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):",
    ] + [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
