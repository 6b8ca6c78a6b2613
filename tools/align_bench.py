"""Times the alignment of generated samples at L = 320 (protein_redesign_amd.align) with HIP events -- ``superimpose`` of 64 samples
against one reference and ``pairwise_tm`` of the 64 samples -- and the float64 numpy yardstick tests/align_ref.py on the same
inputs with 16 processes.  Not gated by any test.

    python tools/align_bench.py [--out profiles/align_bench.txt] [--samples 64] [--length 320]

Warm-up calls come first; every timed figure is the median over ``--iters`` calls, each bracketed by device events (the
first-to-last spread is printed beside it).  The CPU figure for the pairwise matrix is EXTRAPOLATED from the pairs (0, r) -- it says so."""
import argparse
import multiprocessing as mp
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


def inputs(S, L, seed=0):
    """S noisy, partly diverging variants of one fold and a reference, float32 [S,L,3] / [L,3]; every fourth variant mirrored"""
    rng = np.random.default_rng(seed)
    base = AR.chain(rng, L)
    xs = []
    for k in range(S):
        v = base @ AR.MIRROR if k % 4 == 3 else base.copy()
        v = rng.uniform(-8.0, 8.0, 3) + v @ AR.random_rotation(rng) + rng.uniform(0.3, 2.0) * rng.normal(size=(L, 3))
        cut = int(rng.integers(L // 2, L))
        v[cut:] = (AR.chain(rng, L) + rng.uniform(-8.0, 8.0, 3))[cut:]
        xs.append(v)
    return np.stack(xs).astype(np.float32), base.astype(np.float32)


def _one(args):
    x, y = args
    return AR.superimpose(x, y, mirror=True)["tm"]


def device_time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.txt"))
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--length", type=int, default=320)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu-procs", type=int, default=16)
    a = ap.parse_args()
    S, L = a.samples, a.length
    xs, ref = inputs(S, L)
    # the yardstick first: its worker processes are gone before this process opens the GPU
    with mp.get_context("fork").Pool(a.cpu_procs) as pool:
        pool.map(_one, [(xs[0].astype(np.float64), ref.astype(np.float64))] * a.cpu_procs)         # start the workers
        t0 = time.perf_counter()
        cpu_tm = np.array(pool.map(_one, [(xs[k].astype(np.float64), ref.astype(np.float64)) for k in range(S)], chunksize=1))
        cpu_sup = time.perf_counter() - t0
        t0 = time.perf_counter()
        cpu_row = np.array(pool.map(_one, [(xs[0].astype(np.float64), xs[r].astype(np.float64)) for r in range(1, S)], chunksize=1))
        cpu_pairs = time.perf_counter() - t0
    if not torch.cuda.is_available():
        raise SystemExit("align_bench needs the GPU: a CPU run says nothing about the device path")
    from protein_redesign_amd import align, build
    x, y, m = torch.from_numpy(xs).cuda(), torch.from_numpy(ref).cuda(), torch.ones(L, device="cuda")
    sup = device_time(lambda: align.superimpose(x, y, m), a.iters, 3)
    pw = device_time(lambda: align.pairwise_tm(x, m), max(3, a.iters // 2), 2)
    rm = device_time(lambda: align.superimpose(x, y, m, mode="rmsd"), a.iters, 3)
    gpu_tm = align.superimpose(x, y, m).tm.cpu().numpy()
    gpu_pw = align.pairwise_tm(x, m).cpu().numpy()
    npairs = S * (S - 1) // 2
    seeds = len(AR.seeds(L))
    res = build.resource_usage(sources=build.SIDE_LIBS["align"].sources)
    lines = [
        f"align_bench: {S} samples, L = {L} masked positions (N = {L}), mirror on, {seeds} seeds per (pair, mirror)",
        f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; host {platform.processor() or platform.machine()}, {a.cpu_procs} processes for the yardstick",
        f"superimpose   {S} x 1 (TM mode)   : {sup[0]:9.3f} ms  (min {sup[1]:.3f}, max {sup[2]:.3f}; {a.iters} calls, HIP events)  3 launches per call, {S * 2} x G search workgroups",
        f"superimpose   {S} x 1 (RMSD mode) : {rm[0]:9.3f} ms  (min {rm[1]:.3f}, max {rm[2]:.3f})  3 launches per call",
        f"pairwise_tm   {S} x {S} ({npairs} pairs) : {pw[0]:9.3f} ms  (min {pw[1]:.3f}, max {pw[2]:.3f})  3 launches per call",
        f"align_ref     {S} x 1 on {a.cpu_procs} processes : {cpu_sup * 1e3:9.1f} ms",
        f"align_ref     {S - 1} pairs (0, r) on {a.cpu_procs} processes : {cpu_pairs * 1e3:9.1f} ms  -> EXTRAPOLATED to {npairs} pairs: {cpu_pairs * npairs / (S - 1):.1f} s",
        f"agreement: min over samples of tm(GPU) - tm(align_ref) = {float((gpu_tm - cpu_tm).min()):+.2e}, max {float((gpu_tm - cpu_tm).max()):+.2e}; "
        f"pairs (0, r): min {float((gpu_pw[0, 1:] - cpu_row).min()):+.2e}, max {float((gpu_pw[0, 1:] - cpu_row).max()):+.2e}",
        f"tm to the reference: mean {gpu_tm.mean():.4f}; diversity (mean pairwise tm) {(gpu_pw.sum() - np.trace(gpu_pw)) / (S * (S - 1)):.4f}",
        "resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):",
    ] + [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
