"""Times ``quality.lddt`` (protein_redesign_amd.quality: one fused sweep, integer counts) against the same quantity written with
``torch.cdist`` -- which materialises [S,N,N] matrices -- with HIP events, and records the peak device memory of both.  Not gated by
any test.

    python tools/quality_bench.py [--out profiles/quality_bench.txt] [--iters 20]

Shapes: S = 16 and 64 at N = 320 and 1024, S = 64 at N = 2048; all positions masked in, radius 15.  Warm-up calls come first; every timed
figure is the median over ``--iters`` calls, each bracketed by device events (min and max beside it).  Peak memory is
``torch.cuda.max_memory_allocated`` over one call, above what was allocated before it (the inputs).  The two must agree: the
largest difference of the per-structure score is printed (a pair on a threshold may fall either way between fp32 sweeps)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(16, 320), (64, 320), (16, 1024), (64, 1024), (64, 2048)]


def inputs(S, N, seed=0):
    """a folded-chain-like cloud (the density of quality_ref.walk, drawn directly: a walk of 2048 steps is slow and the timing does not
    care) and S noisy copies, fp32 on the device"""
    g = torch.Generator().manual_seed(seed)
    radius = 2.6 * N ** (1.0 / 3.0)
    v = torch.randn(N, 3, generator=g)
    y = radius * v / v.norm(dim=1, keepdim=True) * torch.rand(N, 1, generator=g) ** (1.0 / 3.0)
    sigma = torch.tensor([0.3, 1.0, 3.0])[torch.arange(S) % 3].view(S, 1, 1)
    x = y.unsqueeze(0) + sigma * torch.randn(S, N, 3, generator=g)
    return x.cuda(), y.cuda()


def lddt_cdist(x, y, mask, radius=15.0):
    """the per-structure lDDT of quality.lddt in plain torch"""
    D = torch.cdist(y, y)
    inc = (mask[:, None] > 0.5) & (mask[None, :] > 0.5) & (D < radius) & ~torch.eye(y.shape[0], dtype=torch.bool, device=y.device)
    diff = (torch.cdist(x, x) - D).abs()
    preserved = sum(((diff < t) & inc).sum((1, 2)) for t in (0.5, 1.0, 2.0, 4.0))
    return preserved.double() / (4.0 * inc.sum().double())


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_bench.txt"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_bench needs the GPU: a CPU run says nothing about the device path")
    from protein_redesign_amd import build, quality
    lines = [f"quality_bench: quality.lddt (one launch of quality_lddt_kernel + the torch quotients) against torch.cdist; radius 15, all positions masked in",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {a.iters} calls after 3 warm-up calls, HIP events",
             f"{'S':>4} {'N':>5} | {'fused ms':>9} {'(min':>8} {'max)':>8} {'peak MiB':>9} | {'cdist ms':>9} {'(min':>8} {'max)':>8} {'peak MiB':>9} | {'cdist/fused':>11} {'max |score diff|':>17}"]
    for S, N in SHAPES:
        x, y = inputs(S, N)
        m = torch.ones(N, device="cuda")
        fused, plain = (lambda: quality.lddt(x, y, m).score), (lambda: lddt_cdist(x, y, m))
        tf, tp = device_time(fused, a.iters, 3), device_time(plain, a.iters, 3)
        mf, mp = peak_bytes(fused), peak_bytes(plain)
        diff = float((fused() - plain()).abs().max())
        lines.append(f"{S:4d} {N:5d} | {tf[0]:9.3f} {tf[1]:8.3f} {tf[2]:8.3f} {mf / 2 ** 20:9.2f} | {tp[0]:9.3f} {tp[1]:8.3f} {tp[2]:8.3f} {mp / 2 ** 20:9.2f} | "
                     f"{tp[0] / tf[0]:11.2f} {diff:17.2e}")
    res = build.resource_usage(sources=build.SIDE_LIBS["quality"].sources)
    lines.append("resources (hipcc -Rpass-analysis=kernel-resource-usage, committed flags):")
    lines += [f"  {u['vgprs']:4d} VGPR {u['agprs']:3d} AGPR {u['scratch']:5d} B scratch  occ {u['occupancy']}  LDS {u['lds']:6d}  {name}" for name, u in sorted(res.items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
