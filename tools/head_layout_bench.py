"""Timing of the general-layout triangle-attention core (csrc/prd_tri_heads.hip) on one GPU:

    python tools/head_layout_bench.py [--out profiles/head_layouts.txt]

  * the core + output projection against torch_ref.triangle_attention (the differentiable torch restatement: the "slow but correct"
    floor) for (H, c) in {(8, 32), (4, 16)}, N in {320, 769}, b = 1, P = 64;
  * the general core at 4 x 16 against the tuned core (ops.tri_attn_core) at the same shapes;
  * steps/s of sample_step and of one replayed sample() step at the BASELINE configs[1] shape (256 residues + 64 ligand atoms,
    single_dim 512, pair_dim 64, 4 blocks) with --num_heads 8 --head_dim 32.
Median of CUDA-event timings after warm-up.

    python tools/head_layout_bench.py --backward [--out profiles/head_layouts_backward.txt]

  * forward + backward of training.tri_attn_update (TriAttnFn: the general backward core, prd_tri_attn_bwd_core_heads) against the
    HipOp recompute through torch_ref.triangle_attention that it replaced (kept callable here, not in the package), per (N, layout),
    the two arms alternating in one process: time and torch.cuda.max_memory_allocated above the inputs.  4 x 16 at N = 769 is the
    former "> 416" fallback; 4 x 16 at N = 320 runs the tuned backward cores and is timed against the general core as well."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from protein_redesign_amd import _lib, ops, torch_ref, training  # noqa: E402
from protein_redesign_amd.constants import make_args  # noqa: E402
from protein_redesign_amd.diffusion_model import ProteinReDiffModel, ReverseDiffusion  # noqa: E402
from protein_redesign_amd.synthetic import NoiseSource, batch_to, deterministic_state_dict, synthetic_batch  # noqa: E402
from protein_redesign_amd.weights import spec_tensors  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)          # us


def ops_table(lines):
    P = 64
    for N in (320, 769):
        for H, c in ((8, 32), (4, 16)):
            g = torch.Generator(device="cuda").manual_seed(N)
            pair = torch.randn(1, N, N, P, device="cuda", generator=g)
            mask = torch.ones(1, N, device="cuda")
            HC = H * c
            w = [torch.randn(HC, P, device="cuda", generator=g) / 8 for _ in range(4)] + [torch.randn(HC, device="cuda", generator=g)]
            wo, bo = torch.randn(P, HC, device="cuda", generator=g) / HC ** 0.5, torch.randn(P, device="cuda", generator=g)
            ws = torch.empty(ops.tri_attn_heads_ws_floats(1, N, P, H, c), device="cuda")
            out = torch.empty_like(pair)
            core = timed(lambda: ops.tri_attn_core_heads(pair, mask, w, H, c, ending=False, ws=ws), 10)
            full = timed(lambda: ops.linear(ops.tri_attn_core_heads(pair, mask, w, H, c, ending=False, ws=ws), wo, bo, out=out), 10)
            with torch.no_grad():
                ref = timed(lambda: torch_ref.triangle_attention(pair, mask, *w, wo, bo, H, c, ending=False), 3, warmup=1)
            line = (f"N={N:4d} H={H} c={c:2d} P={P}: general core {core:9.1f} us, core + out-proj {full:9.1f} us, "
                    f"torch_ref.triangle_attention {ref:9.1f} us ({ref / full:.1f}x)")
            if (H, c) == (4, 16):
                og = torch.empty(1, N, N, 64, device="cuda")
                tuned = timed(lambda: ops.tri_attn_core(pair, mask, w, H, c, ending=False, og=og), 10)
                line += f"; tuned core {tuned:8.1f} us (general / tuned {core / tuned:.2f})"
            lines.append(line)
            print(line, flush=True)


def recompute_update(pair, mask, wts, H, c):
    """What training.tri_attn_update did for these shapes before the general backward core: HIP forward, torch_ref under autograd."""
    def ref(p, *w):
        return torch_ref.triangle_attention(p, mask, *w, H, c, ending=False)

    def hip(p, *w):
        return ops.tri_attn(p.contiguous(), mask, w, H, c, ending=False, residual=False)
    return training.HipOp.apply(hip, ref, pair, *wts)


def backward_table(lines):
    from types import SimpleNamespace
    P = 64
    for N in (320, 769):
        for H, c in ((8, 32), (4, 16)):
            g = torch.Generator(device="cuda").manual_seed(N)
            HC = H * c
            pair = torch.randn(1, N, N, P, device="cuda", generator=g).requires_grad_(True)
            mask = torch.ones(1, N, device="cuda")
            wts = [torch.randn(HC, P, device="cuda", generator=g) / 8 for _ in range(4)] + [torch.randn(HC, device="cuda", generator=g)]
            wts += [torch.randn(P, HC, device="cuda", generator=g) / HC ** 0.5, torch.randn(P, device="cuda", generator=g)]
            wts = [w.requires_grad_(True) for w in wts]
            dy = torch.randn(1, N, N, P, device="cuda", generator=g)
            ta = SimpleNamespace(attn=SimpleNamespace(num_heads=H, head_dim=c, weights=lambda: wts), mode="starting")

            def new():
                return torch.autograd.grad(training.tri_attn_update(ta, pair, mask), [pair, *wts], dy)

            def old():
                return torch.autograd.grad(recompute_update(pair, mask, wts, H, c), [pair, *wts], dy)

            def general():                  # 4 x 16 at N <= 416: the general core where the tuned cores are the dispatch (the limit is read
                                            # by forward and backward alike: the forward keeps no statistics, the core finds them)
                prev, ops.TRI_ATTN_BWD_TUNED_MAX_N = ops.TRI_ATTN_BWD_TUNED_MAX_N, 0
                try:
                    return new()
                finally:
                    ops.TRI_ATTN_BWD_TUNED_MAX_N = prev
            arms = [("hand-written", new), ("HipOp recompute", old)]
            if (H, c) == (4, 16) and N <= training.TRI_ATTN_BWD_MAX_N:
                arms = [("tuned cores", new), ("HipOp recompute", old), ("general core", general)]
            res = {name: [] for name, _ in arms}
            peak = {}
            for rnd in range(4):            # round 0 warms up; the arms alternate
                for name, fn in arms:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    out = fn()
                    e.record()
                    e.synchronize()
                    del out
                    peak[name] = torch.cuda.max_memory_allocated() - before
                    if rnd:
                        res[name].append(a.elapsed_time(e) * 1e3)
            line = f"N={N:4d} H={H} c={c:2d} P={P} forward + backward: " + "; ".join(
                f"{name} {statistics.median(res[name]):9.1f} us, peak {peak[name] / 1e9:6.3f} GB" for name, _ in arms)
            lines.append(line)
            print(line, flush=True)


def step_table(lines):
    args = make_args(single_dim=512, pair_dim=64, num_blocks=4, head_dim=32, num_heads=8, num_steps=1000)
    model = ProteinReDiffModel(args)
    model.load_state_dict(deterministic_state_dict(spec_tensors(args), seed=1))
    model = model.to("cuda").eval()
    batch = batch_to(synthetic_batch([(64, 256)], esm_dim=args["esm_dim"], seed=0), "cuda")
    with torch.inference_mode():
        loop = ReverseDiffusion(model, batch, [NoiseSource(0, 0)])
        loop.step()                        # eager
        loop.step()                        # capture + replay
        us = timed(loop.step, 20, warmup=2)
        d = loop.batch
        eager = timed(lambda: model.sample_step(d, loop.z, loop.seq_t, loop.mask, loop.t), 10)
    line = (f"configs[1] shape (N = 320, S = 512, P = 64, 4 blocks), num_heads 8 x head_dim 32, arith {_lib.arith()}: "
            f"replayed step {us:.1f} us = {1e6 / us:.1f} steps/s; eager sample_step {eager:.1f} us")
    lines.append(line)
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--backward", action="store_true", help="the training backward against the HipOp recompute it replaced")
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}"]
    if a.backward:
        backward_table(lines)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if not a.steps_only:
        ops_table(lines)
    step_table(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
