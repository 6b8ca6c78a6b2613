"""Inputs, float64 references and error measures of the cases of tests/gemm_cases.py (a helper module, imported by
tests/test_gemm_dispatch_cpu.py -- which evaluates the references alone, on the CPU -- and tests/test_gemm_edges.py; not a conftest).

inputs(case)              the operands as float32 CPU tensors, from the case's own seed (a CRC of its id): A rows 1.5 randn + 0.7, weights
                          randn / sqrt(K); under a_ln every third row has |mean| several times its spread (the inputs of test_hip_parity.py)
reference(case, inp, dev) {output name: float64 tensor on ``dev``}: the operation in float64 with the epilogue restated in the header's order
measure(got, want)        whole-tensor rel-L2, the worst row and the worst column (||got - want|| / ||want|| per row / per column, against a
                          floor of 1e-3 of the mean norm as worst_row of test_model_widths.py); rows where N >= 16, columns where M >= 16,
                          a smaller output as max |error| over the rms of the reference
floors(want)              what the CPU test asserts so that the GPU test exempts nothing: no measured row or column lies under that floor
"""
import math
import zlib

import torch

import gemm_cases as T

FILL = -1.5                     # PrdGemm.fill of the colmask cases
FLOOR = 1e-3                    # a row / column norm is measured against at least FLOOR x the mean row / column norm
MIN_LEN = 16                    # rows are measured where N >= MIN_LEN, columns where M >= MIN_LEN

# whole-tensor bars of the suite (test_hip_parity.py); the worst row and the worst column get twice the bar (test_model_widths.py: ROW_TOL)
BAR_PLAIN, BAR_A_LN, BAR_A_SOFTMAX, BAR_LN, BAR_OUT_LN = 2e-6, 5e-6, 3e-6, 2e-6, 3e-6


def bar(c, name):
    if c.entry == "fc1_folded":
        return BAR_A_LN if name == "h" else BAR_PLAIN
    if name == "ln_out" or c.entry == "ln_rows":
        return BAR_LN
    if name == "out_ln":
        return BAR_OUT_LN
    return BAR_A_LN if c.a_ln == 1 else BAR_A_SOFTMAX if c.a_ln == 2 else BAR_PLAIN


def family(c):
    k = c.kernels[0]
    for prefix, name in (("gemm_kernel", "tile"), ("gemm_skinny", "skinny"), ("gemm_h2", "h2"), ("gemm_slab_kernel<0>", "slab"), ("gemm_slab_kernel<1>", "fc1_folded"),
                         ("ln_rows", "ln_rows"), ("softmax", "softmax_rows")):
        if k.startswith(prefix):
            return name
    return "ring[K][N]" if k == T.RING_BKN else "ring"


def seed(c):
    return zlib.crc32(c.id.encode())


def ln64(x):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)


def ln_rows_input(g, rows, K):
    x = torch.randn(rows, K, generator=g) * 2.0
    x[::3] = x[::3] * 0.25 + 4.0                       # |mean| several times the spread
    return x


def inputs(c):
    g = torch.Generator().manual_seed(seed(c))
    o, e = c.opts or {}, c.epi
    if c.entry == "ln_rows":
        inp = dict(x=torch.randn(c.M, c.N, generator=g) * 3 + 1)
        if o.get("gamma"):
            inp.update(gamma=torch.randn(c.N, generator=g), beta=torch.randn(c.N, generator=g))
        return inp
    if c.entry == "softmax_rows":
        x = torch.randn(c.M, c.N, generator=g) * 4
        if o.get("gap"):
            x[c.M // 2, c.N // 3] += o["gap"]
        return dict(x=x)
    if c.entry == "fc1_folded":
        S, Hd, HC = c.K, c.N, 64
        return dict(single=ln_rows_input(g, c.M, S), og=torch.randn(c.M, HC, generator=g), wo=torch.randn(S, HC, generator=g) / math.sqrt(HC),
                    bo=torch.randn(S, generator=g) * 0.1, w1=torch.randn(Hd, S, generator=g) / math.sqrt(S), b1=torch.randn(Hd, generator=g) * 0.5)
    G, M, N, K = c.G1 * c.G2, c.M, c.N, c.K
    if c.a_ln == 1:
        A = ln_rows_input(g, G * M, K).view(G, M, K)
    elif c.a_ln == 2:
        A = torch.randn(G, M, K, generator=g) * 3       # logits
    else:
        A = torch.randn(G, M, K, generator=g) * 1.5 + 0.7
    if "a_scale" in e and c.a_ln != 2:                  # (under a_ln = 2 the operand is the softmax of A: probabilities already)
        A = A * 1e-3                                    # far below 1: the lo part of the split needs the scale
    if "a_amax" in e:
        A = A * 1e-4
    B = torch.randn(*((G, K, N) if c.b_kn else (G, N, K)), generator=g) / math.sqrt(K)
    inp = dict(A=A, B=B)
    if "bias" in e:
        inp["bias"] = torch.randn(N, generator=g) * 0.5
    if "colscale" in e:
        inp["colscale"] = torch.rand(N, generator=g) + 0.5
    if "addmat" in e:
        inp["addmat"] = torch.randn(G, M, N, generator=g)
    if "colmask" in e:
        inp["colmask"] = (torch.rand(c.G1, N, generator=g) < 0.7).float()
    if "rowmask" in e:
        inp["rowmask"] = (torch.rand(c.G1, M, generator=g) < 0.8).float()
    if "mulmat" in e:
        inp["mulmat"] = torch.randn(G, M, N, generator=g) if "mul_pos" in e else torch.rand(G, M, N, generator=g) + 0.5
    if "resid" in e:
        inp["resid"] = torch.randn(G, M, N, generator=g)
    if "rscale" in e:
        inp["rscale"] = torch.rand(N, generator=g) + 0.5
    return inp


def alpha(c):
    return 0.5 if "alpha" in c.epi else 1.0


def reference(c, inp, dev="cpu"):
    """{name: float64 tensor}.  gemm: "C" [G, M, N] (or [M, n_split] with "C2" [M, N - n_split]), "ln_out" [M, K], "out_ln" [M, N]"""
    d = {k: v.to(dev).double() for k, v in inp.items()}
    if c.entry == "ln_rows":
        y = ln64(d["x"])
        return dict(y=y * d["gamma"] + d["beta"] if "gamma" in d else y)
    if c.entry == "softmax_rows":
        return dict(x=torch.softmax(d["x"], -1))
    if c.entry == "fc1_folded":
        s1 = d["single"] + d["og"] @ d["wo"].t() + d["bo"]
        return dict(single_out=s1, h=torch.relu(ln64(s1) @ d["w1"].t() + d["b1"]))
    e, N, M = c.epi, c.N, c.M
    A = ln64(d["A"]) if c.a_ln == 1 else torch.softmax(d["A"], -1) if c.a_ln == 2 else d["A"]
    v = torch.matmul(A, d["B"] if c.b_kn else d["B"].transpose(1, 2))                   # [G, M, N]
    cols = torch.arange(N, device=v.device)
    v = v * alpha(c)
    if "colscale" in e:
        v = v * d["colscale"]
    if "bias" in e:
        v = v + d["bias"]
    if "addmat" in e:
        v = v + d["addmat"]
    if "colmask" in e:
        cm = d["colmask"].repeat_interleave(c.G2, 0)[:, None, :]                        # [G, 1, N]: the mask of batch g1
        v = torch.where(cm < 0.5, torch.full_like(v, FILL), v)
    if "act1" in e or "act2" in e:
        a = torch.relu(v) if "act1" in e else torch.sigmoid(v)
        v = torch.where(cols >= T.act_from(c), a, v)
    if "rowmask" in e:
        rm = d["rowmask"].repeat_interleave(c.G2, 0)[:, :, None]                        # [G, M, 1]
        rc = T.rowmask_cols(c)
        v = torch.where(cols < rc, v * rm, v) if rc > 0 else v * rm
    if "mulmat" in e:
        v = torch.where(d["mulmat"] > 0, v, torch.zeros_like(v)) if "mul_pos" in e else v * d["mulmat"]
    if "resid" in e:
        v = v + (d["resid"] * d["rscale"] if "rscale" in e else d["resid"])
    out = {}
    if "c2" in e:
        ns = T.n_split(c)
        out["C"], out["C2"] = v[0][:, :ns], v[0][:, ns:]
    else:
        out["C"] = v
    if "ln_out" in e:
        out["ln_out"] = A[0]
    if "out_ln" in e:
        out["out_ln"] = ln64(v[0])
    return out


def _norms(x, dim):
    n = x.norm(dim=dim)
    return n, n.clamp_min(FLOOR * float(n.mean()))


def measure(got, want):
    """{"rel": whole-tensor rel-L2, "row": worst row, "col": worst column, "small": max |error| / rms} -- row where the rows have at least
    MIN_LEN elements, col where the columns have, small where either has not.  ``want``: [..., rows, columns] float64."""
    err = got.to(want.device).double() - want
    out = dict(rel=float(err.norm() / want.norm().clamp_min(1e-30)))
    R, Cn = want.shape[-2], want.shape[-1]
    if Cn >= MIN_LEN:
        out["row"] = float((err.norm(dim=-1) / _norms(want, -1)[1]).max())
    if R >= MIN_LEN:
        out["col"] = float((err.norm(dim=-2) / _norms(want, -2)[1]).max())
    if Cn < MIN_LEN or R < MIN_LEN:
        out["small"] = float(err.abs().max() / want.pow(2).mean().sqrt().clamp_min(1e-30))
    return out


def floors(want):
    """[what lies under the floor of its measure] -- empty when the GPU test may measure every row, every column and the tensor"""
    bad = []
    R, Cn = want.shape[-2], want.shape[-1]
    if not float(want.norm()) > 0 or not bool(torch.isfinite(want).all()):
        bad.append("tensor")
    if Cn >= MIN_LEN:
        n, fl = _norms(want, -1)
        if bool((n < fl).any()):
            bad.append(f"{int((n < fl).sum())} rows")
    if R >= MIN_LEN:
        n, fl = _norms(want, -2)
        if bool((n < fl).any()):
            bad.append(f"{int((n < fl).sum())} columns")
    return bad
