"""GPU: every case of tests/gemm_cases.py -- one per kernel instantiation of csrc/prd_gemm.hip, one on each side of every dispatch
threshold, ragged tiles, pitched and offset operands, every epilogue field off a tile edge -- against float64 on the device.

A case runs through ops.gemm (ops.layer_norm / prd_ln_rows, ops.softmax_rows_, prd_single_fc1_folded as ops.transition_single_folded calls
it) in the arithmetic it names, inside guarded("nan") (tests/guarded_alloc.py): every input sits in a guarded buffer of its own with NaN in
its padding, every output in a poisoned one.  Checked per case, in this order:
  1. the guard bands are intact;
  2. every element of C[:, :N], C2, ln_out, out_ln is written and finite;
  3. everything else of the output buffers -- the padding columns [N, ldc), the gaps between batches, the part of C beside C2 -- still
     holds the poison (prd_softmax_rows: the tail [n, ld) is zero, as its contract says);
  4. the whole-tensor rel-L2 against the bar of the suite: 2e-6 plain, 5e-6 with a_ln, 3e-6 with a_ln = 2, 2e-6 ln_out / LayerNorm,
     3e-6 out_ln;
  5. the worst row and the worst column (||got - want|| / ||want|| per row / column; rows where N >= 16, columns where M >= 16, a
     smaller output as max |error| / rms) against TWICE that bar.  tests/test_gemm_dispatch_cpu.py shows that no reference row or
     column lies under the floor of this measure, so nothing is exempt.
Every figure is printed (-s).  The largest per kernel family, arithmetic and kind of output, as measured on an MI355X (rel = whole
tensor, row / col = worst row / column, small = max |error| / rms of the outputs with fewer than 16 rows or columns); every one is
below its bar, so no bar was raised and torch's own fp32 matmul was not needed as a second yardstick:
  family        arith    output
  tile          fp32     plain   rel 1.26e-07  row 2.54e-07  col 2.42e-07  small 2.69e-07
  tile          split16  plain   rel 1.37e-07  row 1.62e-07  col 2.23e-07
  skinny        fp32     plain   rel 2.19e-07  row 2.75e-07  col 3.38e-07  small 2.12e-07
  skinny        fp32     a_ln    rel 2.80e-07  row 7.72e-07  col 1.00e-06
  skinny        fp32     ln_out  rel 2.55e-07  row 1.04e-06  col 3.24e-07
  skinny        split16  plain   rel 2.20e-07  row 3.15e-07  col 2.84e-07  small 6.70e-07
  skinny        split16  a_ln    rel 1.85e-07  row 7.88e-07  col 1.87e-06
  h2            split16  plain   rel 2.68e-07  row 3.00e-07  col 4.60e-07  small 1.50e-06
  h2            split16  a_ln    rel 2.93e-07  row 9.48e-07  col 1.42e-06
  h2            split16  ln_out  rel 2.15e-07  row 1.03e-06  col 3.72e-07
  ring          split16  plain   rel 1.56e-07  row 1.82e-07  col 2.37e-07  small 1.87e-07
  ring          split16  a_ln    rel 3.27e-07  row 1.17e-06  col 9.52e-07  small 4.70e-07
  ring          split16  ln_out  rel 4.19e-07  row 1.06e-06  col 5.07e-07  small 5.49e-07
  ring[K][N]    split16  plain   rel 1.60e-07  row 2.26e-07  col 2.09e-07  small 3.31e-07
  ring[K][N]    split16  a_ln=2  rel 1.41e-07  row 2.90e-07  col 2.33e-07
  slab          split16  plain   rel 1.74e-07  row 2.18e-07  col 2.23e-07
  slab          split16  a_ln    rel 7.16e-07  row 1.42e-06  col 2.75e-06
  slab          split16  ln_out  rel 1.97e-07  row 9.29e-07  col 2.39e-07
  slab          split16  out_ln  rel 1.59e-07  row 1.87e-07  col 2.02e-07
  fc1_folded    split16  plain   rel 3.98e-08  row 5.86e-08  col 5.22e-08      (single_out)
  fc1_folded    split16  a_ln    rel 3.75e-07  row 8.18e-07  col 2.96e-06      (h)
  ln_rows       fp32     plain   rel 1.00e-07  row 1.70e-07  col 7.33e-08  small 7.30e-07
  softmax_rows  fp32     plain   rel 1.22e-07  row 1.98e-07                small 2.12e-06
"""
import ctypes

import pytest
import torch

import gemm_cases as T
import gemm_ref as R
from guarded_alloc import guarded
from protein_redesign_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture
def arith(request):
    """the arithmetic the case names, set and restored as the gemm_mode fixtures do"""
    prev = _lib.lib().prd_get_gemm_mode()
    assert _lib.lib().prd_set_gemm_mode(1 if request.param == "split16" else 0) == 0
    yield request.param
    assert _lib.lib().prd_set_gemm_mode(prev) == 0


def pitched(t, ld, off=0, stride=None):
    """flat float32 CPU buffer [off + batches * stride] holding the [batches, rows, cols] tensor ``t`` with row pitch ``ld``; NaN elsewhere"""
    Gn, rows, cols = t.shape
    stride = rows * ld if stride is None else stride
    buf = torch.full((off + Gn * stride,), NAN)
    buf[off:].as_strided((Gn, rows, cols), (stride, ld, 1)).copy_(t)
    return buf


def region(buf, shape, ld, off=0, stride=0):
    """the [batches, rows, cols] view of the flat buffer ``buf``"""
    return buf[off:].as_strided(shape, (stride, ld, 1))


def poison_intact_outside(buf, views):
    """True when every element of the flat float32 buffer outside ``views`` still holds the 0xFF poison"""
    bits = buf.view(torch.int32) == -1
    written = torch.zeros_like(bits)
    for v in views:
        written.as_strided(v.shape, v.stride(), v.storage_offset() - buf.storage_offset()).fill_(True)
    return bool(bits[~written].all()), int((~bits[~written]).sum())


def run_gemm(c, g, inp):
    """{name: (got view, flat output buffer, [views a kernel may write])}"""
    G, M, N, K, e = c.G1 * c.G2, c.M, c.N, c.K, c.epi
    lda, ldb, ldc = T.dims(c)
    sA, sB, sC = M * lda + c.spad, (K if c.b_kn else N) * ldb + c.spad, M * ldc + c.spad
    A = g.put(pitched(inp["A"], lda, c.a_off, sA), DEV)
    B = g.put(pitched(inp["B"], ldb, c.b_off, sB), DEV)
    Cb = g.empty(c.c_off + G * sC, device=DEV)
    dev = lambda name: g.put(inp[name], DEV) if name in inp else None
    kw = {}
    if "addmat" in e:
        kw.update(addmat=g.put(pitched(inp["addmat"], N + 4), DEV), sad=(c.G2 * M * (N + 4), M * (N + 4)), ldadd=N + 4)
    if "colmask" in e:
        kw.update(colmask=dev("colmask"), scm1=N, fill=R.FILL)
    if "rowmask" in e:
        kw.update(rowmask=dev("rowmask"), srm1=M, rowmask_cols=T.rowmask_cols(c))
    if "mulmat" in e:
        kw.update(mulmat=g.put(pitched(inp["mulmat"], N + 8), DEV), smu=(c.G2 * M * (N + 8), M * (N + 8)), ldmul=N + 8, mul_pos="mul_pos" in e)
    if "resid" in e:
        kw.update(resid=g.put(pitched(inp["resid"], N + 4), DEV), sr=(c.G2 * M * (N + 4), M * (N + 4)), ldr=N + 4, rscale=dev("rscale"))
    ns = T.n_split(c)
    outs = {}
    if "c2" in e:
        kw.update(c2=g.empty(M, N - ns + 4, device=DEV), n_split=ns)
    if "ln_out" in e:
        kw.update(ln_out=g.empty(M, K + 4, device=DEV))
    if "out_ln" in e:
        kw.update(out_ln=g.empty(M, N + 4, device=DEV))
    if c.slab and c.a_ln and not (c.opts or {}).get("no_wsum"):
        kw.update(wsum=g.put(inp["B"][0].double().sum(1).float(), DEV))
    if "a_scale" in e:
        kw.update(a_scale=1024.0)
    if "a_amax" in e:
        kw.update(a_amax=g.put(inp["A"].abs().max().reshape(1).view(torch.int32), DEV))
    ops.gemm(A, B, Cb, M, N, K, lda, ldb, ldc, a_off=c.a_off, b_off=c.b_off, c_off=c.c_off, G1=c.G1, G2=c.G2, sa=(c.G2 * sA, sA), sb=(c.G2 * sB, sB),
             sc=(c.G2 * sC, sC), b_kn=bool(c.b_kn), alpha=R.alpha(c), bias=dev("bias"), colscale=dev("colscale"), act=1 if "act1" in e else 2 if "act2" in e else 0,
             act_from=T.act_from(c), tile_hint=c.tile_hint, a_ln=c.a_ln, slab=bool(c.slab), **kw)
    torch.cuda.synchronize()
    if "c2" in e:
        cv = region(Cb, (1, M, ns), ldc, c.c_off, sC)
        outs["C"] = (cv[0], Cb, [cv])
        outs["C2"] = (kw["c2"][:, :N - ns], kw["c2"].view(-1), [kw["c2"][:, :N - ns]])
    else:
        cv = region(Cb, (G, M, N), ldc, c.c_off, sC)
        outs["C"] = (cv, Cb, [cv])
    for name, cols in (("ln_out", K), ("out_ln", N)):
        if name in e:
            outs[name] = (kw[name][:, :cols], kw[name].view(-1), [kw[name][:, :cols]])
    return outs


def run_ln_rows(c, g, inp):
    rows, C, ldx, ldy = c.M, c.N, c.lda or c.N, c.ldc or c.N
    x = g.put(pitched(inp["x"][None], ldx, c.a_off), DEV)
    gamma, beta = (g.put(inp[k], DEV) if k in inp else None for k in ("gamma", "beta"))
    if ldx == C and ldy == C and c.a_off == 0:
        y = ops.layer_norm(x.view(rows, C), gamma, beta)           # (allocates its output through the guarded factories)
        torch.cuda.synchronize()
        return dict(y=(y, y.view(-1), [y]))
    y = g.empty(rows * ldy, device=DEV)
    _lib.check(_lib.lib().prd_ln_rows(_lib.dptr(x) + 4 * c.a_off, _lib.dptr(y), _lib.dptr(gamma), _lib.dptr(beta), rows, C, ldx, ldy, _lib.stream()), "prd_ln_rows")
    torch.cuda.synchronize()
    yv = region(y, (1, rows, C), ldy)[0]
    return dict(y=(yv, y, [yv]))


def run_softmax_rows(c, g, inp):
    rows, n, ld = c.M, c.N, c.ldc or c.N
    x = g.put(pitched(inp["x"][None], ld), DEV).view(rows, ld)
    ops.softmax_rows_(x, n)
    torch.cuda.synchronize()
    assert bool((x[:, n:] == 0).all()), "the tail [n, ld) is not zero"
    return dict(x=(x[:, :n], x.reshape(-1), [x]))


def run_fc1_folded(c, g, inp):
    M, S, Hd, HC = c.M, c.K, c.N, 64
    d = {k: v.to(DEV) for k, v in inp.items()}
    w1cat, woT, wsum1, w1bo = (g.put(t) for t in ops.pack_fc1_fold(d["wo"], d["bo"], d["w1"]))
    single, og, bo, b1 = (g.put(d[k]) for k in ("single", "og", "bo", "b1"))
    assert ops.fc1_fold_ok(M, S, HC, Hd)
    s1, h = g.empty(M, S, device=DEV), g.empty(M, Hd, device=DEV)
    wsb = ops.gemm_workspace(single.device, int(_lib.lib().prd_gemm_slab_workspace(M, Hd, S)))
    _lib.check(_lib.lib().prd_single_fc1_folded(_lib.dptr(single), _lib.dptr(og), _lib.dptr(w1cat), _lib.dptr(woT), _lib.dptr(bo), _lib.dptr(wsum1), _lib.dptr(w1bo),
                                                _lib.dptr(b1), _lib.dptr(s1), _lib.dptr(h), M, S, HC, Hd, _lib.dptr(wsb), wsb.numel() * 4, _lib.stream()),
               "prd_single_fc1_folded")
    torch.cuda.synchronize()
    return dict(single_out=(s1, s1.view(-1), [s1]), h=(h, h.view(-1), [h]))


RUN = {"gemm": run_gemm, "ln_rows": run_ln_rows, "softmax_rows": run_softmax_rows, "fc1_folded": run_fc1_folded}


@pytest.mark.parametrize("arith,case", [pytest.param(c.arith, c, id=c.id) for c in T.GPU_CASES], indirect=["arith"])
def test_case_against_float64(arith, case):
    c = case
    inp = R.inputs(c)
    want = R.reference(c, inp, DEV)
    with guarded("nan") as g:
        outs = RUN[c.entry](c, g, inp)
        assert g.intact(), (c.id, g.report())                                               # 1
        assert set(outs) == set(want)
        for name, (got, flat, views) in outs.items():
            assert bool(torch.isfinite(got).all()), f"{c.id} {name}: {int((~torch.isfinite(got)).sum())} of {got.numel()} elements unwritten or non-finite"    # 2
            ok, n = poison_intact_outside(flat, views)
            assert ok, f"{c.id} {name}: {n} elements outside the output region were written"                                                          # 3
        figures = {name: R.measure(got, want[name]) for name, (got, _, _) in outs.items()}
    for name, m in figures.items():
        print(f"\nGEMM_EDGES {R.family(c)} {c.arith} {c.id} {name} " + " ".join(f"{k}={v:.3e}" for k, v in m.items()), end="")
    for name, m in figures.items():
        b = R.bar(c, name)
        assert m["rel"] < b, (c.id, name, m)                                                # 4
        for k in ("row", "col", "small"):                                                   # 5
            assert m.get(k, 0.0) < 2 * b, (c.id, name, k, m)
