"""CPU: the general triangle-attention backward (prd_tri_attn_bwd_core_heads and the statistics-keeping forward entry): their
declarations against the binding table and the library's exports, the host-only answers of the supported-set and workspace queries,
and the dispatch of training.tri_attn_update (every layout and every row length reaches TriAttnFn; nothing recomputes through
torch_ref)."""
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from protein_redesign_amd import _lib, ops, torch_ref, training

ENTRIES = ("prd_tri_attn_bwd_heads_supported", "prd_tri_attn_bwd_heads_workspace_bytes", "prd_tri_attn_bwd_core_heads",
           "prd_tri_attn_core_heads_lse")


def test_header_binding_and_exports():
    text = open(os.path.join(ROOT, "include", "prd_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(prd_\w+)\s*\(", text, flags=re.M))
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in ENTRIES:
        assert n in declared, n
        assert n in _lib.SIGNATURES, n
        assert hasattr(_lib.lib(), n), n
        assert re.search(rf"\bT {n}$", exported, flags=re.M), n
    assert len(_lib.SIGNATURES["prd_tri_attn_bwd_core_heads"]) == 22
    assert len(_lib.SIGNATURES["prd_tri_attn_core_heads_lse"]) == len(_lib.SIGNATURES["prd_tri_attn_core_heads"]) + 1
    assert _lib.lib().prd_version() == 101


@pytest.mark.parametrize("arith", [0, 1])
def test_supported_set(arith):
    raw = _lib.lib()._cdll.prd_tri_attn_bwd_heads_supported
    for H in range(0, 10):
        for c in range(0, 130, 2):
            for P in (16, 32, 48, 64, 128):
                want = int(1 <= H <= 8 and 4 <= c <= 64 and c % 4 == 0 and P in (32, 64))
                assert raw(97, P, H, c, arith) == want, (H, c, P)
    assert raw(0, 64, 8, 32, arith) == 0
    assert raw(1, 64, 8, 32, arith) == 1
    assert raw(100000, 32, 1, 4, arith) == 1            # no row limit
    assert raw(417, 64, 4, 16, arith) == 1              # 4 x 16 beyond the tuned cores
    assert raw(97, 64, 8, 32, 7) == -1                  # an invalid arithmetic word
    assert ops.tri_attn_bwd_heads_supported(320, 64, 4, 16)


def test_workspace_bytes():
    """One slab of round_up(N, 64) x (4 CP + 4) floats per workgroup, CP = c padded to 16 / 32 / 64, at most 256 workgroups (as many
    per head as reach the minimum number of row rounds): bounded by (workgroups) x (N x 4 CP), nothing grows as N^3."""
    q = _lib.lib().prd_tri_attn_bwd_heads_workspace_bytes

    def want(b, N, H, c):
        rows, cap = b * N, 256 // H
        per = max(1, min(cap, rows))
        rounds = -(-rows // per)
        per = -(-rows // rounds)
        cp = 16 if c <= 16 else 32 if c <= 32 else 64
        return per * H * (-(-N // 64) * 64) * (4 * cp + 4) * 4
    for b, N, P, H, c in ((1, 320, 64, 8, 8), (2, 97, 64, 8, 32), (1, 769, 64, 8, 32), (1, 30, 32, 3, 20), (1, 449, 64, 4, 16),
                          (2, 30, 32, 5, 12), (1, 1, 64, 1, 4), (1, 5000, 64, 4, 64)):
        assert q(b, N, P, H, c) == want(b, N, H, c), (b, N, P, H, c)
        assert q(b, N, P, H, c) <= 256 * (N + 63) * (4 * 64 + 4) * 4
    assert q(1, 320, 64, 8, 8) == 256 * 320 * 68 * 4
    for bad in ((0, 30, 64, 8, 32), (1, 0, 64, 8, 32), (1, 30, 48, 8, 32), (1, 30, 64, 9, 32), (1, 30, 64, 4, 18), (1, 30, 64, 4, 128)):
        assert q(*bad) == 0, bad


@pytest.mark.parametrize("H,c,N", [(8, 32, 24), (4, 16, 417)])
def test_tri_attn_update_reaches_the_hand_written_backward(H, c, N, monkeypatch):
    """tri_attn_update hands (8, 32) at N = 24 and 4 x 16 at N = 417 to TriAttnFn: forward on the layout's own core, backward through
    ops.tri_attn_backward, and torch_ref.triangle_attention is never called.  The operators are recorders: nothing runs on a GPU."""
    P = 32
    HC = H * c
    calls = []

    def core(pair, mask, wts, H_, c_, *, ending, lse=None, **kw):
        calls.append(("core" if ops.default_head_layout(H_, c_) else "core_heads", lse is not None))
        return torch.zeros(*pair.shape[:3], HC)

    def out_proj(pair, og, wo, bo, *, residual, out=None):
        calls.append(("out", residual))
        return torch.zeros_like(pair)

    def linear(x, w, bias=None, **kw):
        calls.append(("linear", kw.get("resid") is not None))
        return torch.zeros(*x.shape[:-1], w.shape[0])

    def backward(dy, pair, mask, wts, H_, c_, *, ending, og=None, lse=None, residual=False):
        calls.append(("backward", og is not None, lse is not None))
        return torch.zeros_like(pair), tuple(torch.zeros_like(w) for w in wts)

    def forbidden(*a, **k):
        raise AssertionError("tri_attn_update recomputed through torch_ref.triangle_attention")
    monkeypatch.setattr(ops, "tri_attn_core", core)
    monkeypatch.setattr(ops, "tri_attn_core_heads", core)
    monkeypatch.setattr(ops, "tri_attn_out", out_proj)
    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "tri_attn_backward", backward)
    monkeypatch.setattr(ops, "tri_attn", forbidden)
    monkeypatch.setattr(torch_ref, "triangle_attention", forbidden)
    monkeypatch.setattr(training, "USE_CHECKPOINT", False)
    shapes = [(HC, P), (HC, P), (HC, P), (HC, P), (HC,), (P, HC), (P,)]
    wts = [torch.zeros(*s, requires_grad=True) for s in shapes]
    pair = torch.zeros(1, N, N, P, requires_grad=True)
    mask = torch.ones(1, N)
    ta = SimpleNamespace(attn=SimpleNamespace(num_heads=H, head_dim=c, weights=lambda: wts), mode="ending")
    out = training.tri_attn_update(ta, pair, mask, residual=True)
    assert isinstance(out.grad_fn, training.TriAttnFn._backward_cls)
    grads = torch.autograd.grad(out, [pair, *wts], torch.zeros_like(out))
    assert all(g is not None for g in grads)
    if (H, c) == (4, 16):
        assert calls == [("core", False), ("out", True), ("backward", True, False)]       # long 4 x 16 rows keep no statistics
    else:
        assert calls == [("core_heads", True), ("linear", True), ("backward", True, True)]
    assert training.TRI_ATTN_BWD_MAX_N == 416 == ops.TRI_ATTN_BWD_TUNED_MAX_N
