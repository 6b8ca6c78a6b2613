"""Python-side operator wrappers over the C ABI (include/prd_hip.h).

Each function takes CUDA fp32 tensors, allocates outputs / scratch with PyTorch's caching allocator,
and enqueues HIP kernels on the current torch stream.  Weight tensors are passed as they sit in the
``state_dict`` (nn.Linear layout).  Nothing here has a CPU implementation.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from typing import Mapping, NamedTuple, Optional, Tuple

import torch

from ._lib import _DEFINES, _TUNE_SHIFT, PrdGemm, arithmetic, check, dptr, lib, stream

F32 = torch.float32


def _device_index(device) -> int:
    idx = torch.device(device).index
    return idx if idx is not None else torch.cuda.current_device()


_QUEUES = {}


def task_queue(device) -> int:
    """Device pointer of the per-device task-queue counters (zero-initialised int32s, see prd_hip.h), or 0 = static
    wave-major task order.  The static order measured faster for every row kernel at the bench shape,
    so the queue is opt-in: PRD_TASK_QUEUE=1."""
    if not os.environ.get("PRD_TASK_QUEUE"):
        return 0
    key = _device_index(device)
    q = _QUEUES.get(key)
    if q is None:
        q = _QUEUES[key] = torch.zeros(256, dtype=torch.int32, device=f"cuda:{key}")
    return q.data_ptr()


class SideStream:
    """Fork / join of a second HIP stream around kernels that do not depend on each other (works eagerly and inside
    ``torch.cuda.graph`` capture, where the branches become parallel paths of the hipGraph): the single track's small kernels at
    the head and tail of a step are independent of the pair-track kernels next to them.  MEASURED SLOWER on MI355X (2.388 vs
    2.350 ms per step, two A/B pairs on one box: the cross-branch dependencies of the replayed graph cost more than the ~70 us
    of small kernels they take off the critical path), so it is OFF unless ``PRD_SIDE_STREAM=1``."""

    def __init__(self, device):
        self.enabled = os.environ.get("PRD_SIDE_STREAM", "0") == "1"
        self.stream = torch.cuda.Stream(device=device) if self.enabled else None

    def fork(self):
        """Context manager: launches inside run on the side stream, ordered after everything enqueued so far on the current one."""
        if not self.enabled:
            return contextlib.nullcontext()
        self.stream.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.stream)

    def join(self):
        """The current stream waits for everything enqueued on the side stream."""
        if self.enabled:
            torch.cuda.current_stream().wait_stream(self.stream)


def _off(t, elem_offset: int = 0) -> int:
    """device address of element ``elem_offset`` of a contiguous tensor (or of a raw device address, for column blocks)"""
    return (t if isinstance(t, int) else dptr(t)) + 4 * elem_offset


def round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def gemm(A, B, Cout, M, N, K, lda, ldb, ldc, *, a_off=0, b_off=0, c_off=0, G1=1, G2=1,
         sa=(0, 0), sb=(0, 0), sc=(0, 0), b_kn=False, alpha=1.0, bias=None, act=0, act_from=0,
         addmat=None, sad=(0, 0), ldadd=0, colmask=None, scm1=0, fill=0.0, rowmask=None, srm1=0,
         mulmat=None, mul_off=0, smu=(0, 0), ldmul=0, resid=None, res_off=0, sr=(0, 0), ldr=0,
         colscale=None, tile_hint=0, a_ln=False, ln_out=None, c2=None, n_split=0, rowmask_cols=0, rscale=None,
         slab=False, wsum=None, out_ln=None, a_scale=0.0, mul_pos=False, a_amax=None, unsupported_ok=False):
    """Raw batched GEMM + epilogue (see PrdGemm in include/prd_hip.h).  ``a_ln`` may be 2 (row softmax of A, see the header);
    with ``unsupported_ok`` a PRD_ERR_UNSUPPORTED shape returns None instead of raising (the caller falls back)."""
    g = PrdGemm()
    g.A, g.B, g.C = _off(A, a_off), _off(B, b_off), _off(Cout, c_off)
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc, g.G1, g.G2 = M, N, K, lda, ldb, ldc, G1, G2
    g.sa1, g.sa2, g.sb1, g.sb2, g.sc1, g.sc2 = sa[0], sa[1], sb[0], sb[1], sc[0], sc[1]
    g.b_kn, g.alpha = int(b_kn), float(alpha)
    g.bias, g.act, g.act_from = dptr(bias), act, act_from
    g.addmat, g.sad1, g.sad2, g.ldadd = dptr(addmat), sad[0], sad[1], ldadd
    g.colmask, g.scm1, g.fill = dptr(colmask), scm1, float(fill)
    g.rowmask, g.srm1 = dptr(rowmask), srm1
    g.mulmat = (_off(mulmat, mul_off) if mulmat is not None else None)
    g.smu1, g.smu2, g.ldmul = smu[0], smu[1], ldmul
    g.resid = (_off(resid, res_off) if resid is not None else None)
    g.sr1, g.sr2, g.ldr = sr[0], sr[1], ldr
    g.colscale, g.tile_hint = dptr(colscale), tile_hint
    g.a_ln = int(a_ln) if a_ln in (1, 2) else (1 if a_ln else 0)
    g.ln_out, g.ldlo = dptr(ln_out), (ln_out.shape[-1] if ln_out is not None else 0)
    g.C2, g.ldc2, g.n_split = dptr(c2), (c2.shape[-1] if c2 is not None else 0), n_split
    g.rowmask_cols, g.rscale = rowmask_cols, dptr(rscale)
    if slab:                        # K split across workgroups (prd_hip.h: PrdGemm.ws); the library falls back by itself if the shape does not qualify
        wsb = gemm_workspace(Cout.device, int(lib().prd_gemm_slab_workspace(M, N, K)))
        g.ws, g.ws_bytes = dptr(wsb), wsb.numel() * 4
    g.wsum = dptr(wsum)
    g.out_ln, g.ldol = dptr(out_ln), (out_ln.shape[-1] if out_ln is not None else 0)
    g.a_scale = float(a_scale)
    g.mul_pos = int(mul_pos)
    g.a_amax = (a_amax if isinstance(a_amax, int) else dptr(a_amax, torch.int32)) if a_amax is not None else None
    g.arith = lib().prd_get_gemm_mode() | (lib().prd_get_tune() << _TUNE_SHIFT)
    code = lib().prd_gemm(ctypes.byref(g), stream())
    if unsupported_ok and code == _DEFINES["ERR_UNSUPPORTED"]:
        return None
    check(code, "prd_gemm")
    return Cout


_GEMM_WS = {}


def gemm_workspace(device, nbytes: int) -> torch.Tensor:
    """Scratch of the K-slab GEMM path (partial tiles; at most a few tens of MB).  Eager launches: one persistent buffer per
    (device, stream) -- the launches that use it are ordered on that stream.  Under graph capture: a fresh tensor per call from the
    capturing graph's own memory pool (the allocator reuses it between the GEMMs of the captured step, which are ordered on the
    capture stream, and the graph keeps the addresses alive exactly as long as it exists; a cached buffer would outlive the graph
    it was carved from)."""
    dev = _device_index(device)
    n = max(1, (nbytes + 3) // 4)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n, device=f"cuda:{dev}", dtype=F32)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)     # per stream: launches on different streams must not share partials
    buf = _GEMM_WS.get(key)
    if buf is None or buf.numel() < n:
        buf = _GEMM_WS[key] = torch.empty(n, device=f"cuda:{dev}", dtype=F32)
    return buf


def split16_gemm_ok(M: int, N: int, K: int) -> bool:
    """True when an unbatched [M, K] x [N, K]^T GEMM lands on the split-16 tile kernel (gemm_h2: split-16 mode, K a multiple of 32,
    at least 512 tiles of 64 x 64) -- otherwise the fp32 tile kernel would run, and for large shapes the BLAS is the better fallback."""
    return lib().prd_get_gemm_mode() == 1 and K % 32 == 0 and ((M + 63) // 64) * ((N + 63) // 64) >= 512


def slab_ok(M: int, N: int, K: int) -> bool:
    """True when a linear of this shape takes the K-slab path (prd_hip.h: prd_gemm_slab_ok) in the current arithmetic."""
    return lib().prd_gemm_slab_ok(M, N, K) == 1


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, act: int = 0,
           alpha: float = 1.0, resid: Optional[torch.Tensor] = None, rowmask: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, ln_a: bool = False, rscale: Optional[torch.Tensor] = None,
           slab: bool = False, wsum: Optional[torch.Tensor] = None, out_ln: Optional[torch.Tensor] = None,
           ln_a_out: Optional[torch.Tensor] = None, relu_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(alpha * x W^T + bias) [* rowmask] [+ resid] for x [..., K], W [N, K]; ``ln_a``: x is LayerNorm-ed
    (no affine) inside the GEMM instead of by a separate launch, and with ``ln_a_out`` [rows, K] the normalised rows are
    written there as well; ``relu_mask`` [rows, N]: y is zeroed where relu_mask <= 0 (the ReLU backward from recomputed activations)."""
    K = x.shape[-1]
    M = x.numel() // K
    N = w.shape[0]
    if ln_a and not ln_fusable(K):
        x, ln_a = layer_norm(x.contiguous()), False
        if ln_a_out is not None:
            ln_a_out.copy_(x.view_as(ln_a_out))
    if out is None:
        out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=F32)
    a, lda = x, K
    if not x.is_contiguous():          # a column block of a wider GEMM output
        a, lda = row_block(x)
    gemm(a, w, out, M, N, K, lda, w.stride(0), N, alpha=alpha, bias=bias, act=act,
         rowmask=rowmask, resid=resid, ldr=N, a_ln=ln_a, rscale=rscale, slab=slab, wsum=wsum, out_ln=out_ln,
         ln_out=ln_a_out if ln_a else None, mulmat=relu_mask, ldmul=N, mul_pos=relu_mask is not None)
    return out


def ln_fusable(K: int) -> bool:
    """PrdGemm.a_ln keeps a lane's K slice in registers: K <= 512 and a multiple of 4 (prd_hip.h)."""
    return K <= 512 and K % 4 == 0


def layer_norm(x: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None) -> torch.Tensor:
    Cn = x.shape[-1]
    rows = x.numel() // Cn
    y = torch.empty_like(x)
    check(lib().prd_ln_rows(dptr(x), dptr(y), dptr(gamma), dptr(beta), rows, Cn, Cn, Cn, stream()), "prd_ln_rows")
    return y


def softmax_rows_(x: torch.Tensor, n: int) -> torch.Tensor:
    ld = x.shape[-1]
    check(lib().prd_softmax_rows(dptr(x), x.numel() // ld, n, ld, stream()), "prd_softmax_rows")
    return x


# ---------------------------------------------------------------------------------------------------
# input stage
# ---------------------------------------------------------------------------------------------------

def static_pair(batch, tabs, max_bond_distance: int, max_relpos: int, P: int) -> torch.Tensor:
    am = batch["atom_mask"]
    b, N = am.shape
    out = torch.empty(b, N, N, P, device=am.device, dtype=F32)
    i64 = torch.int64
    check(lib().prd_static_pair(
        dptr(out), dptr(am), dptr(batch["residue_mask"]), dptr(batch["bond_mask"]),
        dptr(batch["bond_feats"], i64), dptr(batch["bond_distance"], i64),
        dptr(batch["residue_index"], i64), dptr(batch["residue_chain_index"], i64),
        dptr(tabs[0]), dptr(tabs[1]), dptr(tabs[2]), dptr(tabs[3]), dptr(tabs[4]),
        max_bond_distance, max_relpos, b, N, P, stream()), "prd_static_pair")
    return out


def atom_embed(atom_feats, atom_mask, tables_cat, offsets, S: int) -> torch.Tensor:
    b, N, nf = atom_feats.shape
    out = torch.empty(b, N, S, device=atom_mask.device, dtype=F32)
    check(lib().prd_atom_embed(dptr(out), dptr(atom_feats, torch.int64), dptr(atom_mask), dptr(tables_cat),
                               dptr(offsets, torch.int32), nf, b, N, S, stream()), "prd_atom_embed")
    return out


def single_init(static_single, seq_t, residue_mask, w_rt, out=None) -> torch.Tensor:
    b, N, S = static_single.shape
    if out is None:
        out = torch.empty_like(static_single)
    check(lib().prd_single_init(dptr(out), dptr(static_single), dptr(seq_t), dptr(residue_mask), dptr(w_rt),
                                b * N, S, seq_t.shape[-1], stream()), "prd_single_init")
    return out


def time_embed(t, freqs, w_beta, num_steps: int, out=None) -> torch.Tensor:
    b = t.shape[0]
    P, TD = w_beta.shape
    if out is None:
        out = torch.empty(b, P, device=t.device, dtype=F32)
    check(lib().prd_time_embed(dptr(out), dptr(t, torch.int64), dptr(freqs), dptr(w_beta), num_steps, b, P, TD,
                               stream()), "prd_time_embed")
    return out


def pair_init(static_pair_t, z, mask, centers, w_dist, ebeta, out=None) -> torch.Tensor:
    b, N, _, P = static_pair_t.shape
    if out is None:
        out = torch.empty_like(static_pair_t)
    check(lib().prd_pair_init(dptr(out), dptr(static_pair_t), dptr(z), dptr(mask), dptr(centers), dptr(w_dist),
                              dptr(ebeta), b, N, P, w_dist.shape[1], stream()), "prd_pair_init")
    return out


# ---------------------------------------------------------------------------------------------------
# pair-track operators
# ---------------------------------------------------------------------------------------------------

def pair_bias(pair, w, bvec=None, gamma=None, beta=None) -> torch.Tensor:
    b, N, _, P = pair.shape
    H = w.shape[0]
    out = torch.empty(b, H, N, N, device=pair.device, dtype=F32)
    check(lib().prd_pair_bias(dptr(out), dptr(pair), dptr(gamma), dptr(beta), dptr(w), dptr(bvec), b, N, P, H,
                              stream()), "prd_pair_bias")
    return out


def pair_bias2(pair, set_a, set_b):
    """Two pair_bias results from one pass over ``pair``; each set = (w, bvec, gamma, beta) as in pair_bias."""
    b, N, _, P = pair.shape
    (wa, ba, ga, bea), (wb, bb, gb, beb) = set_a, set_b
    Ha, Hb = wa.shape[0], wb.shape[0]
    oa = torch.empty(b, Ha, N, N, device=pair.device, dtype=F32)
    ob = torch.empty(b, Hb, N, N, device=pair.device, dtype=F32)
    check(lib().prd_pair_bias2(dptr(oa), dptr(pair), dptr(ga), dptr(bea), dptr(wa), dptr(ba), Ha,
                               dptr(ob), dptr(gb), dptr(beb), dptr(wb), dptr(bb), Hb, b, N, P, stream()), "prd_pair_bias2")
    return oa, ob


def opm_pair(pair, ab, mask, w_out, b_out, *, residual: bool, apply_mask: bool, out=None) -> torch.Tensor:
    b, N, _, P = pair.shape
    Cc = ab.shape[-1] // 2
    if out is None:
        out = torch.empty_like(pair)
    flags = (1 if residual else 0) | (2 if apply_mask else 0)
    check(lib().prd_opm_pair(dptr(out), dptr(pair), dptr(ab), dptr(mask), dptr(w_out), dptr(b_out), flags,
                             b, N, P, Cc, stream()), "prd_opm_pair")
    return out


def row_block(t: torch.Tensor):
    """(device pointer, row pitch in floats) of ``t`` [b, N, C]: a contiguous tensor or a COLUMN BLOCK of one (``big[..., c0:c1]``:
    unit column stride, rows ``pitch`` floats apart, batches N rows apart) -- how the kernels take an operand that sits inside a
    wider GEMM output."""
    if t.dim() != 3 or t.stride(-1) != 1 or t.stride(0) != t.shape[1] * t.stride(1) or not t.is_cuda or t.dtype != F32:
        raise RuntimeError("expected a CUDA fp32 [b, N, C] tensor or a column block of one")
    if (t.storage_offset() | t.stride(1)) & 3:
        raise RuntimeError("column block must start on a 16-byte boundary and have a row pitch that is a multiple of 4 floats")
    return t.data_ptr(), t.stride(1)


def pair_head_supported(P: int, dist_dim: int, C: int) -> bool:
    """True when the fused head of the pair track (prd_pair_head) exists for these widths in the current arithmetic."""
    return lib().prd_pair_head_supported(P, dist_dim, C) == 1


def pair_head(static_pair_t, z, mask, centers, w_dist, ebeta, ab, w_out, b_out, *, apply_mask: bool, set_a, set_b, out=None):
    """pair_init -> OuterProductUpdate tail (residual) -> two attention-bias heads, one row pass (prd_pair_head).
    set = (w, bvec, gamma, beta) as in pair_bias2.  Returns (pair, bias_a [b,Ha,N,N], bias_b [b,Hb,N,N])."""
    b, N, _, P = static_pair_t.shape
    (wa, ba, ga, bea), (wb, bb_, gb, beb) = set_a, set_b
    Ha, Hb = wa.shape[0], wb.shape[0]
    if out is None:
        out = torch.empty_like(static_pair_t)
    oa = torch.empty(b, Ha, N, N, device=out.device, dtype=F32)
    ob = torch.empty(b, Hb, N, N, device=out.device, dtype=F32)
    check(lib().prd_pair_head(dptr(out), dptr(static_pair_t), dptr(z), dptr(mask), dptr(centers), dptr(w_dist), dptr(ebeta),
                              w_dist.shape[1], dptr(ab), dptr(w_out), dptr(b_out), ab.shape[-1] // 2, int(apply_mask),
                              dptr(oa), dptr(ga), dptr(bea), dptr(wa), dptr(ba), Ha, dptr(ob), dptr(gb), dptr(beb), dptr(wb), dptr(bb_), Hb,
                              b, N, P, stream()), "prd_pair_head")
    return out, oa, ob


def outer_linear_pair(pair, x, u, w, bias, *, residual: bool, out=None) -> torch.Tensor:
    """``u`` [b,N,P]: contiguous, or a column block of a wider GEMM output (row_block)."""
    b, N, _, P = pair.shape
    if out is None:
        out = torch.empty_like(pair)
    up, ldu = row_block(u)
    check(lib().prd_outer_linear(dptr(out), dptr(pair), dptr(x), up, ldu, dptr(w), dptr(bias), int(residual),
                                 b, N, P, x.shape[-1], task_queue(pair.device), stream()), "prd_outer_linear")
    return out


def workspace_bytes(op: str, b: int, N: int, S: int, P: int) -> int:
    return int(lib().prd_workspace_bytes(op.encode(), b, N, S, P))


def tri_mul(pair, mask, wts, *, incoming: bool, residual: bool, out=None, ws=None) -> torch.Tensor:
    """wts = (ab_proj.w, ab_proj.b, ab_gate.w, ab_gate.b, out_proj.w, out_proj.b, out_gate.w, out_gate.b)"""
    b, N, _, P = pair.shape
    if out is None:
        out = torch.empty_like(pair)
    nbytes = workspace_bytes("tri_mul", b, N, 0, P)
    if ws is None:
        ws = torch.empty(nbytes // 4, device=pair.device, dtype=F32)
    check(lib().prd_tri_mul(dptr(out), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(incoming), int(residual),
                            b, N, P, dptr(ws), ws.numel() * 4, task_queue(pair.device), stream()), "prd_tri_mul")
    return out


def tri_mul_chain_supported(N: int, P: int) -> bool:
    """True when the fused outgoing -> incoming chain (prd_tri_mul_chain) exists for this shape in the current arithmetic mode."""
    return lib().prd_tri_mul_chain_supported(N, P) == 1


def tri_mul_chain_(pair, mask, wts_outgoing, wts_incoming, ws=None) -> torch.Tensor:
    """pair += TriMul_outgoing(pair); pair += TriMul_incoming(pair), in place (modules.py:336-337), with the output stage of the
    first and the projection stage of the second fused into one row pass (prd_tri_mul_chain; gemm mode 1)."""
    b, N, _, P = pair.shape
    nbytes = workspace_bytes("tri_mul", b, N, 0, P)
    if ws is None:
        ws = torch.empty(nbytes // 4, device=pair.device, dtype=F32)
    arr = ctypes.c_void_p * 8
    wa = arr(*[dptr(w) for w in wts_outgoing])
    wb = arr(*[dptr(w) for w in wts_incoming])
    check(lib().prd_tri_mul_chain(dptr(pair), dptr(mask), ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(wb, ctypes.c_void_p),
                                  b, N, P, dptr(ws), ws.numel() * 4, stream()), "prd_tri_mul_chain")
    return pair


# 1: the starting triangle attention (core + output projection + residual) and the ending attention's core as ONE persistent launch with
# two in-kernel grid barriers (prd_tri_attn_pair) instead of three launches.  Bit-identical; measured in DESIGN.md 4.3.
PERSISTENT_ATTN = os.environ.get("PRD_PERSISTENT_ATTN", "0") == "1"
_PAIR_BARS = {}


def tri_attn_pair_supported(N: int, P: int) -> bool:
    return lib().prd_tri_attn_pair_supported(N, P) == 1


def tri_attn_pair_bar(device) -> torch.Tensor:
    """The 32 uint32 (counters, memberships, [1] = timeout flag) of prd_tri_attn_pair on ``device``: zeroed by every call, stream-ordered."""
    key = _device_index(device)
    bar = _PAIR_BARS.get(key)
    if bar is None:
        bar = _PAIR_BARS[key] = torch.zeros(32, dtype=torch.int32, device=f"cuda:{key}")
    return bar


def tri_attn_pair_(pair, mask, wts_start, wts_end, H: int, c: int, og=None) -> torch.Tensor:
    """pair += TriangleAttention_starting(pair) in place, then og [b,N,N,64] = the gated head outputs of the ENDING attention on the
    updated pair (its output projection rides in block_tail_): modules.py:338-339 as ONE persistent launch (prd_tri_attn_pair).
    wts_start = (q.w, k.w, v.w, gate.w, gate.b, out.w, out.b), wts_end = (q.w, k.w, v.w, gate.w, gate.b)."""
    b, N, _, P = pair.shape
    if og is None:
        og = torch.empty(b, N, N, 64, device=pair.device, dtype=F32)
    wa = (ctypes.c_void_p * 7)(*[dptr(w) for w in wts_start])
    wb = (ctypes.c_void_p * 5)(*[dptr(w) for w in wts_end])
    bar = tri_attn_pair_bar(pair.device)
    check(lib().prd_tri_attn_pair(dptr(og), dptr(pair), dptr(mask), ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(wb, ctypes.c_void_p),
                                  b, N, P, H, c, bar.data_ptr(), stream()), "prd_tri_attn_pair")
    return og


def tri_attn_pair_timed_out(device) -> bool:
    """True when a grid barrier of the last prd_tri_attn_pair on ``device`` gave up (synchronises; tests and the sampler's final check)."""
    return int(tri_attn_pair_bar(device)[1].item()) != 0


def tri_mul_backward(dy, pair, mask, wts, *, incoming: bool, ws=None):
    """Gradients of the TriangleMultiplication update (ops.tri_mul with residual=False) with respect to ``pair`` and its eight
    weight tensors, on the hand-written backward kernels (csrc/prd_bwd.hip): forward recompute (projection, contraction) ->
    output-stage backward -> the two gradient contractions on the forward contraction kernel -> projection-stage backward.
    The weight gradients are tall-skinny GEMMs over all N^2 rows and go through torch (rocBLAS)."""
    wp, bp, wg, bg, wo, bo, wog, bog = wts
    b, N, _, P = pair.shape
    ldn = round_up(N, 32)
    dev = pair.device
    unit = b * P * N * ldn
    if ws is None:                                       # forward recompute of the operands and the contraction output
        ws = torch.empty(3 * unit, device=dev, dtype=F32)
        scratch = torch.empty_like(pair)
        check(lib().prd_tri_mul(dptr(scratch), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(incoming), 0, b, N, P,
                                dptr(ws), ws.numel() * 4, 0, stream()), "prd_tri_mul (recompute)")
    AB = ws[:2 * unit].view(b, 2 * P, N, ldn)
    O = ws[2 * unit:].view(b, P, N, ldn)
    dy = dy.contiguous()
    dz, dgp, dx1 = torch.empty_like(pair), torch.empty_like(pair), torch.empty_like(pair)
    x, lo = torch.empty_like(pair), torch.empty_like(pair)       # LN(pair), LN(O) by pair position: inputs of the weight gradients
    # dA[i][k] = sum_j dO[i][j] B^T[k][j];  dB[j][k] = sum_i dO^T[j][i] A^T[k][i]: one contraction over the stacked operands
    # dO | dO^T | B^T | A^T (dO written in place by the output-stage backward, the transposes by prd_tri_mul_bwd_operands)
    ops4 = torch.empty(b, 4 * P, N, ldn, device=dev, dtype=F32)
    # max |dO| per complex (float bits): the split-16 contraction scales its gradient operand by a power of two from it
    amax = torch.zeros(b, device=dev, dtype=torch.int32)
    # (the transposed weight images are staged from wo / wog / wp / wg read column-wise: no transposed copies)
    check(lib().prd_tri_mul_out_bwd_amax(dptr(dz), dptr(dgp), dptr(ops4), dptr(dx1), dptr(dy), dptr(pair), dptr(O), dptr(wo), dptr(bo),
                                         dptr(wog), dptr(bog), None, None, dptr(x), dptr(lo), 4 * P, b, N, P, dptr(amax, torch.int32), stream()),
          "prd_tri_mul_out_bwd_amax")
    check(lib().prd_tri_mul_bwd_operands(dptr(ops4), dptr(AB), b, N, P, stream()), "prd_tri_mul_bwd_operands")
    dAB = torch.empty(b, 2 * P, N, ldn, device=dev, dtype=F32)
    check(lib().prd_tri_mul_contract_scaled(dptr(dAB), dptr(ops4), dptr(amax, torch.int32), b, N, 2 * P, stream()), "prd_tri_mul_contract_scaled")
    del ops4
    dpair = torch.empty_like(pair)
    dpp = torch.empty(b, N, N, 2 * P, device=dev, dtype=F32)
    dpg = torch.empty(b, N, N, 2 * P, device=dev, dtype=F32)
    check(lib().prd_tri_mul_proj_bwd(dptr(dpair), dptr(dpp), dptr(dpg), dptr(dAB), dptr(dx1), dptr(pair), dptr(mask), dptr(wp),
                                     dptr(bp), dptr(wg), dptr(bg), None, None, int(incoming), b, N, P, stream()),
          "prd_tri_mul_proj_bwd")
    # weight gradients: dW = dOut^T In over all rows (linear_wgrad)
    x, lo = x.view(-1, P), lo.view(-1, P)
    dz2, dgp2, dpp2, dpg2 = dz.view(-1, P), dgp.view(-1, P), dpp.view(-1, 2 * P), dpg.view(-1, 2 * P)
    grads = (*linear_wgrad(dpp2, x, bias=True), *linear_wgrad(dpg2, x, bias=True), *linear_wgrad(dz2, lo, bias=True),
             *linear_wgrad(dgp2, x, bias=True))
    return dpair, grads


TRI_ATTN_BWD_V2 = os.environ.get("PRD_TRI_ATTN_BWD_V2", "1") != "0"      # 0: the fp32-MFMA backward core in split-16 mode too (A/B measurements)
# longest row of the two 4 x 16 backward cores: q, k, v, do of a row (padded to 32) and the head's weights in LDS, 156 KB (BASELINE draws N <= 384)
TRI_ATTN_BWD_TUNED_MAX_N = 416
# core: the backward core, "v2" (prd_tri_attn_bwd_core_v2) | "tuned" (prd_tri_attn_bwd_core) | "heads" (prd_tri_attn_bwd_core_heads);
# keeps_lse: the forward core leaves the softmax statistics of its queries for it; forward: "core" (tri_attn_core) | "core_heads"
TriAttnBwdPlan = NamedTuple("TriAttnBwdPlan", [("core", str), ("keeps_lse", bool), ("forward", str)])


def tri_attn_bwd_plan(N: int, P: int, H: int, c: int) -> TriAttnBwdPlan:
    """What the triangle-attention backward of this shape runs (long 4 x 16 rows: the general core finds the statistics).  ``core`` and
    ``keeps_lse`` read the arithmetic in force: they hold for the backward where that is the backward's arithmetic (training._pin_arithmetic)."""
    if not default_head_layout(H, c):
        return TriAttnBwdPlan("heads", True, "core_heads")
    if N > TRI_ATTN_BWD_TUNED_MAX_N:
        return TriAttnBwdPlan("heads", False, "core")
    v2 = lib().prd_get_gemm_mode() == 1 and TRI_ATTN_BWD_V2 and lib().prd_tri_attn_bwd_core_v2_supported(N, P) == 1
    return TriAttnBwdPlan("v2" if v2 else "tuned", tri_attn_lse_supported(N, P), "core")


def tri_attn_core_for_bwd(pair, mask, wts, H: int, c: int, *, ending: bool, plan: TriAttnBwdPlan, keep_lse: bool = True):
    """(og, lse) of the plan's forward core: the gated head outputs and, where the plan keeps them and ``keep_lse``, the statistics (else None)."""
    b, N = pair.shape[:2]
    lse = torch.empty(b * N, H, N, 2, device=pair.device, dtype=F32) if keep_lse and plan.keeps_lse else None
    return (tri_attn_core if plan.forward == "core" else tri_attn_core_heads)(pair, mask, wts, H, c, ending=ending, lse=lse), lse


def tri_attn_backward(dy, pair, mask, wts, H: int, c: int, *, ending: bool, og=None, lse=None, residual: bool = False):
    """Gradients of the TriangleAttention update (ops.tri_attn with residual=False; ``residual``: of pair + update, i.e. dy is added
    to the pair gradient) with respect to ``pair`` and its seven weight tensors on the hand-written backward (csrc/prd_bwd.hip):
    out-projection backward (row GEMM) -> attention core backward per (row, head), the core of tri_attn_bwd_plan -> projections backward
    (row GEMM) -> LayerNorm backward.  Weight gradients: slab reductions over all N^2 rows (linear_wgrad)."""
    b, N, _, P = pair.shape
    HC = H * c
    dy2 = dy.contiguous().view(-1, P)
    plan = tri_attn_bwd_plan(N, P, H, c)
    if og is None:                                                                                # forward recompute: gated head outputs
        og, lse = tri_attn_core_for_bwd(pair, mask, wts[:5], H, c, ending=ending, plan=plan)
    # The two activation-gradient GEMMs multiply RAW gradient rows.  The row kernel (pair_linear: rows >= WGRAD_MIN_ROWS, its
    # shapes) normalises every row before the split; where it declines, the GEMM runs on fp32 MFMA whatever the core: a split-16
    # GEMM loses training-scale gradients to the fp16 subnormals (measured at 2 x 24^2 rows, near-init weights: the gradients
    # of the outer-product / outer-linear weights 2e-4 .. 3e-4 off the oracle's, 1e-7 in fp32).
    arith = 0
    dog = rows_linear(dy2, wts[5], transposed=True, fallback_arith=arith)                         # d og = dy W_o
    dqkvg = torch.empty(b, N, N, 4, HC, device=pair.device, dtype=F32)
    x = torch.empty_like(pair) if plan.core != "tuned" else None                                  # LN(pair), left by the core
    if plan.core == "heads":
        tri_attn_bwd_core_heads(dog, og, pair, mask, wts[:5], H, c, ending=ending, lse=lse, x_out=x, dqkvg=dqkvg)
    elif plan.core == "v2":
        check(lib().prd_tri_attn_bwd_core_v2(dptr(dqkvg), dptr(dog), dptr(og), dptr(pair), dptr(mask), *map(dptr, wts[:5]), dptr(lse), dptr(x),
                                             int(ending), b, N, P, H, c, stream()), "prd_tri_attn_bwd_core_v2")
    else:
        check(lib().prd_tri_attn_bwd_core(dptr(dqkvg), dptr(dog), dptr(pair), dptr(mask), *map(dptr, wts[:5]), int(ending), b, N, P, H, c, stream()),
              "prd_tri_attn_bwd_core")
    d2 = dqkvg.view(-1, 4 * HC)                                                                   # (W_q | W_k | W_v | W_g stacked: [4 HC, P])
    dxn = rows_linear(d2, torch.cat(wts[:4], dim=0), transposed=True, fallback_arith=arith)       # gradient of LN(pair)
    dpair = ln_rows_bwd(dxn, pair.view(-1, P), res=dy2 if residual else None).view_as(pair)
    x = (x if x is not None else layer_norm(pair.contiguous())).view(-1, P)
    dw4, db4 = linear_wgrad(d2, x, bias=True)                                                     # d W_q | W_k | W_v | W_g stacked [4 HC, P]
    grads = (dw4[:HC], dw4[HC:2 * HC], dw4[2 * HC:3 * HC], dw4[3 * HC:], db4[3 * HC:], *linear_wgrad(dy2, og.view(-1, HC), bias=True))
    return dpair, grads


WGRAD_MIN_ROWS = 8192


def outer_linear_bwd_reduce(T: torch.Tensor, w1: torch.Tensor, x: torch.Tensor, chunks: int = 4):
    """(dx [R, S] = sum_p T w1,  dw1 [P, S] = sum_r T x) for T [R, P, S], w1 [P, S], x [R, S] (prd_outer_linear_bwd_reduce)."""
    R_, P, S = T.shape
    dx = torch.empty(R_, S, device=T.device, dtype=F32)
    part = torch.empty(chunks, P, S, device=T.device, dtype=F32)
    check(lib().prd_outer_linear_bwd_reduce(dptr(dx), dptr(part), chunks, dptr(T), dptr(w1.contiguous()), dptr(x.contiguous()), R_, P, S, stream()),
          "prd_outer_linear_bwd_reduce")
    return dx, part.sum(0)


def sym_rows(x: torch.Tensor, scale: float = 0.5) -> torch.Tensor:
    """scale * (x + x.transpose(1, 2)) for x [b, N, N, P] (prd_sym_rows)."""
    b, N, _, P = x.shape
    out = torch.empty_like(x)
    check(lib().prd_sym_rows(dptr(out), dptr(x), float(scale), b, N, P, stream()), "prd_sym_rows")
    return out


def sym_transpose(dy: torch.Tensor, amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[b, N, N, P] -> [b, N, P, N]: out[b,i,p,j] = dy[b,i,j,p] + dy[b,j,i,p] (prd_sym_transpose_amax).  ``amax`` (optional, int32 [b],
    zeros): receives max |out| per complex as float bits (PrdGemm.a_amax)."""
    b, N, _, P = dy.shape
    out = torch.empty(b, N, P, N, device=dy.device, dtype=F32)
    check(lib().prd_sym_transpose_amax(dptr(out), dptr(dy), b, N, P, dptr(amax, torch.int32), stream()), "prd_sym_transpose_amax")
    return out


PAIR_LINEAR = os.environ.get("PRD_PAIR_LINEAR", "1") != "0"      # 0: the activation-gradient GEMMs of the backward through prd_gemm (A/B)


def pair_linear(x2: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, ln_in: bool = False,
                xn_out: Optional[torch.Tensor] = None, act: int = 0, relu_mask: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """act(LN?(x2) w^T + bias) over the rows of x2 [rows, K] on the row kernel prd_pair_linear (weights resident in LDS, rows
    streamed), with ``relu_mask`` zeroed where relu_mask <= 0.  Returns None where the row kernel does not serve the call (shape,
    arithmetic, few rows, strided input): the caller then uses ``linear``."""
    rows, K = x2.shape
    OUT = w.shape[0]
    if not (PAIR_LINEAR and x2.is_cuda and x2.is_contiguous() and rows >= WGRAD_MIN_ROWS and lib().prd_pair_linear_supported(K, OUT) == 1):
        return None
    out = torch.empty(rows, OUT, device=x2.device, dtype=F32)
    kn = (not w.is_contiguous()) and w.t().is_contiguous()      # a transposed view of a [K, OUT] matrix: staged as it lies in memory
    wsrc = w.t() if kn else w.contiguous()
    check(lib().prd_pair_linear(dptr(out), dptr(x2), dptr(wsrc), dptr(bias), rows, K, OUT, int(ln_in), dptr(xn_out), act,
                                dptr(relu_mask), int(kn), stream()), "prd_pair_linear")
    return out


def ln_rows_bwd(dy2: torch.Tensor, x2: torch.Tensor, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx of nn.LayerNorm(C, elementwise_affine=False) over the rows of x2 [rows, C] (prd_ln_rows_bwd), plus ``res`` if given."""
    rows, Cn = x2.shape
    dx = torch.empty_like(x2)
    check(lib().prd_ln_rows_bwd(dptr(dx), dptr(dy2), dptr(x2), dptr(res), rows, Cn, stream()), "prd_ln_rows_bwd")
    return dx


def rows_linear(x2: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, transposed: bool = False, ln_in: bool = False,
                xn_out: Optional[torch.Tensor] = None, act: int = 0, relu_mask: Optional[torch.Tensor] = None, fallback_arith=None) -> torch.Tensor:
    """act(LN?(x2) w^T + bias) as [rows, OUT]: ``pair_linear`` where the row kernel serves the call, else the same through ``linear``, that
    fallback alone inside ``arithmetic(fallback_arith)`` (None: a context that does nothing on entry and exit).  ``transposed``: multiply
    by w as [K, OUT] (w.t(); a contiguous copy of it for the GEMM)."""
    y = pair_linear(x2, w.t() if transposed else w, bias, ln_in=ln_in, xn_out=xn_out, act=act, relu_mask=relu_mask)
    if y is None:
        with arithmetic(fallback_arith):
            y = linear(x2, w.t().contiguous() if transposed else w, bias, act=act, ln_a=ln_in, ln_a_out=xn_out, relu_mask=relu_mask)
    return y


def ln_relu_rows(x2: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor):
    """(h, xn) = (relu(W1 LN(x2) + b1), LN(x2)): the forward recompute of a LayerNorm-linear-ReLU, the normalised rows on the side."""
    xn = torch.empty_like(x2)
    return rows_linear(x2, w1, b1, ln_in=True, xn_out=xn, act=1), xn


def pair_bias_bwd(dbias: torch.Tensor, wf: torch.Tensor, pair: torch.Tensor):
    """Backward of an attention-bias head in one pass over the pair rows (prd_pair_bias_bwd): dbias [b, H, N, N] (any layout: made
    contiguous), wf [H, P] (W diag(gamma) for the affine form), pair [b, N, N, P] -> (dx [b N N, P], xn = LN(pair) rows, d2 [b N N, H]);
    None where the kernel does not cover the shape (P = 64, H in (4, 8))."""
    b, N, _, P = pair.shape
    H = wf.shape[0]
    if P != 64 or H not in (4, 8) or not pair.is_cuda:
        return None
    x2 = pair.contiguous().view(-1, P)
    dx, xn = torch.empty_like(x2), torch.empty_like(x2)
    d2 = torch.empty(x2.shape[0], H, device=pair.device, dtype=F32)
    check(lib().prd_pair_bias_bwd(dptr(dx), dptr(xn), dptr(d2), dptr(dbias.contiguous()), dptr(wf.contiguous()), dptr(x2), b, N * N, H, P,
                                  stream()), "prd_pair_bias_bwd")
    return dx, xn, d2


def linear_wgrad(dy2: torch.Tensor, x2: torch.Tensor, bias: bool = False):
    """dW [O, I] = dy2^T x2 for row-major 2-D views dy2 [rows, O] and x2 [rows, I] (row stride = their stride(0), unit column
    stride): the weight gradient of a linear applied at every pair position; with ``bias`` also db [O] = column sums of dy2 from the
    same pass -> (dW, db).  Hand-written slab reduction (prd_linear_wgrad) for the shapes it covers -- rows >= 8192, I a multiple of
    64, O a multiple of 64 or at most 16, both up to 256 -- else a library GEMM."""
    rows, O = dy2.shape
    I = x2.shape[1]
    wide = (O % 64 == 0 and dy2.stride(0) % 2 == 0 and x2.stride(0) % 2 == 0 and dy2.storage_offset() % 2 == 0
            and x2.storage_offset() % 2 == 0)
    if (rows >= WGRAD_MIN_ROWS and (wide or O <= 16) and I % 64 == 0 and O <= 256 and I <= 256 and dy2.stride(1) == 1
            and x2.stride(1) == 1):
        dw = torch.empty(O, I, device=dy2.device, dtype=F32)
        db = torch.empty(O, device=dy2.device, dtype=F32) if bias else None
        nbytes = lib().prd_linear_wgrad_workspace(rows, O, I)
        ws = torch.empty(nbytes // 4, device=dy2.device, dtype=F32)
        check(lib().prd_linear_wgrad(dptr(dw), dptr(db), dy2.data_ptr(), x2.data_ptr(), rows, O, I, dy2.stride(0), x2.stride(0),
                                     dptr(ws), nbytes, stream()), "prd_linear_wgrad")
        return (dw, db) if bias else dw
    dw = dy2.t() @ x2
    return (dw, dy2.sum(0)) if bias else dw


def rbf_rows(z: torch.Tensor, centers: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """[b, N, N, R] radial-basis rows of the pair distances times mask_i mask_j (prd_rbf_rows)."""
    b, N, _ = z.shape
    R_ = centers.numel()
    out = torch.empty(b, N, N, R_, device=z.device, dtype=F32)
    check(lib().prd_rbf_rows(dptr(out), dptr(z.contiguous()), dptr(centers), dptr(mask.contiguous()), b, N, R_, stream()), "prd_rbf_rows")
    return out


def embed_wgrad(idx: torch.Tensor, dy2: torch.Tensor, card: int, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dtable [card, C] = scatter-sum of the rows of dy2 [rows, C] (times ``scale`` [rows] if given) by idx [rows] (int64): the
    gradient of a small embedding table looked up at every pair position (prd_embed_wgrad; card <= 128, C <= 64, contiguous inputs)."""
    rows, Cn = dy2.shape
    dt = torch.empty(card, Cn, device=dy2.device, dtype=F32)
    nbytes = lib().prd_embed_wgrad_workspace(rows, card, Cn)
    ws = torch.empty(nbytes // 4, device=dy2.device, dtype=F32)
    check(lib().prd_embed_wgrad(dptr(dt), dptr(idx, torch.int64), dptr(dy2), dptr(scale), rows, card, Cn, Cn, dptr(ws), nbytes, stream()),
          "prd_embed_wgrad")
    return dt


def embed_wgrad_multi(idxs, dy2: torch.Tensor, cards, scales=None):
    """The gradients of several small tables looked up at the same rows, in one pass over dy2 [rows, C] (prd_embed_wgrad_multi):
    ``idxs`` int64 [rows] each, ``cards`` their table sizes, ``scales`` optional per-set row factors [rows] (entries may be None).
    Returns the list of [card_k, C] gradients."""
    K = len(idxs)
    rows, Cn = dy2.shape
    total = int(sum(cards))
    dt = torch.empty(total, Cn, device=dy2.device, dtype=F32)
    nbytes = lib().prd_embed_wgrad_workspace(rows, total, Cn)
    ws = torch.empty(nbytes // 4, device=dy2.device, dtype=F32)
    ip = (ctypes.c_void_p * K)(*[dptr(i, torch.int64) for i in idxs])
    sp = (ctypes.c_void_p * K)(*[dptr(s) for s in (scales if scales is not None else [None] * K)])
    cp = (ctypes.c_int * K)(*[int(c) for c in cards])
    check(lib().prd_embed_wgrad_multi(dptr(dt), ip, sp, cp, K, dptr(dy2), rows, Cn, Cn, dptr(ws), nbytes, stream()), "prd_embed_wgrad_multi")
    return list(torch.split(dt, [int(c) for c in cards], dim=0))


def tri_attn_uses_long_rows(N: int, P: int) -> bool:
    """True when rows of N positions take the re-projecting long-row core kernel (prd_hip.h: prd_tri_attn_variant)."""
    return tri_attn_variant(N, P) >= 1


def tri_attn_variant(N: int, P: int) -> int:
    """0 short rows, 1 long rows (fp32 kernel), 2 long rows (split-operand kernel), 3 key-chunked rows (N > 960) --
    prd_hip.h: prd_tri_attn_variant."""
    v = lib().prd_tri_attn_variant(N, P)
    if v < 0:
        check(v, "prd_tri_attn_variant")
    return v


HEAD_LAYOUTS = "num_heads 1..8, head_dim a multiple of 4 up to 64, pair_dim 32/64"


def default_head_layout(H: int, c: int) -> bool:
    """4 heads x 16 channels: the layout the tuned triangle-attention kernels (and their fused / persistent forms) serve."""
    return H == 4 and c == 16


def check_head_layout(H: int, c: int, P: int) -> None:
    """Raises ValueError naming the supported set when the GPU path cannot run an attention layout (host-only, no launch)."""
    if not (1 <= H <= 8 and 4 <= c <= 64 and c % 4 == 0 and P in (32, 64)):
        raise ValueError(f"attention layout num_heads={H}, head_dim={c}, pair_dim={P} does not run on the GPU; "
                         f"supported: {HEAD_LAYOUTS}")


MODEL_WIDTHS = ("transition_factor 4; single_dim a multiple of 32 up to 2528 (pair_dim 64) / 5088 (pair_dim 32); "
                "dist_dim a multiple of 8 up to 624 (pair_dim 64) / 1232 (pair_dim 32); esm_dim a multiple of 4; time_dim even, up to 16384")


def _width_refusals(w) -> list:
    """The widths of ``w`` (a mapping; missing keys are not checked) that an entry point of the library refuses, or that it would
    read out of bounds with.  Mirrors the refusals of the C entries: prd_outer_linear (S % 8), prd_opm_pair (C = S/4: C % 8, LDS
    P (C + 4) + P floats <= 160 KiB), prd_pair_init (dist_dim % 8, LDS P (dist_dim + 4) + dist_dim floats <= 160 KiB),
    prd_time_embed (time_dim even; its feature row is the launch's dynamic LDS, 64 KiB), the row GEMMs (lda % 4); the pair-transition
    kernels hard-code the hidden width 4 P and take none."""
    bad = []
    P = w.get("pair_dim")
    if w.get("transition_factor", 4) != 4:
        bad.append(f"transition_factor={w['transition_factor']}")
    if P not in (32, 64):               # refused by every pair entry itself (PRD_ERR_UNSUPPORTED); the LDS limits below are per pair_dim
        P = None
    lds_floats = 40 * 1024
    S = w.get("single_dim")
    if S is not None and (S <= 0 or S % 32 or (P is not None and P * (S // 4 + 4) + P > lds_floats)):
        bad.append(f"single_dim={S}")
    D = w.get("dist_dim")
    if D is not None and (D <= 0 or D % 8 or (P is not None and P * (D + 4) + D > lds_floats)):
        bad.append(f"dist_dim={D}")
    E = w.get("esm_dim")
    if E is not None and (E <= 0 or E % 4):
        bad.append(f"esm_dim={E}")
    T = w.get("time_dim")
    if T is not None and (T <= 0 or T % 2 or T > 16384):
        bad.append(f"time_dim={T}")
    return bad


def check_model_widths(args) -> None:
    """Raises ValueError naming the supported set when a model width cannot run on the GPU (host-only, no launch).  ``args``: a
    mapping or an object with the width attributes (an argparse namespace, the model, its Denoiser); absent widths are skipped."""
    keys = ("single_dim", "pair_dim", "dist_dim", "time_dim", "esm_dim", "transition_factor")
    if isinstance(args, Mapping):
        w = {k: args[k] for k in keys if k in args}
    else:
        w = {k: getattr(args, k) for k in keys if hasattr(args, k)}
    bad = _width_refusals(w)
    if bad:
        raise ValueError(f"model widths {', '.join(bad)} do not run on the GPU; supported: {MODEL_WIDTHS}")


def step_boundary_fusable(time_dim: int) -> bool:
    """True when prd_step_boundary serves this time embedding (its feature row is a fixed 512-float LDS array); wider ones run
    the boundary as separate launches (reverse update, then the next step's single / time-embedding inputs)."""
    return 0 < time_dim <= 512 and time_dim % 2 == 0


def tri_attn_heads_supported(N: int, P: int, H: int, c: int) -> bool:
    """True when prd_tri_attn_core_heads serves this shape (any N; the arithmetic does not matter: fp32 MFMA in both)."""
    return lib().prd_tri_attn_heads_supported(N, P, H, c) == 1


def tri_attn_heads_ws_floats(b: int, N: int, P: int, H: int, c: int) -> int:
    """floats of the workspace of tri_attn_core_heads: og [b,N,N,H c] (+ softmax statistics: none in the single-launch kernel)"""
    return int(lib().prd_tri_attn_heads_workspace_bytes(b, N, P, H, c)) // 4


def tri_attn_core_heads(pair, mask, wts, H: int, c: int, *, ending: bool, ws=None, lse=None) -> torch.Tensor:
    """The general-layout core (prd_tri_attn_core_heads): og [b,N,N,H c] = the gated head outputs, a view of the start of ``ws``
    (allocated here if not given or too small).  wts = (q.w, k.w, v.w, gate.w, gate.b).  ``lse`` [b*N, H, N, 2]: receives
    (m, log2 l) of every query for tri_attn_backward (prd_tri_attn_core_heads_lse; og has the same bits)."""
    b, N, _, P = pair.shape
    check_head_layout(H, c, P)
    need = tri_attn_heads_ws_floats(b, N, P, H, c)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=pair.device, dtype=F32)
    og = ws[:b * N * N * H * c].view(b, N, N, H * c)
    if lse is not None:
        if lse.numel() != b * N * H * N * 2:
            raise ValueError("tri_attn_core_heads: lse must be [b*N, H, N, 2]")
        check(lib().prd_tri_attn_core_heads_lse(dptr(og), dptr(lse), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(ending), b, N, P,
                                                H, c, dptr(ws), ws.numel() * 4, stream()), "prd_tri_attn_core_heads_lse")
        return og
    check(lib().prd_tri_attn_core_heads(dptr(og), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(ending), b, N, P, H, c,
                                        dptr(ws), ws.numel() * 4, stream()), "prd_tri_attn_core_heads")
    return og


def tri_attn_bwd_heads_supported(N: int, P: int, H: int, c: int) -> bool:
    """True when prd_tri_attn_bwd_core_heads serves this shape (the set of the general forward core, any N)."""
    return lib().prd_tri_attn_bwd_heads_supported(N, P, H, c) == 1


def tri_attn_bwd_core_heads(dog, og, pair, mask, wts, H: int, c: int, *, ending: bool, lse=None, x_out=None, dqkvg=None, ws=None):
    """The general backward core (prd_tri_attn_bwd_core_heads) called directly: dqkvg [b,N,N,4,H c] from dog, og [b,N,N,H c];
    wts = (q.w, k.w, v.w, gate.w, gate.b).  ``lse``: the statistics of tri_attn_core_heads(lse=) (None: recomputed in the kernel);
    ``x_out``: receives LN(pair)."""
    b, N, _, P = pair.shape
    HC = H * c
    check_head_layout(H, c, P)
    if dqkvg is None:
        dqkvg = torch.empty(b, N, N, 4, HC, device=pair.device, dtype=F32)
    need = int(lib().prd_tri_attn_bwd_heads_workspace_bytes(b, N, P, H, c)) // 4
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=pair.device, dtype=F32)
    check(lib().prd_tri_attn_bwd_core_heads(dptr(dqkvg), dptr(dog), dptr(og), dptr(pair), dptr(mask), *[dptr(w) for w in wts], dptr(lse),
                                            dptr(x_out), int(ending), b, N, P, H, c, dptr(ws), ws.numel() * 4, stream()),
          "prd_tri_attn_bwd_core_heads")
    return dqkvg


def tri_attn(pair, mask, wts, H: int, c: int, *, ending: bool, residual: bool, out=None, ws=None) -> torch.Tensor:
    """wts = (q.w, k.w, v.w, gate.w, gate.b, out.w, out.b).  Layouts other than 4 x 16: the general core, then the output
    projection (+ bias, + residual) as a row GEMM with K = H c."""
    b, N, _, P = pair.shape
    if not default_head_layout(H, c):
        og = tri_attn_core_heads(pair, mask, wts[:5], H, c, ending=ending, ws=ws)
        return linear(og, wts[5], wts[6], resid=pair if residual else None, out=out)
    if out is None:
        out = torch.empty_like(pair)
    nbytes = workspace_bytes("tri_attn", b, N, 0, P)
    if ws is None:
        ws = torch.empty(nbytes // 4, device=pair.device, dtype=F32)
    check(lib().prd_tri_attn(dptr(out), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(ending), int(residual),
                             b, N, P, H, c, dptr(ws), ws.numel() * 4, task_queue(pair.device), stream()), "prd_tri_attn")
    return out


def pair_transition(pair, w1, b1, w2, b2, *, residual: bool, out=None) -> torch.Tensor:
    b, N, _, P = pair.shape
    if out is None:
        out = torch.empty_like(pair)
    check(lib().prd_pair_transition(dptr(out), dptr(pair), dptr(w1), dptr(b1), dptr(w2), dptr(b2), int(residual),
                                    b, N, P, task_queue(pair.device), stream()), "prd_pair_transition")
    return out


def block_tail_(pair, og, wo, bo, w1, b1, w2, b2, bias_w=None, bias_b=None) -> Optional[torch.Tensor]:
    """In place: pair += W_o og + b_o; pair += transition(pair); returns the next block's attention bias
    [b,H,N,N] = Linear(LN(pair)) when ``bias_w`` is given (else None)."""
    b, N, _, P = pair.shape
    bias_out = None
    H = 0
    if bias_w is not None:
        H = bias_w.shape[0]
        bias_out = torch.empty(b, H, N, N, device=pair.device, dtype=F32)
    check(lib().prd_block_tail(dptr(pair), dptr(og), dptr(wo), dptr(bo), dptr(w1), dptr(b1), dptr(w2), dptr(b2),
                               dptr(bias_w), dptr(bias_b), dptr(bias_out), b, N, P, H, task_queue(pair.device), stream()),
          "prd_block_tail")
    return bias_out


def coord_head(pair, z, mask, w1, b1, w2) -> torch.Tensor:
    b, N, _, P = pair.shape
    out = torch.empty(b, N, 3, device=pair.device, dtype=F32)
    check(lib().prd_coord_head(dptr(out), dptr(pair), dptr(z), dptr(mask), dptr(w1), dptr(b1), dptr(w2), b, N, P,
                               stream()), "prd_coord_head")
    return out


def remove_mean(x, mask) -> torch.Tensor:
    b, N, D = x.shape
    out = torch.empty_like(x)
    check(lib().prd_remove_mean(dptr(out), dptr(x), dptr(mask), b, N, D, stream()), "prd_remove_mean")
    return out


MASK_RANDOM, MASK_SPATIAL, MASK_LIGAND_NEAREST, MASK_LIGAND_WITHIN = 0, 1, 2, 3        # prd_hip.h: PRD_MASK_*
_LIGAND_MODES = {"nearest": MASK_LIGAND_NEAREST, "within": MASK_LIGAND_WITHIN}


def mask_lowest_k(residue_mask, p, *, key=None, atom_pos=None, atom_mask=None, ca_pos=None, tokens=None, out=None,
                  ligand: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The redesign mask of a batch (prd_hip.h: prd_mask_lowest_k): among the valid residues of every sample the k
    with the smallest key leave the known set, k computed on the device from the fraction ``p`` [b] -- one launch on the current
    stream, no host synchronisation.  ``key`` [b,N]: random mode (k = int(count * p) per sample); ``atom_pos`` / ``atom_mask`` /
    ``ca_pos``: spatial mode (key = distance of the C-alpha to the ligand centroid, ONE k from the lower median of the counts).
    ``ligand`` = "nearest" | "within", with ``atom_pos`` / ``atom_mask`` / ``ca_pos`` and no ``key``: the design regions of
    inference -- the key is the distance of the C-alpha to the nearest ligand atom; "nearest" selects the int(count * p) residues
    with the smallest key per sample, "within" every residue whose key is <= ``p``, a radius in Angstrom.
    ``ca_pos`` may be the view ``residue_atom_pos[:, :, 1]``.  ``tokens`` (int64, optional) is masked in place.
    Returns (extra, inv) = residue_mask without the selected positions, and the selected positions (``out``: written there)."""
    b, N = residue_mask.shape
    if ligand is not None:
        if ligand not in _LIGAND_MODES:
            raise ValueError(f"mask_lowest_k: ligand must be 'nearest' or 'within', got {ligand!r}")
        if key is not None:
            raise ValueError("mask_lowest_k: the ligand modes form their own key; key must not be given")
    spatial = key is None
    if spatial and (atom_pos is None or atom_mask is None or ca_pos is None):
        raise ValueError("mask_lowest_k needs either key (random mode) or atom_pos, atom_mask and ca_pos (spatial mode, ligand modes)")
    mode = _LIGAND_MODES[ligand] if ligand is not None else MASK_SPATIAL if spatial else MASK_RANDOM
    ld_ca, ca_ptr = 0, None
    if spatial:
        if not (ca_pos.stride(2) == 1 and ca_pos.stride(0) == N * ca_pos.stride(1) and ca_pos.stride(1) >= 3):
            ca_pos = ca_pos.contiguous()
        if not ca_pos.is_cuda or ca_pos.dtype != F32:
            dptr(ca_pos.contiguous())                   # raises: CPU tensor / wrong type
        ld_ca, ca_ptr = ca_pos.stride(1), ca_pos.data_ptr()
    extra, inv = out if out is not None else (torch.empty_like(residue_mask), torch.empty_like(residue_mask))
    if extra.shape != residue_mask.shape or inv.shape != residue_mask.shape:
        raise ValueError("mask_lowest_k: out must be two tensors of residue_mask's shape")
    err = lib().prd_mask_lowest_k(dptr(extra), dptr(inv), dptr(tokens, torch.int64), dptr(residue_mask), dptr(key), dptr(atom_pos),
                                  dptr(atom_mask), ca_ptr, ld_ca, dptr(p), mode, b, N, stream())
    if ligand is not None and err == -1:
        # PRD_ERR_ARG although the pointers and sizes above are what the entry documents: the library does not know the mode -- a
        # build from before the ligand modes, selected through PRD_LIB
        raise RuntimeError(f"prd_mask_lowest_k: this library does not know mode {mode} (PRD_MASK_LIGAND_{ligand.upper()}): an older "
                           "build selected through PRD_LIB? rebuild it (python -m protein_redesign_amd.build)")
    check(err, "prd_mask_lowest_k")
    return extra, inv


def reverse_update_(z, seq_t, t, noise_pred, seq_pred, noise, mask, coef, num_steps: int):
    """noise: the whole table [T-1, b, N, 3]; the kernel picks row T-1-t and decrements t."""
    b, N, _ = z.shape
    check(lib().prd_reverse_update(dptr(z), dptr(seq_t), dptr(t, torch.int64), dptr(noise_pred), dptr(seq_pred),
                                   dptr(noise), dptr(mask), dptr(coef), b, N, seq_pred.shape[-1], num_steps, stream()),
          "prd_reverse_update")


def step_boundary_(z, seq_t, t, eps_raw, seq_pred, noise, mask, coef, num_steps: int, single_next, static_single, residue_mask,
                   w_rt, ebeta_next, freqs, w_beta, sync, seq_h=None, w_seq=None):
    """Reverse update + the next step's single / time-embedding inputs in one launch (prd_hip.h: prd_step_boundary).
    ``seq_h`` (+ ``w_seq``): the sequence head's hidden units -- its last layer then runs inside this launch and ``seq_pred`` is
    written instead of read."""
    b, N, _ = z.shape
    P, TD = w_beta.shape
    hp, ldh = row_block(seq_h) if seq_h is not None else (None, 0)
    check(lib().prd_step_boundary(dptr(z), dptr(seq_t), dptr(t, torch.int64), dptr(eps_raw), dptr(seq_pred), dptr(noise), dptr(mask),
                                  dptr(coef), dptr(single_next), dptr(static_single), dptr(residue_mask), dptr(w_rt),
                                  dptr(ebeta_next), dptr(freqs), dptr(w_beta), dptr(sync, torch.int32), b, N, seq_pred.shape[-1],
                                  num_steps, static_single.shape[-1], P, TD, hp, ldh, dptr(w_seq),
                                  (seq_h.shape[-1] if seq_h is not None else 0), stream()), "prd_step_boundary")


def tri_attn_stats_floats(b: int, N: int, P: int, H: int = 4) -> int:
    """floats of softmax statistics the key-chunked core needs (0 unless rows exceed the LDS: prd_tri_attn_stats_bytes)"""
    return lib().prd_tri_attn_stats_bytes(b, N, P, H) // 4


def tri_attn_lse_supported(N: int, P: int) -> bool:
    """True when the forward core can keep the softmax statistics of its queries for prd_tri_attn_bwd_core_v2 (split-16 mode, rows
    of up to 384 positions: the second-generation short-row kernels)."""
    return (lib().prd_get_gemm_mode() == 1 and lib().prd_tri_attn_v2_form(N, P) in (1, 2)
            and lib().prd_tri_attn_bwd_core_v2_supported(N, P) == 1 and TRI_ATTN_BWD_V2)


def tri_attn_core(pair, mask, wts, H: int, c: int, *, ending: bool, og=None, stats=None, lse=None) -> torch.Tensor:
    """First launch of tri_attn alone: og[b,N,N,64]; wts = (q.w, k.w, v.w, gate.w, gate.b).  Rows beyond the LDS (N > 960) run
    key-chunked and need ``stats`` (tri_attn_stats_floats; allocated here if not given).  ``lse`` [b*N, H, N, 2] (only where
    tri_attn_lse_supported): receives (m, log2 l) of every query, which the split-16 backward core then does not recompute."""
    b, N, _, P = pair.shape
    if og is None:
        og = torch.empty(b, N, N, 64, device=pair.device, dtype=F32)
    if lse is not None:
        if not tri_attn_lse_supported(N, P) or lse.numel() != b * N * H * N * 2:
            raise ValueError("tri_attn_core: lse is kept by the split-16 short-row kernels only, as [b*N, H, N, 2]")
        check(lib().prd_tri_attn_core_v2_lse(dptr(og), dptr(lse), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(ending),
                                             b, N, P, H, c, stream()), "prd_tri_attn_core_v2_lse")
        return og
    nst = tri_attn_stats_floats(b, N, P, H)
    if nst:
        if stats is None:
            stats = torch.empty(nst, device=pair.device, dtype=F32)
        if stats.numel() < nst:
            raise ValueError("tri_attn_core: stats buffer too small")
        check(lib().prd_tri_attn_core_chunked(dptr(og), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(ending),
                                              b, N, P, H, c, dptr(stats), stats.numel() * 4, stream()), "prd_tri_attn_core_chunked")
        return og
    check(lib().prd_tri_attn_core(dptr(og), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(ending),
                                  b, N, P, H, c, stream()), "prd_tri_attn_core")
    return og


def tri_attn_v2_supported(N: int, P: int) -> bool:
    """True when the second-generation core (csrc/prd_tri2.hip) serves rows of N positions."""
    return lib().prd_tri_attn_v2_supported(N, P) == 1


def tri_attn_core_v2(pair, mask, wts, H: int, c: int, *, ending: bool, og=None) -> torch.Tensor:
    """The second-generation core called directly (split-16 arithmetic whatever the gemm mode); arguments as tri_attn_core."""
    b, N, _, P = pair.shape
    if og is None:
        og = torch.empty(b, N, N, 64, device=pair.device, dtype=F32)
    check(lib().prd_tri_attn_core_v2(dptr(og), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(ending),
                                     b, N, P, H, c, stream()), "prd_tri_attn_core_v2")
    return og


def tri_attn_core_v2_lse(pair, mask, wts, H: int, c: int, *, ending: bool, lse, og=None) -> torch.Tensor:
    """prd_tri_attn_core_v2_lse called directly (split-16 arithmetic whatever the gemm mode): og, and (m, log2 l) of every query
    into ``lse`` [b*N, H, N, 2]."""
    b, N, _, P = pair.shape
    if og is None:
        og = torch.empty(b, N, N, 64, device=pair.device, dtype=F32)
    check(lib().prd_tri_attn_core_v2_lse(dptr(og), dptr(lse), dptr(pair), dptr(mask), *[dptr(w) for w in wts], int(ending),
                                         b, N, P, H, c, stream()), "prd_tri_attn_core_v2_lse")
    return og


def tri_attn_core_fused_supported(N: int, P: int) -> bool:
    """True when prd_tri_attn_core_fused exists for this shape in the current arithmetic mode."""
    return lib().prd_tri_attn_core_fused_supported(N, P) == 1


def tri_attn_core_fused(pair, og_in, wo_in, bo_in, mask, wts, H: int, c: int, *, ending: bool, pair_out, og=None) -> torch.Tensor:
    """og of a triangle attention over the rows of ``pair + og_in W_o^T + b_o`` (the previous attention's residual update,
    applied on the fly and written to ``pair_out``, a different buffer); wts = (q.w, k.w, v.w, gate.w, gate.b)."""
    b, N, _, P = pair.shape
    if og is None:
        og = torch.empty(b, N, N, 64, device=pair.device, dtype=F32)
    check(lib().prd_tri_attn_core_fused(dptr(og), dptr(pair_out), dptr(pair), dptr(og_in), dptr(wo_in), dptr(bo_in), dptr(mask),
                                        *[dptr(w) for w in wts], int(ending), b, N, P, H, c, stream()), "prd_tri_attn_core_fused")
    return og


def tri_attn_out(pair, og, wo, bo, *, residual: bool, out=None) -> torch.Tensor:
    """Second launch of tri_attn alone: (residual ? pair : 0) + og W_o^T + b_o."""
    b, N, _, P = pair.shape
    if out is None:
        out = torch.empty_like(pair)
    check(lib().prd_tri_attn_out(dptr(out), dptr(pair), dptr(og), dptr(wo), dptr(bo), int(residual), b, N, P,
                                 task_queue(pair.device), stream()), "prd_tri_attn_out")
    return out


# ---------------------------------------------------------------------------------------------------
# single-track composites (LayerNorm + GEMMs + softmax)
# ---------------------------------------------------------------------------------------------------

_PACK_GENERATION = 0        # bumped by invalidate_packs(): part of every cached_pack key


def invalidate_packs(*_, **__) -> None:
    """Every pack ``cached_pack`` holds, on every module, is rebuilt at its next use.  Host-only: one integer, no launch, no
    synchronisation.  Call it after changing parameter values by a route ``cached_pack`` cannot see (its docstring lists them): a
    foreign optimiser, a write through ``p.data``.  Takes and ignores any arguments, so it serves as an optimiser hook as it
    stands: ``optimizer.register_step_post_hook(ops.invalidate_packs)`` -- what ``configure_optimizers`` does."""
    global _PACK_GENERATION
    _PACK_GENERATION += 1


def cached_pack(module, name: str, params, build):
    """Memoise ``build()`` -- a packed / concatenated / folded copy of the parameters ``params`` -- on ``module``.

    The pack is rebuilt when, since it was built,
    * a source parameter was written in place through autograd's version counter (``p.copy_`` / ``p.mul_`` ... under ``no_grad``
      or ``inference_mode``, ``load_state_dict``, the EMA swap, an unfused or foreach optimiser step),
    * a source parameter moved (``model.to(device)``, ``load_state_dict(assign=True)``: another ``data_ptr``), or
    * ``invalidate_packs()`` was called.  The optimiser of ``configure_optimizers`` calls it after every ``step()`` (a step post
      hook, whoever steps it), and so does ``training.Fitter`` for any optimiser it drives.  This is what covers the fused Adam:
      its single kernel writes the parameters WITHOUT moving their version counter.
    NOT seen: writes through ``p.data`` (a view with a version counter of its own), a foreign fused optimiser, raw-pointer writes
    -- call ``invalidate_packs()`` after them.  The key is host-side integers only (no launch, no synchronisation); a replayed
    inference graph never comes here."""
    key = (_PACK_GENERATION, *((p.data_ptr(), p._version) for p in params))
    cache = module.__dict__.setdefault("_prd_pack_cache", {})
    hit = cache.get(name)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            cache[name] = (key, build())
    return cache[name][1]


SPA_CORE = os.environ.get("PRD_SPA_CORE", "1") != "0"       # 0: SPAttention's logits / softmax / P V as three GEMM-path launches (A/B)


def pack_attention(wq, wk, wv, wg, bg, q_scale: float):
    """[q | k | v | gate] projections as ONE GEMM: weight [4HC, S], bias (gate only), per-column scale (q only)."""
    HC = wq.shape[0]
    w = torch.cat([wq, wk, wv, wg], dim=0).contiguous()
    bias = torch.cat([torch.zeros(3 * HC, device=w.device, dtype=F32), bg]).contiguous()
    colscale = torch.cat([torch.full((HC,), q_scale, device=w.device, dtype=F32),
                          torch.ones(3 * HC, device=w.device, dtype=F32)]).contiguous()
    return w, bias, colscale


def project_qkvg(x_normed, packed, HC: int, ln_a: bool = False) -> torch.Tensor:
    """[q * scale | k | v | sigmoid(gate)] = one packed GEMM over the node rows (``packed`` from ``pack_attention``)."""
    b, N, S = x_normed.shape
    w, pbias, colscale = packed
    L = 4 * HC
    qkvg = torch.empty(b, N, L, device=x_normed.device, dtype=F32)
    gemm(x_normed, w, qkvg, b * N, L, S, S, S, L, bias=pbias, colscale=colscale, act=2, act_from=3 * HC, a_ln=ln_a)
    return qkvg


def single_attn_core(qkvg, mask, bias, H: int, c: int) -> torch.Tensor:
    """Gated attention output [b,N,H c] BEFORE the output projection from the packed projection ``qkvg`` [b,N,4 H c] (possibly a
    column block of a wider GEMM output): logits + bias + key mask + softmax + P V + gate in one launch (4 heads x 16 channels)."""
    b, N = qkvg.shape[:2]
    o = torch.empty(b, N, H * c, device=qkvg.device, dtype=F32)
    qp, ldq = row_block(qkvg)
    check(lib().prd_single_attn_core(dptr(o), qp, ldq, dptr(bias), dptr(mask) if mask is not None else None,
                                     b, N, H, c, stream()), "prd_single_attn_core")
    return o


def gated_attention_single(x_normed, mask, bias, packed, wo, bo, H: int, c: int, *,
                           key_mask: bool, resid: Optional[torch.Tensor], ln_a: bool = False,
                           qkvg: Optional[torch.Tensor] = None, rscale: Optional[torch.Tensor] = None,
                           out_ln: Optional[torch.Tensor] = None, logits_fp32: bool = True) -> torch.Tensor:
    """Multi-head gated attention over the node axis with an additive [b,H,N,N] bias.

    Covers reference modules.py:185-225 (c = head_dim, key mask filled with -2**15, q pre-scaled by
    1/sqrt(c)) and models/AF2_modules.py:251-293,613-628 (c = single_dim, no mask).  ``packed`` comes
    from ``pack_attention``.  Returns ``resid + out_proj(...)`` (or the bare update when ``resid`` is None).
    ``ln_a``: ``x_normed`` is the raw input and its (affine-free) LayerNorm is fused into the q|k|v|g projection.
    ``qkvg``: the projection, if the caller already computed it (``project_qkvg``, e.g. on a side stream).
    ``rscale``: per-column factor of ``resid`` (an affine-LayerNorm-ed residual given as the plain normalised rows x gamma, with
    beta folded into ``bo`` by the caller).  ``out_ln``: buffer for LN(result) (no affine) -- only with an output projection that takes
    the K-slab path (``slab_ok(b N, S_out, H c)``), whose reduce launch holds whole output rows.  ``logits_fp32`` (wide heads only):
    the logits on fp32 MFMA in either arithmetic -- what a training forward needs (below); sampling passes False."""
    b, N, S = x_normed.shape
    HC = H * c
    w, pbias, colscale = packed
    L = 4 * HC
    if qkvg is None:
        if ln_a and not ln_fusable(S):
            x_normed, ln_a = layer_norm(x_normed.contiguous()), False
        qkvg = project_qkvg(x_normed, packed, HC, ln_a)
    if c == 16 and HC == 64:
        # heads of width 16 (FoldingBlock.single_attn): fused logits + bias + mask + softmax + PV + gate
        o = single_attn_core(qkvg, mask if key_mask else None, bias, H, c)
        return linear(o, wo, bo, resid=resid, rscale=rscale)
    o = torch.empty(b, N, HC, device=x_normed.device, dtype=F32)
    if SPA_CORE and not logits_fp32 and lib().prd_spa_attn_core_supported(N, c) == 1:
        # logits + softmax + P V in one launch (prd_spa_attn_core: split-16 arithmetic; a training forward keeps the fp32-MFMA logits)
        qp, ldq = row_block(qkvg)
        nws = int(lib().prd_spa_attn_core_workspace(b, N, H, c))
        wsb = torch.empty(max(nws // 4, 4), device=o.device, dtype=F32)
        check(lib().prd_spa_attn_core(dptr(o), qp, ldq, dptr(bias), dptr(mask) if key_mask else None, b, N, H, c, dptr(wsb), nws, stream()),
              "prd_spa_attn_core")
        return linear(o, wo, bo, resid=resid, rscale=rscale, slab=slab_ok(b * N, wo.shape[0], HC), out_ln=out_ln)
    ldp = round_up(N, 4)
    logits = torch.empty(b, H, N, ldp, device=x_normed.device, dtype=F32)
    # qkvg may be a column block of a wider projection (the previous block's merged one, FoldingBlock.run_): rows L floats apart
    # when it is contiguous, else its own pitch
    qkvg, L = row_block(qkvg)
    gemm(qkvg, qkvg, logits, N, N, c, L, L, ldp, b_off=HC, G1=b, G2=H, sa=(N * L, c), sb=(N * L, c),
         sc=(H * N * ldp, N * ldp), addmat=bias, sad=(H * N * N, N * N), ldadd=N,
         colmask=(mask if key_mask else None), scm1=N, fill=-(2.0 ** 15),
         tile_hint=32 if logits_fp32 else 0)
    # logits_fp32: fp32 MFMA in either arithmetic -- a softmax follows, and with full-strength weights (|logit| ~ 50) the split
    # operands' 2^-22 shows in the GRADIENTS of q / k at the 1e-4 level (tests/test_training_gpu.py: the backward differentiates an
    # fp32 restatement); a sampling step has no such consumer and stays inside the 1e-5 parity bound with the split operands
    pv = dict(b_off=2 * HC, G1=b, G2=H, sa=(H * N * ldp, N * ldp), sb=(N * L, c), sc=(N * HC, c), b_kn=True, mulmat=qkvg, mul_off=3 * HC,
              smu=(N * L, c), ldmul=L, a_scale=1024.0)                                                        # probabilities: see PrdGemm.a_scale
    # the row softmax rides in the P V product where the library has that form (a_ln = 2); else its own launch
    if ldp != N or gemm(logits, qkvg, o, N, c, N, ldp, L, HC, a_ln=2, unsupported_ok=True, **pv) is None:
        softmax_rows_(logits, N)
        gemm(logits, qkvg, o, N, c, N, ldp, L, HC, **pv)
    return linear(o, wo, bo, resid=resid, rscale=rscale, slab=slab_ok(b * N, wo.shape[0], HC), out_ln=out_ln)


def project_many(single, packed, P_first: int, *, act: int, act_from: int, xhat=None):
    """ONE GEMM over LN(single) (LayerNorm without affine, fused) for several consumers of the same normalised rows:
    ``packed`` = (W [Ncat, S], bias [Ncat] or None, colscale [Ncat] or None).  Returns (x = LN(single) [b,N,S], C [b,N,Ncat]);
    the consumers take column blocks of C (row_block).  ``xhat``: LN(single) if the producer of ``single`` already wrote it."""
    b, N, S = single.shape
    w, pbias, colscale = packed
    Ncat = w.shape[0]
    out = torch.empty(b, N, Ncat, device=single.device, dtype=F32)
    if xhat is not None:
        gemm(xhat, w, out, b * N, Ncat, S, S, S, Ncat, bias=pbias, colscale=colscale, act=act, act_from=act_from)
        return xhat, out
    if ln_fusable(S):
        x = torch.empty_like(single)
        gemm(single, w, out, b * N, Ncat, S, S, S, Ncat, bias=pbias, colscale=colscale, act=act, act_from=act_from, a_ln=True, ln_out=x)
    else:
        x = layer_norm(single)
        gemm(x, w, out, b * N, Ncat, S, S, S, Ncat, bias=pbias, colscale=colscale, act=act, act_from=act_from)
    return x, out


def transition_single(single, w1, b1, w2, b2, *, residual: bool, wsum1=None, want_ln: bool = False):
    """single + W2 relu(W1 LN(single) + b1) + b2 (modules.py:306-311).  ``wsum1`` = row sums of W1: lets the first linear take
    the K-slab path, where the LayerNorm is applied by linearity (PrdGemm.wsum).  ``want_ln``: also return
    LN(result) -- the next linears of the block start with it -- when the second linear runs on the K-slab path, whose
    reduce launch holds whole output rows; returns (result, LN(result) or None) then."""
    b, N, S = single.shape
    Hd = w1.shape[0]
    slab1 = wsum1 is not None and slab_ok(b * N, Hd, S)
    slab2 = slab_ok(b * N, S, Hd)
    h = linear(single, w1, b1, act=1, ln_a=True, slab=slab1, wsum=wsum1 if slab1 else None)   # LayerNorm (no affine) fused into the first linear
    xhat = torch.empty_like(single) if (want_ln and slab2 and S <= 512) else None
    out = linear(h, w2, b2, resid=single if residual else None, slab=slab2, out_ln=xhat)
    return (out, xhat) if want_ln else out


def fc1_fold_ok(M: int, S: int, HC: int, Hd: int) -> bool:
    """True when the attention out-projection can ride in the transition's first layer (prd_hip.h: prd_single_fc1_folded_ok) in
    the current arithmetic; otherwise the out-projection stays a launch of its own."""
    return lib().prd_single_fc1_folded_ok(M, S, HC, Hd) == 1


def pack_fc1_fold(wo, bo, w1):
    """Weights of ``transition_single_folded`` (prd_hip.h: prd_single_fc1_folded): ([W1 | W1 Wo] with the product formed in
    float64 and rounded once, Wo^T, row sums of W1, W1 bo)."""
    w1d, wod = w1.detach().double(), wo.detach().double()
    w1cat = torch.cat([w1.detach().float(), (w1d @ wod).float()], dim=1).contiguous()
    return w1cat, wo.detach().t().contiguous(), w1d.sum(1).float().contiguous(), (w1d @ bo.detach().double()).float().contiguous()


def transition_single_folded(single, og, pack, bo, b1, w2, b2, *, want_ln: bool = False):
    """Attention out-projection + transition of the single track with the projection folded into the first layer:
    s1 = single + og Wo^T + bo;  result = s1 + W2 relu(W1 LN(s1) + b1) + b2, where ``og`` is ``single_attn_core``'s output and
    ``pack`` = ``pack_fc1_fold(Wo, bo, W1)``.  Call only where ``fc1_fold_ok``.  Returns like ``transition_single``."""
    b, N, S = single.shape
    w1cat, woT, wsum1, w1bo = pack
    Hd, HC = w1cat.shape[0], og.shape[-1]
    M = b * N
    s1 = torch.empty_like(single)
    h = torch.empty(b, N, Hd, device=single.device, dtype=F32)
    wsb = gemm_workspace(single.device, int(lib().prd_gemm_slab_workspace(M, Hd, S)))
    check(lib().prd_single_fc1_folded(dptr(single), dptr(og), dptr(w1cat), dptr(woT), dptr(bo), dptr(wsum1), dptr(w1bo), dptr(b1),
                                      dptr(s1), dptr(h), M, S, HC, Hd, dptr(wsb), wsb.numel() * 4, stream()), "prd_single_fc1_folded")
    slab2 = slab_ok(M, S, Hd)
    xhat = torch.empty_like(single) if (want_ln and slab2 and S <= 512) else None
    out = linear(h, w2, b2, resid=s1, slab=slab2, out_ln=xhat)
    return (out, xhat) if want_ln else out
