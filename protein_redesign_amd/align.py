"""Superposition and TM-score of generated samples on the device: ctypes binding of libprd_align.so (include/prd_align.h) and the
public functions on top of it.  The reference's generate.py:163-195 does this per sample with the TM-align program; here the residue
correspondence is known, so what is left is the TM-score superposition search, run for many pairs in one call.

Everything runs on the current stream with no host synchronisation.  HIP only: a missing library or a CPU tensor raises."""
from __future__ import annotations

import dataclasses
import functools

import torch

from ._lib import SideLibrary, dptr, position_mask, stream, structures

_BINDING = SideLibrary("align", 100, "at most {MAX_N} positions per structure (PRD_ALIGN_MAX_N) and 65535 structures per apply")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version      # 100: include/prd_align.h PRD_ALIGN_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_N = _DEFINES["MAX_N"]
MODES = {"tm": _DEFINES["MODE_TM"], "rmsd": _DEFINES["MODE_RMSD"]}
PAIRS_CROSS, PAIRS_SELF = _DEFINES["PAIRS_CROSS"], _DEFINES["PAIRS_SELF"]
_structures = functools.partial(structures, runs="the alignment runs", letter="K")


@dataclasses.dataclass(frozen=True)
class Superposition:
    """Device tensors, one entry per pair: ``ref ~ translation + x @ rotation`` (row vectors, generate.py:180)."""
    tm: torch.Tensor                # [...]
    rmsd: torch.Tensor              # [...] Angstrom, over the masked positions under the transform
    rotation: torch.Tensor          # [..., 3, 3]; determinant -1 where mirrored
    translation: torch.Tensor       # [..., 3]
    mirrored: torch.Tensor          # [...] int32


def _run(x, y, mask, S, R, N, pairs, mode, mirror):
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if N > MAX_N:
        raise ValueError(f"superimpose: {N} positions per structure, at most {MAX_N} (PRD_ALIGN_MAX_N) are supported")
    L = lib()
    x, xs, xr = x
    y, ys, yr = y if y is not None else (None, 0, 0)
    dev = x.device
    nbytes = L.prd_align_workspace_bytes(S, R, N, pairs, MODES[mode], int(bool(mirror)))
    if nbytes == 0:
        raise ValueError(f"superimpose: {S} x {R} structures of {N} positions are outside what the library takes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out = Superposition(torch.empty(S, R, **f32), torch.empty(S, R, **f32), torch.empty(S, R, 3, 3, **f32), torch.empty(S, R, 3, **f32),
                        torch.empty(S, R, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        _check(L.prd_align_superimpose(dptr(out.tm), dptr(out.rmsd), dptr(out.rotation), dptr(out.translation), dptr(out.mirrored, torch.int32),
                                       x.data_ptr(), xs, xr, y.data_ptr() if y is not None else None, ys, yr, dptr(mask),
                                       S, R, N, pairs, MODES[mode], int(bool(mirror)), ws.data_ptr(), nbytes, stream()),
               "prd_align_superimpose")
    return out


def superimpose(x, ref, mask, mirror: bool = True, mode: str = "tm") -> Superposition:
    """Superimpose every structure of ``x`` [S,N,3] on ``ref`` -- [N,3] (results [S]) or [R,N,3] (results [S,R]) -- over the positions
    where ``mask`` [N] is 1.  ``mode="tm"``: the TM-score superposition search; ``"rmsd"``: one Kabsch fit over all masked positions.
    ``mirror``: also try the mirror image of ``x`` and keep the better fit (the network is equivariant under reflections).  ``ref``
    may be a strided view such as ``residue_atom_pos[:, 1]``.  fp32 device tensors; one call, no host synchronisation."""
    x = _structures(x, "x")
    S, N = x[0].shape[:2]
    if not torch.is_tensor(ref) or ref.dim() not in (2, 3):
        raise ValueError("ref must be a [N,3] or [R,N,3] tensor")
    single = ref.dim() == 2
    y = _structures(ref.unsqueeze(0) if single else ref, "ref", N=N)
    if y[0].device != x[0].device:
        raise ValueError(f"ref is on {y[0].device}, x on {x[0].device}")
    R = y[0].shape[0]
    out = _run(x, y, position_mask(mask, "mask", N, x[0].device), S, R, N, PAIRS_CROSS, mode, mirror)
    if single:
        out = Superposition(out.tm[:, 0], out.rmsd[:, 0], out.rotation[:, 0], out.translation[:, 0], out.mirrored[:, 0])
    return out


def pairwise(x, mask, mirror: bool = True, mode: str = "tm") -> Superposition:
    """All pairs of the structures ``x`` [S,N,3] among themselves ([S,S] results): only s < r is searched, (r, s) is its inverse,
    the diagonal is tm 1, rmsd 0, identity."""
    x = _structures(x, "x")
    S, N = x[0].shape[:2]
    return _run(x, None, position_mask(mask, "mask", N, x[0].device), S, S, N, PAIRS_SELF, mode, mirror)


def pairwise_tm(x, mask, mirror: bool = True) -> torch.Tensor:
    """[S,S] TM-scores of the structures ``x`` [S,N,3] among themselves (symmetric, diagonal 1)."""
    return pairwise(x, mask, mirror=mirror).tm


def diversity(x, mask, mirror: bool = True) -> torch.Tensor:
    """Mean pairwise TM-score over s != r (a 0-dim device tensor; NaN for a single structure): the paper's diversity figure."""
    tm = pairwise_tm(x, mask, mirror=mirror)
    S = tm.shape[0]
    return (tm.sum() - tm.diagonal().sum()) / float(S * (S - 1)) if S > 1 else torch.full((), float("nan"), device=tm.device)


def apply(pos, rotation, translation) -> torch.Tensor:
    """``translation + pos @ rotation`` for ``pos`` [S,N,3] (or [N,3]) with one transform per structure: whole rows, ligand atoms
    included.  A new tensor."""
    single = pos.dim() == 2
    p = pos.unsqueeze(0) if single else pos
    if p.dim() != 3 or p.shape[2] != 3:
        raise ValueError(f"pos must be [S,N,3] or [N,3], got {tuple(pos.shape)}")
    S, N = p.shape[:2]
    rot, tr = rotation.reshape(-1, 3, 3), translation.reshape(-1, 3)
    if rot.shape[0] != S or tr.shape[0] != S:
        raise ValueError(f"{S} structures but {rot.shape[0]} rotations and {tr.shape[0]} translations")
    p, rot, tr = p.contiguous(), rot.contiguous(), tr.contiguous()
    out = torch.empty_like(p)
    with torch.cuda.device(p.device):
        _check(lib().prd_align_apply(dptr(out), dptr(p), dptr(rot), dptr(tr), S, N, stream()), "prd_align_apply")
    return out[0] if single else out
