"""Structural alignment of generated samples to a reference of ANOTHER length on the device: ctypes binding of libprd_tmalign.so
(include/prd_tmalign.h) and the public function on top of it.  The reference's tmalign.py shells out to the TM-align program; here
the cut of TM-align that the header states -- secondary structure, three initial alignments, Needleman-Wunsch refinement with Kabsch
fits, the TM-score search of ``protein_redesign_amd.align`` on the aligned pairs -- runs for all pairs in one call.

Everything runs on the current stream with no host synchronisation.  HIP only: a missing library or a CPU tensor raises."""
from __future__ import annotations

import dataclasses
import functools

import torch

from ._lib import SideLibrary, dptr, position_mask, stream, structures

_BINDING = SideLibrary("tmalign", 100, "at most {MAX_N} positions per structure (PRD_TMALIGN_MAX_N)")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version      # 100: include/prd_tmalign.h PRD_TMALIGN_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_N = _DEFINES["MAX_N"]
_structures = functools.partial(structures, runs="the alignment runs", letter="K")


@dataclasses.dataclass(frozen=True)
class StructuralAlignment:
    """Device tensors, one entry per pair: ``ref[mapping] ~ translation + x @ rotation`` over the aligned rows (row vectors)."""
    tm: torch.Tensor                # [...] normalised by the reference (TM-align's TM2)
    rmsd: torch.Tensor              # [...] Angstrom, over the aligned pairs under the transform
    n_aligned: torch.Tensor         # [...] int32
    rotation: torch.Tensor          # [..., 3, 3]; determinant -1 where mirrored
    translation: torch.Tensor       # [..., 3]
    mirrored: torch.Tensor          # [...] int32
    mapping: torch.Tensor           # [..., Nx] int32: the row of ref aligned to row i of x, or -1


def align(x, ref, mask, ref_mask, mirror: bool = True) -> StructuralAlignment:
    """Align every structure of ``x`` [S,Nx,3] to ``ref`` -- [Ny,3] (results [S]) or [R,Ny,3] (results [S,R]) -- by structure: the rows
    where ``mask`` [Nx] / ``ref_mask`` [Ny] are 1 take part, and the correspondence between them is found, not assumed.  ``mirror``:
    also try the mirror image of ``x`` and keep the better alignment.  ``ref`` may be a strided view such as
    ``residue_atom_pos[:, 1]``.  fp32 device tensors; one call, no host synchronisation."""
    x = _structures(x, "x")
    S, Nx = x[0].shape[:2]
    if not torch.is_tensor(ref) or ref.dim() not in (2, 3):
        raise ValueError("ref must be a [N,3] or [R,N,3] tensor")
    single = ref.dim() == 2
    y = _structures(ref.unsqueeze(0) if single else ref, "ref")
    if y[0].device != x[0].device:
        raise ValueError(f"ref is on {y[0].device}, x on {x[0].device}")
    R, Ny = y[0].shape[:2]
    dev = x[0].device
    mx, my = position_mask(mask, "mask", Nx, dev), position_mask(ref_mask, "mask", Ny, dev)
    if max(Nx, Ny) > MAX_N:
        raise ValueError(f"align: {max(Nx, Ny)} positions per structure, at most {MAX_N} (PRD_TMALIGN_MAX_N) are supported")
    L = lib()
    nbytes = L.prd_tmalign_workspace_bytes(S, R, Nx, Ny, int(bool(mirror)))
    if nbytes == 0:
        raise ValueError(f"align: {S} x {R} structures of {Nx} and {Ny} positions are outside what the library takes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    out = StructuralAlignment(torch.empty(S, R, **f32), torch.empty(S, R, **f32), torch.empty(S, R, **i32), torch.empty(S, R, 3, 3, **f32),
                              torch.empty(S, R, 3, **f32), torch.empty(S, R, **i32), torch.empty(S, R, Nx, **i32))
    with torch.cuda.device(dev):
        _check(L.prd_tmalign_align(dptr(out.tm), dptr(out.rmsd), dptr(out.rotation), dptr(out.translation), dptr(out.n_aligned, torch.int32),
                                   dptr(out.mirrored, torch.int32), dptr(out.mapping, torch.int32),
                                   x[0].data_ptr(), x[1], x[2], dptr(mx), y[0].data_ptr(), y[1], y[2], dptr(my),
                                   S, R, Nx, Ny, int(bool(mirror)), ws.data_ptr(), nbytes, stream()), "prd_tmalign_align")
    if single:
        out = StructuralAlignment(*(getattr(out, f.name)[:, 0] for f in dataclasses.fields(out)))
    return out
