"""Structure-conditioned sampling: which rows of a complex the reverse-diffusion loop keeps where the input structure has them
(``Scaffold``), the ctypes binding of libprd_condition.so (include/prd_condition.h) that holds them there, and a torch restatement of
what that launch computes.

The method is replacement conditioning in the centred frame.  With ``x0c`` the input structure minus its masked mean and
``A[l] = sqrt_alphas_cumprod[l]``, ``S[l] = sqrt_one_minus_alphas_cumprod[l]`` of the model's own schedule, the state ENTERING the step
with counter ``l`` has ``z[K] = A[l] * x0c[K] + S[l] * eps_l[K]`` on the kept rows ``K`` -- the forward process ``q`` of training with a
fresh, mean-free ``eps_l`` per level -- and ``z[K] = x0c[K]`` after the last step.  Every other row follows the reverse update as it
always did.  ``start = L`` begins the loop at level ``L`` from the noised input instead of from pure noise (partial diffusion).  The
loop itself is ``diffusion_model.ReverseDiffusion(..., scaffold=...)``; this module holds the spec, the launcher and the restatement.
``restate_rows`` says in torch what the launch computes: the tests hold the kernel against it; the model never calls it (there is no
CPU fallback)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Mapping, Optional

import torch

from ._lib import SideLibrary, dptr, stream

_BINDING = SideLibrary("condition", 100, "sequence rows of {N_CLS} classes (PRD_CONDITION_N_CLS), at most {MAX_B} samples per call "
                       "(PRD_CONDITION_MAX_B) of {MAX_N} positions (PRD_CONDITION_MAX_N)")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version    # 100: include/prd_condition.h PRD_CONDITION_VERSION
lib, _check = _BINDING.lib, _BINDING.check
N_CLS = _DEFINES["N_CLS"]
BATCH_KEY = "scaffold_keep"         # where a conditioned loop leaves the rows it kept, [b,N] 0/1, in the prepared batch


def level_table(tables: Mapping[str, torch.Tensor]) -> torch.Tensor:
    """[T,2] = (sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod) per level, from schedule tables as ``schedule.schedule_tables``
    builds them (the model's own attributes): the ``level`` argument of the launch.  No arithmetic, so bit-equal to its sources."""
    return torch.stack([tables["sqrt_alphas_cumprod"], tables["sqrt_one_minus_alphas_cumprod"]], dim=1).to(torch.float32).contiguous()


def _tensor(t, name, shape, like, dtype=torch.float32, runs="the conditioning runs", ref="the state"):
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a tensor of shape {tuple(shape)}, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: {runs} on the GPU only (got a CPU tensor); there is no CPU fallback")
    if like is not None and t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, {ref} on {like.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def condition_rows_(z, seq_t, t, *, x0c=None, keep_z=None, noise=None, level=None, seq0=None, keep_seq=None):
    """One launch of prd_condition_rows (include/prd_condition.h) on the current stream, in place, no host synchronisation: the rows of
    ``z`` [b,N,3] marked in ``keep_z`` [b,N] become ``level[l,0] * x0c + level[l,1] * noise[l]`` with ``l = t[s]`` the device-resident
    counter of the sample (``x0c`` where ``l < 0``, untouched where ``l >= noise.shape[0]``), the rows of ``seq_t`` [b,N,21] marked in
    ``keep_seq`` become those of ``seq0``.  ``keep_z`` / ``keep_seq`` may each be None (with what belongs to them); ``z`` and ``seq_t``
    may be None when their mask is.  Every argument is checked here: shape, dtype, device, contiguity."""
    ref = z if z is not None else seq_t
    if ref is None or not torch.is_tensor(ref) or ref.dim() != 3:
        raise ValueError("condition_rows_: z [b,N,3] or seq_t [b,N,n_cls] must be given")
    b, N = ref.shape[:2]
    if keep_z is not None and (noise is None or not torch.is_tensor(noise) or noise.dim() != 4):
        raise ValueError("condition_rows_: keep_z needs noise [levels,b,N,3]")
    if keep_seq is not None and (seq_t is None or not torch.is_tensor(seq_t) or seq_t.dim() != 3):
        raise ValueError("condition_rows_: keep_seq needs seq_t [b,N,n_cls]")
    _tensor(t, "t", (b,), None, torch.int64)
    ref = t
    levels, n_cls = 1, N_CLS
    if keep_z is not None:
        levels = noise.shape[0]
        _tensor(z, "z", (b, N, 3), ref), _tensor(x0c, "x0c", (b, N, 3), ref), _tensor(keep_z, "keep_z", (b, N), ref)
        _tensor(noise, "noise", (levels, b, N, 3), ref)
        if not torch.is_tensor(level) or level.dim() != 2 or level.shape[1] != 2 or level.shape[0] < levels:
            raise ValueError(f"level must be a [T,2] tensor with T >= {levels} (the levels of noise)")
        _tensor(level, "level", level.shape, ref)
    if keep_seq is not None:
        n_cls = seq_t.shape[2]
        _tensor(seq_t, "seq_t", (b, N, n_cls), ref), _tensor(seq0, "seq0", (b, N, n_cls), ref), _tensor(keep_seq, "keep_seq", (b, N), ref)
    with torch.cuda.device(t.device):
        _check(lib().prd_condition_rows(dptr(z) if keep_z is not None else None, dptr(seq_t) if keep_seq is not None else None,
                                        dptr(t, torch.int64), dptr(x0c), dptr(keep_z), dptr(noise), dptr(level), dptr(seq0), dptr(keep_seq),
                                        b, N, n_cls, levels, stream()), "prd_condition_rows")


def restate_rows(z, seq_t, t, *, x0c=None, keep_z=None, noise=None, level=None, seq0=None, keep_seq=None):
    """What ``condition_rows_`` computes, in torch on any device, NOT in place: (z, seq_t) after the launch (None where None went
    in).  Same operation order: two fp32 products, each rounded on its own, then their fp32 sum."""
    zo = z.clone() if z is not None else None
    so = seq_t.clone() if seq_t is not None else None
    if keep_z is not None:
        levels = noise.shape[0]
        for s in range(z.shape[0]):
            l = int(t[s])
            if l >= levels:
                continue
            rows = keep_z[s] >= 0.5
            if l < 0:
                zo[s, rows] = x0c[s, rows]
            else:
                a = level[l, 0] * x0c[s, rows]
                n = level[l, 1] * noise[l, s, rows]
                zo[s, rows] = a + n
    if keep_seq is not None:
        rows = keep_seq >= 0.5
        so[rows] = seq0[rows]
    return zo, so


@dataclass(frozen=True, eq=False)
class Scaffold:
    """Which rows of the complex ``sample()`` keeps where the input structure has them, and where the loop starts.  Immutable and
    deterministic, validated on construction (ValueError), keyword only: there is no model attribute.

    * ``keep="outside"``: the residues outside the design region -- ``residue_extra_mask`` of the prepared batch, whichever way the
      region was chosen (``Redesign.within(8.0)``, explicit positions, the random subset);
    * ``keep=<0/1 tensor [N] or [b,N]>`` over the collated row (ligand atoms first, residues after): the residues marked 1; positions
      that are no residue are ignored (the ligand is ``ligand=``'s to say);
    * ``Scaffold.beyond(radius_angstrom)``: every residue whose C-alpha is farther than the radius from ALL ligand atoms -- one launch
      of prd_mask_lowest_k (PRD_MASK_LIGAND_WITHIN) at this radius, which may be wider than the shell that is resequenced;
    * ``keep=None`` with ``start``: nothing is kept, pure partial diffusion;
    * ``ligand=True``: the ligand atoms keep their pose too;
    * ``sequence=True``: after every step the residues with a known sequence (``residue_extra_mask``) get their one-hot row back, as
      training holds them at every t; by default they are held at initialisation only, as the reference's sampler does;
    * ``start=L`` (0 <= L <= num_steps - 1): every valid row starts from the input noised to level L, and the loop runs the L + 1 steps
      from counter L down, consuming the reverse-update noise the uninterrupted loop consumes from that level on.

    None of it synchronises with the host."""
    keep: object = "outside"
    ligand: bool = False
    sequence: bool = False
    start: Optional[int] = None
    radius: Optional[float] = None          # set by ``beyond`` alone

    def __post_init__(self):
        keep = self.keep
        if self.radius is not None:
            r = float(self.radius)
            if not (r >= 0.0 and math.isfinite(r)):
                raise ValueError(f"Scaffold.beyond: the radius must be a non-negative, finite number of Angstrom, got {self.radius!r}")
            object.__setattr__(self, "radius", r)
            object.__setattr__(self, "keep", "beyond")
        elif isinstance(keep, str):
            if keep != "outside":
                raise ValueError(f"Scaffold: keep must be 'outside', None or a 0/1 tensor, got {keep!r} (a radius: Scaffold.beyond)")
        elif keep is not None:
            m = torch.as_tensor(keep)
            if m.dim() not in (1, 2) or m.numel() == 0:
                raise ValueError(f"Scaffold: the keep mask must be [N] or [b, N], got shape {tuple(m.shape)}")
            m = m.detach().to(torch.float32)
            if not bool(((m == 0) | (m == 1)).all()):
                raise ValueError("Scaffold: the keep mask must hold only 0 and 1")
            object.__setattr__(self, "keep", m.clone().contiguous())
        if self.start is not None:
            if isinstance(self.start, bool) or int(self.start) != self.start or int(self.start) < 0:
                raise ValueError(f"Scaffold: start must be a non-negative integer level, got {self.start!r}")
            object.__setattr__(self, "start", int(self.start))
        elif keep is None:
            raise ValueError("Scaffold: keep=None keeps nothing; give start= (partial diffusion) or rows to keep")
        object.__setattr__(self, "ligand", bool(self.ligand))
        object.__setattr__(self, "sequence", bool(self.sequence))

    @classmethod
    def beyond(cls, radius_angstrom: float, ligand: bool = False, sequence: bool = False, start: Optional[int] = None) -> "Scaffold":
        if radius_angstrom is None:
            raise ValueError("Scaffold.beyond: the radius must be a non-negative, finite number of Angstrom, got None")
        return cls("beyond", ligand, sequence, start, radius=radius_angstrom)

    @property
    def needs_ligand(self) -> bool:
        """True when the input must carry ligand positions: the ligand is kept, or the rows are chosen by their distance to it."""
        return self.ligand or self.radius is not None

    def to(self, device) -> "Scaffold":
        """The spec with its keep mask on ``device`` (the other kinds carry no tensor: returned as they are)."""
        if not torch.is_tensor(self.keep) or self.keep.device == torch.device(device):
            return self
        return Scaffold(self.keep.to(device), self.ligand, self.sequence, self.start)

    def rows(self, batch) -> Optional[torch.Tensor]:
        """K [b,N] 0/1 on the device of the PREPARED ``batch`` (None: nothing is kept), built without a host synchronisation."""
        from . import ops
        rm, am = batch["residue_mask"], batch["atom_mask"]
        b, N = rm.shape
        if self.radius is not None:
            p = torch.full((b,), self.radius, dtype=torch.float32, device=rm.device)
            keep, _ = ops.mask_lowest_k(rm.contiguous(), p, atom_pos=batch["atom_pos"].contiguous(), atom_mask=am.contiguous(),
                                        ca_pos=batch["residue_atom_pos"][:, :, 1], ligand="within")
        elif self.keep is None:
            keep = None
        elif isinstance(self.keep, str):
            keep = batch["residue_extra_mask"]
        else:
            m = self.keep
            if m.shape[-1] != N or (m.dim() == 2 and m.shape[0] not in (1, b)):
                raise ValueError(f"Scaffold: a keep mask of shape {tuple(m.shape)} does not fit a batch of shape {(b, N)}")
            keep = rm * m.to(rm.device)
        if self.ligand:
            keep = am if keep is None else keep + am        # atoms and residues share no row
        return keep.to(torch.float32).contiguous() if keep is not None else None

    def __repr__(self):
        kind = (f"beyond({self.radius!r})" if self.radius is not None else
                f"<{int(self.keep.sum())} of {tuple(self.keep.shape)}>" if torch.is_tensor(self.keep) else repr(self.keep))
        return f"Scaffold({kind}, ligand={self.ligand}, sequence={self.sequence}, start={self.start})"
