"""Redesign masks: the training-mode draws (reference model.py:442-458, mask_utils.py), the design-region spec of inference
(``Redesign``), and a torch restatement of the device selection.

Under ``--training_mode`` the reference draws, per prepared batch, one of three masks: a stochastic random mask (rt < 0.3), a
spatial mask around the ligand centroid (0.3 <= rt < 0.5), or none.  Everything random about that is drawn HERE, on the CPU,
from a generator keyed like ``synthetic.NoiseSource``; nothing drawn depends on device data, so the mask itself is selected by one
HIP launch without a host synchronisation (``ops.mask_lowest_k``).  ``restate_lowest_k`` says in torch what that launch computes:
the tests hold the kernel and the reference's fixtures against it; the model never calls it (there is no CPU fallback).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np
import torch

_torch_rand, _torch_randperm, _torch_randint = torch.rand, torch.randperm, torch.randint   # bound early: harnesses may patch torch.*

LINSPACE_POINTS = 1000      # mask_utils.py:46: np.linspace(0, max_p, 1000)
ESM_MASK_TOKEN = 32         # mask_utils.py:55, 95


@dataclass
class Draw:
    """What one prepared batch draws.  ``branch``: "random" | "spatial" | "none"; ``fraction``: the p handed to the device (float64
    here, rounded to fp32 on upload); ``keys`` [b,N] fp32 on the CPU (random branch only)."""
    rt: float
    u: float
    branch: str
    fraction: float
    keys: Optional[torch.Tensor] = None
    scale: Optional[float] = None
    idx: Optional[int] = None


class MaskDraws:
    """The draws of ONE prepared batch, keyed by ``(seed, running count of prepared batches)``; a CPU generator, like
    ``synthetic.NoiseSource``.  In the reference's order (model.py:444-455, mask_utils.py:44-49, 80, 88):

    * ``rt`` in [0, 1) and ``u`` = uniform(0.1, mask_prob);
    * rt < 0.3: a scale in [0, 1) (p = scale * u) and, per sample, a key vector = the ranks of a random permutation of the N
      positions, so keys are distinct and the k valid residues with the smallest keys are a uniformly drawn k-subset;
    * 0.3 <= rt < 0.5: an index into ``linspace(0, u, 1000)`` (p = that entry);
    * otherwise nothing more (p = 0: no residue is masked).

    ``draw`` is memoised: a second ``prepare_batch`` of the same batch (the fp32 repeat of a non-finite ``sample()``) sees the same
    mask.  ``recorded``: a mapping with ``rt``, ``u`` and, as the branch needs them, ``scale`` and ``keys`` ([b,N]) or ``idx`` --
    the values are then taken from it instead of the generator (parity tests)."""

    def __init__(self, seed: int = 0, index: int = 0, recorded: Optional[Mapping] = None):
        self.g = torch.Generator().manual_seed((seed * 1_000_003 + 7_919 * index + 1) & 0x7FFFFFFF)
        self.recorded = dict(recorded) if recorded is not None else None
        self._draw = None

    def _uniform(self) -> float:
        return float(_torch_rand(1, generator=self.g, dtype=torch.float64))

    def draw(self, b: int, N: int, mask_prob: float) -> Draw:
        if self._draw is not None:
            return self._draw
        rec = self.recorded
        rt = float(rec["rt"]) if rec is not None else self._uniform()
        u = float(rec["u"]) if rec is not None else 0.1 + (float(mask_prob) - 0.1) * self._uniform()      # np.random.uniform(0.1, mask_prob)
        if rt < 0.3:
            scale = float(rec["scale"]) if rec is not None else self._uniform()
            if rec is not None:
                keys = torch.as_tensor(rec["keys"], dtype=torch.float32).reshape(b, N)
            else:                   # ranks of a permutation: key[perm[j]] = j
                keys = torch.stack([torch.argsort(_torch_randperm(N, generator=self.g)) for _ in range(b)]).to(torch.float32)
            d = Draw(rt, u, "random", scale * u, keys=keys, scale=scale)
        elif rt < 0.5:
            idx = int(rec["idx"]) if rec is not None else int(_torch_randint(0, LINSPACE_POINTS, (1,), generator=self.g))
            d = Draw(rt, u, "spatial", float(np.linspace(0, u, LINSPACE_POINTS)[idx]), idx=idx)
        else:
            d = Draw(rt, u, "none", 0.0)
        self._draw = d
        return d


def keys_from_permutation(residue_mask_row: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """Key vector [N] that makes the device pick what RandomMaskingModule picks with ``torch.randperm(count) = perm`` at batch size
    1 (mask_utils.py:87-92: the residues ``ones[perm[:k]]``): the j-th entry of the permutation gets key j."""
    ones = torch.where(residue_mask_row == 1)[0]
    keys = torch.full(residue_mask_row.shape, float(residue_mask_row.numel()), dtype=torch.float32)
    keys[ones[perm]] = torch.arange(perm.numel(), dtype=torch.float32)
    return keys


def spatial_keys(atom_pos: torch.Tensor, atom_mask: torch.Tensor, ca_pos: torch.Tensor) -> torch.Tensor:
    """fp32 distance of every C-alpha to the ligand centroid, safe_norm as mask_utils.py:12-14, 38-42."""
    centroid = (atom_mask.unsqueeze(-1) * atom_pos).sum(-2) / atom_mask.sum(-1, keepdim=True)
    return torch.sqrt(torch.sum(torch.square(centroid.unsqueeze(-2) - ca_pos), dim=-1) + 1e-12)


def ligand_keys(atom_pos: torch.Tensor, atom_mask: torch.Tensor, ca_pos: torch.Tensor) -> torch.Tensor:
    """fp32 distance of every C-alpha to the NEAREST ligand atom of its sample [b,N] (the ligand key of include/prd_hip.h): the
    minimum over the atoms with atom_mask > 0.5 of safe_norm(ca - atom) = sqrt(((dx*dx + dy*dy) + dz*dz) + 1e-12), every operation
    rounded to fp32 on its own, in the kernel's order.  +inf in a sample without ligand atoms."""
    b, N = atom_mask.shape
    keys = torch.full((b, N), float("inf"), dtype=torch.float32, device=atom_mask.device)
    for s in range(b):
        atoms = atom_pos[s][atom_mask[s] > 0.5].float()
        if atoms.shape[0] == 0:
            continue
        dx, dy, dz = (ca_pos[s].float().unsqueeze(1) - atoms.unsqueeze(0)).unbind(-1)          # [N, atoms] each
        keys[s] = torch.sqrt(((dx * dx + dy * dy) + dz * dz) + 1e-12).min(dim=1).values
    return keys


def restate_lowest_k(residue_mask, p, *, key=None, atom_pos=None, atom_mask=None, ca_pos=None, tokens=None, ligand=None):
    """What ``ops.mask_lowest_k`` computes (include/prd_hip.h: prd_mask_lowest_k), in torch on any device: (extra, inv, tokens).
    ``p``: [b] tensor or a number.  ``tokens`` is NOT modified in place here; the masked copy is returned (None without tokens).
    ``ligand`` = "nearest" | "within": the two ligand modes (``p``: a fraction | a radius in Angstrom), keyed by ``ligand_keys``."""
    rm = residue_mask
    b, N = rm.shape
    valid = rm > 0.5
    counts = valid.sum(-1)
    p32 = torch.as_tensor(p, dtype=torch.float32).reshape(-1).expand(b).cpu()
    spatial = key is None
    if ligand is not None:
        if ligand not in ("nearest", "within") or key is not None:
            raise ValueError("ligand must be 'nearest' or 'within', without key")
        key = ligand_keys(atom_pos, atom_mask, ca_pos)
        has_ligand = (atom_mask > 0.5).any(-1)
        if ligand == "nearest":             # the random mode's k; a sample without ligand atoms selects nothing
            ks = [int(float(counts[s]) * float(p32[s])) if bool(has_ligand[s]) else 0 for s in range(b)]
        else:                               # every valid residue within the radius: no ranking, no k (NaN / negative: nothing)
            inv = (valid & (key <= p32.to(key.device).unsqueeze(-1)) & (p32.to(key.device).unsqueeze(-1) >= 0)
                   & has_ligand.unsqueeze(-1)).to(rm.dtype)
            return _with_tokens(rm, rm * (1 - inv), inv, tokens)
    elif spatial:
        key = spatial_keys(atom_pos, atom_mask, ca_pos)
        median = counts.float().median()                                         # the lower median
        ks = [int((p32[s] * median.cpu()).item()) for s in range(b)]             # fp32 product
    else:
        ks = [int(float(counts[s]) * float(p32[s])) for s in range(b)]          # double product of the fp32 fraction
    extra, inv = rm.clone(), torch.zeros_like(rm)
    for s in range(b):
        k = max(0, min(ks[s], int(counts[s])))
        keyed = torch.where(valid[s], key[s].float(), torch.full_like(key[s], float("inf"), dtype=torch.float32))
        order = torch.sort(keyed, stable=True).indices                          # stable: ties go to the lower index
        sel = order[:k]
        extra[s, sel] = 0
        inv[s, sel] = 1
    return _with_tokens(rm, extra, inv, tokens)


def _with_tokens(rm, extra, inv, tokens):
    out_tokens = None
    if tokens is not None:
        esm = 1 - rm + (ESM_MASK_TOKEN - (1 - rm)) * inv                        # 1 - residue_mask, 32 at the selected positions
        out_tokens = tokens * extra.long() + esm.long()
    return extra, inv, out_tokens


@dataclass(frozen=True, eq=False)
class Redesign:
    """Which residues ``sample()`` redesigns at inference (beyond the reference, whose eval branch removes a random
    ``int(n_res * mask_prob)`` of them).  Immutable and deterministic: a repeated ``prepare_batch`` builds the same mask.

    * ``Redesign.within(radius_angstrom)``: the binding pocket -- every residue whose C-alpha lies within the radius of ANY ligand atom;
    * ``Redesign.nearest(fraction)``: the ``int(n_res * fraction)`` residues of every sample closest to the ligand (same distance);
    * ``Redesign.positions(mask)``: exactly the positions marked 1 in ``mask``, a 0/1 tensor [N] or [b,N] over the collated row
      (ligand atoms first, residues after; positions that are no residue are ignored).

    ``within`` / ``nearest`` are selected by one launch of prd_mask_lowest_k (PRD_MASK_LIGAND_WITHIN / _NEAREST), ``positions`` by
    two elementwise products; none synchronises with the host.  ValueError on construction for a NaN or negative radius, a fraction
    outside [0, 1], a mask that is not 0/1."""
    kind: str
    value: Optional[float] = None
    mask: Optional[torch.Tensor] = None
    keep: Optional[torch.Tensor] = None         # 1 - mask, formed once

    def __post_init__(self):
        if self.kind in ("within", "nearest"):
            v = float(self.value)
            if self.kind == "within" and not v >= 0.0:
                raise ValueError(f"Redesign.within: the radius must be a non-negative number of Angstrom, got {self.value!r}")
            if self.kind == "nearest" and not 0.0 <= v <= 1.0:
                raise ValueError(f"Redesign.nearest: the fraction must lie in [0, 1], got {self.value!r}")
            object.__setattr__(self, "value", v)
            object.__setattr__(self, "mask", None)
            object.__setattr__(self, "keep", None)
        elif self.kind == "positions":
            m = torch.as_tensor(self.mask)
            if m.dim() not in (1, 2) or m.numel() == 0:
                raise ValueError(f"Redesign.positions: the mask must be [N] or [b, N], got shape {tuple(m.shape)}")
            m = m.detach().to(torch.float32)
            if not bool(((m == 0) | (m == 1)).all()):
                raise ValueError("Redesign.positions: the mask must hold only 0 and 1")
            m = m.clone().contiguous()
            object.__setattr__(self, "value", None)
            object.__setattr__(self, "mask", m)
            object.__setattr__(self, "keep", 1 - m)
        else:
            raise ValueError(f"Redesign: kind must be 'within', 'nearest' or 'positions', got {self.kind!r}")

    @classmethod
    def within(cls, radius_angstrom: float) -> "Redesign":
        return cls("within", value=radius_angstrom)

    @classmethod
    def nearest(cls, fraction: float) -> "Redesign":
        return cls("nearest", value=fraction)

    @classmethod
    def positions(cls, mask) -> "Redesign":
        return cls("positions", mask=mask)

    @property
    def needs_structure(self) -> bool:
        """True for the specs keyed on the distance to the ligand: the input must carry the complex's coordinates."""
        return self.kind != "positions"

    def to(self, device) -> "Redesign":
        """The spec with its positions mask on ``device`` (``within`` / ``nearest`` carry no tensor: returned as they are)."""
        if self.mask is None or self.mask.device == torch.device(device):
            return self
        return Redesign("positions", mask=self.mask.to(device))

    def __repr__(self):
        if self.kind == "positions":
            return f"Redesign.positions(<{int(self.mask.sum())} of {tuple(self.mask.shape)}>)"
        return f"Redesign.{self.kind}({self.value!r})"
