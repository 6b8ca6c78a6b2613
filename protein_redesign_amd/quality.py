"""Scores of generated samples that need no superposition, on the device: ctypes binding of libprd_quality.so (include/prd_quality.h)
and the public functions on top of it -- ``lddt`` (the local distance difference test, also in its protein-ligand form), ``contacts``
(a census of close pairs with the distance to the nearest partner) and ``assess`` (the named metrics of a protein-ligand complex built
from the two).  ``align.py`` answers "how close is the fold after a global fit"; this module answers the local questions: is the pocket
preserved, is the ligand pose physically possible, is the chain a chain, which residues line the pocket.

EVERY metric here is built from distances alone, so a mirror image scores exactly like the original.  Chirality is what
``protein_redesign_amd.chirality`` reads off the sample itself (``pipeline.generate_samples(handedness=...)``) and what
``alignment["mirrored"]`` of ``pipeline.generate_samples(align_to=...)`` reports against a reference, not this module.

Everything runs on the current stream with no host synchronisation.  HIP only: a missing library or a CPU tensor raises."""
from __future__ import annotations

import dataclasses
import functools
import math

import torch

from ._lib import SideLibrary, dptr, position_mask as _mask, stream, structures

_BINDING = SideLibrary("quality", 100, "at most {MAX_N} positions per structure (PRD_QUALITY_MAX_N) and {MAX_S} structures per call")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version      # 100: include/prd_quality.h PRD_QUALITY_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_N, MAX_S = _DEFINES["MAX_N"], _DEFINES["MAX_S"]
_structures = functools.partial(structures, runs="the quality scores run", letter="S", bounds=_BINDING)
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)       # Angstrom; fixed in the kernel, stated here for readers and for the tests

# the documented defaults of ``assess`` (Angstrom); each is a keyword of it
CA_CLASH, LIGAND_CLASH, LIGAND_SELF_CLASH, SELF_CLASH_MIN_BONDS = 3.0, 2.5, 2.0, 4
BOND_RANGE, CA_STEP, CA_STEP_TOLERANCE, POCKET = (0.9, 2.1), 3.8, 0.5, 8.0
LDDT_RADIUS, LDDT_PLI_RADIUS = 15.0, 10.0
SCALAR_COLUMNS = ("ca_clashes", "ligand_clashes", "ligand_self_clashes", "ligand_bond_outliers", "chain_breaks", "pocket_size",
                  "lddt_ca", "lddt_pli", "lddt_ligand", "pocket_recall")      # the column order of sample_quality.txt (those present)


@dataclasses.dataclass(frozen=True)
class LDDT:
    """Device tensors.  ``per_position`` is NaN where a position has no included pair; ``score`` pools the pairs of a whole structure
    (sum of preserved over 4 x sum of total -- NOT the mean of ``per_position``)."""
    per_position: torch.Tensor      # [S,N] float64
    score: torch.Tensor             # [S] float64
    preserved: torch.Tensor         # [S,N] int32: over the included pairs of a row, how many of the 4 thresholds each one meets
    total: torch.Tensor             # [N] int32: included pairs of a row (the reference's alone)


@dataclasses.dataclass(frozen=True)
class Contacts:
    count: torch.Tensor             # [S] int32
    nearest: torch.Tensor           # [S,N] float32 Angstrom, +inf where a row has no partner or is outside A


def _bound(value, name):
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"{name} must be a positive, finite number of Angstrom, got {value!r}")
    return value


def lddt(x, ref, mask, partner_mask=None, radius: float = LDDT_RADIUS) -> LDDT:
    """The local distance difference test of every structure of ``x`` [S,N,3] against ``ref`` [N,3], without superposition.  A pair
    (i, j) is included when ``mask[i]`` and ``partner_mask[j]`` are 1 (``partner_mask=None``: ``mask``), i != j and the reference
    distance is below ``radius``; it scores the share of the thresholds 0.5, 1, 2, 4 Angstrom within which the sample's distance agrees
    with the reference's.  Rows = columns = residues gives lDDT-C-alpha; rows = ligand atoms, columns = residues its protein-ligand
    form.  ``ref`` may be a strided view such as ``residue_atom_pos[:, 1]``.  fp32 device tensors; one launch, no host synchronisation.
    The device returns integer counts (deterministic); the scores are their quotients in float64."""
    radius = _bound(radius, "radius")
    x, xs, xr = _structures(x, "x")
    S, N = x.shape[:2]
    if not torch.is_tensor(ref) or ref.shape != (N, 3):
        raise ValueError(f"ref must be a [{N},3] tensor, got {tuple(ref.shape) if torch.is_tensor(ref) else type(ref).__name__}")
    if ref.dtype != torch.float32:
        raise ValueError(f"ref must be float32, got {ref.dtype}")
    if ref.device != x.device:
        raise ValueError(f"ref is on {ref.device}, x on {x.device}")
    if ref.stride(1) != 1 or ref.stride(0) < 3:
        ref = ref.contiguous()
    rows = _mask(mask, "mask", N, x.device)
    cols = rows if partner_mask is None else _mask(partner_mask, "partner_mask", N, x.device)
    preserved = torch.empty(S, N, dtype=torch.int32, device=x.device)
    total = torch.empty(N, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().prd_quality_lddt(dptr(preserved, torch.int32), dptr(total, torch.int32), x.data_ptr(), xs, xr, ref.data_ptr(), ref.stride(0),
                                      dptr(rows), dptr(cols), radius, S, N, stream()), "prd_quality_lddt")
    denom = 4.0 * total.double()
    return LDDT(preserved.double() / denom, preserved.sum(1).double() / denom.sum(), preserved, total)


def contacts(x, a_mask, b_mask, cutoff: float, exclude=None) -> Contacts:
    """A census of close pairs in every structure of ``x`` [S,N,3].  A pair (i, j) qualifies when ``a_mask[i]`` and ``b_mask[j]`` are 1,
    i != j and ``exclude[i, j]`` is 0 (``exclude``: an [N,N] bool / uint8 tensor or None).  ``count`` [S]: the qualifying pairs closer
    than ``cutoff``, a pair that qualifies in both orders counted once; ``nearest`` [S,N]: for i in A the distance to its nearest
    qualifying partner whatever the cutoff (+inf without one, and outside A).  fp32 device tensors; no host synchronisation."""
    cutoff = _bound(cutoff, "cutoff")
    x, xs, xr = _structures(x, "x")
    S, N = x.shape[:2]
    a, b = _mask(a_mask, "a_mask", N, x.device), _mask(b_mask, "b_mask", N, x.device)
    if exclude is not None:
        if not torch.is_tensor(exclude) or exclude.shape != (N, N) or exclude.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"exclude must be a [{N},{N}] bool or uint8 tensor")
        if exclude.device != x.device:
            raise ValueError(f"exclude is on {exclude.device}, the structures on {x.device}")
        exclude = exclude.to(torch.uint8).contiguous()
    count = torch.empty(S, dtype=torch.int32, device=x.device)
    nearest = torch.empty(S, N, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().prd_quality_contacts(dptr(count, torch.int32), dptr(nearest), x.data_ptr(), xs, xr, dptr(a), dptr(b),
                                          dptr(exclude, torch.uint8), cutoff, S, N, stream()), "prd_quality_contacts")
    return Contacts(count, nearest)


def assess(pos, batch, ref=None, *, index: int = 0, num_atoms=None, num_residues=None, ref_has_ligand: bool = True,
           ca_clash: float = CA_CLASH, ligand_clash: float = LIGAND_CLASH, ligand_self_clash: float = LIGAND_SELF_CLASH,
           self_clash_min_bonds: int = SELF_CLASH_MIN_BONDS, bond_range=BOND_RANGE, ca_step: float = CA_STEP,
           ca_step_tolerance: float = CA_STEP_TOLERANCE, pocket: float = POCKET, lddt_radius: float = LDDT_RADIUS,
           lddt_pli_radius: float = LDDT_PLI_RADIUS) -> dict:
    """The named metrics of the samples ``pos`` [S,N,3] of ONE complex: complex ``index`` of the collated ``batch`` (the layout of
    ``pipeline.collate_fn`` / ``synthetic_batch``: ligand atoms in rows ``[0, na)``, residues in rows ``[na, na + nr)``, the bond-keyed
    tensors in the ``[0:na, 0:na]`` corner; the same rows ``generate_samples`` uses for its ``ca_mask``).  A residue counts where its
    C-alpha is marked in ``residue_atom_mask[:, :, 1]``.  ``num_atoms`` / ``num_residues``: na and nr as Python ints (default: read from
    the batch, which waits for the device when the batch lives there).  Returns a dict of device tensors.

    Without a reference:
      ``ca_clashes`` [S]            residue-residue pairs with C-alphas closer than ``ca_clash`` (3.0)
      ``ligand_clashes`` [S]        ligand-residue pairs closer than ``ligand_clash`` (2.5)
      ``ligand_self_clashes`` [S]   ligand-ligand pairs closer than ``ligand_self_clash`` (2.0) that are ``self_clash_min_bonds`` (4) or more
                                    bonds apart in ``bond_distance`` (one comparison makes the exclusion matrix)
      ``ligand_bond_outliers`` [S]  bonded pairs (``bond_distance == 1``, taken as symmetric) whose distance is not within ``bond_range``
                                    [0.9, 2.1): TWO ``contacts`` calls restricted to the bonded pairs -- bonds, minus those below 2.1,
                                    plus those below 0.9 -- because ``nearest`` sees one partner per atom and a count sees every bond.
                                    Both comparisons are the strict ``<`` of the census, hence the half-open interval.
      ``chain_breaks`` [S]          consecutive residues of one chain (``residue_index`` differing by 1, both C-alphas marked) whose
                                    C-alphas are not within ``ca_step`` +- ``ca_step_tolerance`` (3.8 +- 0.5); an O(N) comparison of
                                    shifted rows in plain torch
      ``pocket`` [S,N] (0 / 1, int32), ``pocket_size`` [S]   residues whose C-alpha lies within ``pocket`` (8) of any ligand atom of the sample
    With ``ref`` [N,3] (fp32, the same rows; ``ref_has_ligand=False``: its ligand rows hold no coordinates, the three metrics that
    need them are left out):
      ``lddt_ca`` [S], ``lddt_ca_per_residue`` [S,nr]   rows = columns = residues, radius ``lddt_radius`` (15)
      ``lddt_pli`` [S]              rows = ligand atoms, columns = residues, radius ``lddt_pli_radius`` (10).  The protein is a C-alpha
                                    trace here, so this is WIDER than the 6 Angstrom of the all-atom convention: a C-alpha is several
                                    Angstrom further from a ligand atom than the side chain that touches it
      ``lddt_ligand`` [S]           rows = columns = ligand atoms, radius ``lddt_radius``: conformer fidelity
      ``pocket_recall`` [S]         the share of the reference's pocket residues that are in the sample's pocket too (NaN without any)
    All of it is distances: a mirror image scores exactly like the original (see the head of this module), and so does a sample
    moved by any rigid transform, such as the one ``generate_samples(align_to=...)`` applies."""
    x, _, _ = _structures(pos, "pos")
    S, N = x.shape[:2]
    dev = x.device
    na = int(batch["num_atoms"][index]) if num_atoms is None else int(num_atoms)
    nr = int(batch["num_residues"][index]) if num_residues is None else int(num_residues)
    if na < 0 or nr < 0 or na + nr > N:
        raise ValueError(f"{na} ligand atoms and {nr} residues do not fit the {N} rows of pos")
    rows = torch.arange(N, device=dev)
    lig = (rows < na).float()
    ca = ((rows >= na) & (rows < na + nr) & (batch["residue_atom_mask"][index, :N, 1].to(dev) > 0.5))
    res = ca.float()
    bd = batch["bond_distance"][index, :N, :N].to(dev)
    out = {"ca_clashes": contacts(x, res, res, ca_clash).count,
           "ligand_clashes": contacts(x, lig, res, ligand_clash).count,
           "ligand_self_clashes": contacts(x, lig, lig, ligand_self_clash, exclude=bd < self_clash_min_bonds).count}
    bonded = bd == 1
    bonded[na:] = False
    bonded[:, na:] = False
    not_bonded = ~bonded
    n_bonds = bonded.triu(1).sum().to(torch.int32)
    out["ligand_bond_outliers"] = n_bonds - contacts(x, lig, lig, bond_range[1], exclude=not_bonded).count \
        + contacts(x, lig, lig, bond_range[0], exclude=not_bonded).count
    ri, ch = batch["residue_index"][index, :N].to(dev), batch["residue_chain_index"][index, :N].to(dev)
    step = ca[1:] & ca[:-1] & (ch[1:] == ch[:-1]) & (ri[1:] - ri[:-1] == 1)
    d = (x[:, 1:] - x[:, :-1]).norm(dim=-1)
    out["chain_breaks"] = (step & ((d - ca_step).abs() > ca_step_tolerance)).sum(1).to(torch.int32)
    in_pocket = contacts(x, res, lig, pocket).nearest < pocket
    out["pocket"] = in_pocket.to(torch.int32)
    out["pocket_size"] = in_pocket.sum(1).to(torch.int32)
    if ref is not None:
        if not torch.is_tensor(ref) or ref.shape != (N, 3):
            raise ValueError(f"ref must be a [{N},3] tensor over the same rows as pos, got {tuple(ref.shape) if torch.is_tensor(ref) else type(ref).__name__}")
        protein = lddt(x, ref, res, radius=lddt_radius)
        out["lddt_ca"] = protein.score
        out["lddt_ca_per_residue"] = protein.per_position[:, na: na + nr]
        if ref_has_ligand:
            out["lddt_pli"] = lddt(x, ref, lig, partner_mask=res, radius=lddt_pli_radius).score
            out["lddt_ligand"] = lddt(x, ref, lig, radius=lddt_radius).score
            ref_pocket = contacts(ref.unsqueeze(0), res, lig, pocket).nearest[0] < pocket
            out["pocket_recall"] = (in_pocket & ref_pocket).sum(1).double() / ref_pocket.sum().double()
    return out
