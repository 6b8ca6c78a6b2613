"""Secondary structure of all-atom backbones on the device: ctypes binding of libprd_dssp.so (include/prd_dssp.h) and the public
functions on top of it -- ``hbonds`` (the Kabsch-Sander hydrogen-bond energy between every C=O and every N-H of every sample, the two
best partners of every residue in either role; one launch), ``assign`` (the same, then the eight DSSP classes read off the bond
pattern: turns, helices, bridges, ladders, bends; two more launches), ``census`` (counts and fractions per sample, plain torch),
``strings`` / ``three_state`` (the classes as text and as helix / strand / other) and the host spec ``Dssp``.

The inputs are the outputs of ``backbone.build`` as they are -- ``atoms`` [S,N,5,3] in the order N, CA, C, CB, O, ``built`` [S,N] and
the caller's ``link`` [N] -- or any all-atom structure in that layout.  The definition is the header's, including its three stated
deviations from DSSP proper (the mutual two-best rule for a bond, no beta-bulge merging, no sheet labels).

Every quantity here is a function of distances, so a mirror image is assigned exactly like the original: a left-handed helix is an H
like a right-handed one.  Handedness is ``chirality``'s business.

WHAT IS CLAIMED: the launches compute the definitions of the header to fp32 accuracy, deterministically; on the backbone built from an
ideal alpha-helical C-alpha trace the interior is H, and on a 3-10 trace it is G, end to end.  What is NOT: any accuracy on real
proteins.  The builder's carbonyl oxygen is off by up to 1.2 Angstrom off its anchor conformations, so the strand pairing found on
BUILT atoms is expected to be fragile; on true atoms the ladders are found.

Everything runs on the current stream with no host synchronisation.  HIP only: a missing library or a CPU tensor raises."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ._lib import SideLibrary, dptr, position_mask as _mask, stream

_BINDING = SideLibrary("dssp", 100, "at most {MAX_N} positions per structure (PRD_DSSP_MAX_N) and {MAX_S} structures per call (PRD_DSSP_MAX_S)")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version      # 100: include/prd_dssp.h PRD_DSSP_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_N, MAX_S, TILE, HALO = _DEFINES["MAX_N"], _DEFINES["MAX_S"], _DEFINES["TILE"], _DEFINES["HALO"]
ALPHABET = "-HBEGITS"                           # the class codes 0 .. 7
HELIX, STRAND = (1, 4, 5), (2, 3)               # three_state: H, G, I / B, E
FLAG_TURN3, FLAG_LADDER, FLAG_BEND = _DEFINES["FLAG_TURN3"], _DEFINES["FLAG_LADDER"], _DEFINES["FLAG_BEND"]
FLAG_BRIDGE = (_DEFINES["FLAG_PAR0"], _DEFINES["FLAG_ANTI0"], _DEFINES["FLAG_PAR1"], _DEFINES["FLAG_ANTI1"])


def _f32(v):
    return float(np.float32(v))


@dataclasses.dataclass(frozen=True)
class Dssp:
    """What ``hbonds``, ``assign`` and ``pipeline.generate_samples(secondary=...)`` take: ``cutoff``, the energy in kcal/mol below which
    a pair is a hydrogen bond; ``bend``, the angle in degrees between CA(r) - CA(r-2) and CA(r+2) - CA(r) above which residue r is a
    bend; ``coupling``, the factor q of the energy (0.084 x 332); ``floor``, the least energy a pair may have.  ``"assign"`` is shorthand
    for ``Dssp()``."""
    cutoff: float = -0.5
    bend: float = 70.0
    coupling: float = 27.888
    floor: float = -9.9

    def __post_init__(self):
        for name in ("cutoff", "bend", "coupling", "floor"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(float(v)):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        if not self.cutoff < 0.0:
            raise ValueError(f"cutoff must be a negative energy in kcal/mol, got {self.cutoff!r}")
        if not self.floor < self.cutoff:
            raise ValueError(f"floor must lie below cutoff ({self.cutoff}), got {self.floor!r}")
        if not self.coupling > 0.0:
            raise ValueError(f"coupling must be positive, got {self.coupling!r}")
        if not 0.0 < self.bend < 180.0:
            raise ValueError(f"bend must be an angle in degrees between 0 and 180, got {self.bend!r}")

    @staticmethod
    def of(value) -> "Dssp":
        """the spec behind a ``secondary=`` argument: a Dssp or ``"assign"``; TypeError / ValueError otherwise"""
        if isinstance(value, Dssp):
            return value
        if isinstance(value, str):
            if value != "assign":
                raise ValueError(f"secondary must be None, 'assign' or a dssp.Dssp, got {value!r}")
            return Dssp()
        raise TypeError(f"secondary must be None, 'assign' or a dssp.Dssp, got {type(value).__name__}")

    def scalars(self) -> tuple:
        """(q, e_min, cutoff, cos_bend): the scalar arguments of the launches, float64 on the host rounded once to fp32"""
        return _f32(self.coupling), _f32(self.floor), _f32(self.cutoff), _f32(math.cos(math.radians(self.bend)))

    def describe(self) -> dict:
        return {"cutoff": np.float64(self.cutoff), "bend": np.float64(self.bend), "coupling": np.float64(self.coupling), "floor": np.float64(self.floor)}


@dataclasses.dataclass(frozen=True)
class Hbonds:
    """Device tensors, as the launch wrote them (prd_dssp.h)."""
    partner: torch.Tensor           # [S,N,4] int32: the two best acceptors of a residue as donor, then its two best donors as acceptor; -1: none
    energy: torch.Tensor            # [S,N,4] float32 kcal/mol, 0 for an empty slot


@dataclasses.dataclass(frozen=True)
class Assigned:
    """Device tensors, as the launches wrote them (prd_dssp.h)."""
    classes: torch.Tensor           # [S,N] uint8: codes into ALPHABET
    flags: torch.Tensor             # [S,N] int32: the turn, bridge-type, ladder and bend bits
    bridge: torch.Tensor            # [S,N,2] int32: the two lowest bridge partner rows, -1 for none
    partner: torch.Tensor           # [S,N,4] int32
    energy: torch.Tensor            # [S,N,4] float32


def _inputs(atoms, built, link, donor):
    if not torch.is_tensor(atoms) or atoms.dim() != 4 or tuple(atoms.shape[2:]) != (5, 3) or atoms.shape[0] < 1 or atoms.shape[1] < 1:
        raise ValueError(f"atoms must be a [S,N,5,3] tensor, got {tuple(atoms.shape) if torch.is_tensor(atoms) else type(atoms).__name__}")
    if atoms.dtype != torch.float32:
        raise ValueError(f"atoms must be float32, got {atoms.dtype}")
    if not atoms.is_cuda:
        raise RuntimeError("atoms: the secondary-structure assignment runs on the GPU only (got a CPU tensor); there is no CPU fallback")
    S, N = atoms.shape[:2]
    if N > MAX_N or S > MAX_S:
        raise ValueError(f"atoms: {S} structures of {N} positions, at most {MAX_S} structures (PRD_DSSP_MAX_S) of {MAX_N} positions "
                         f"(PRD_DSSP_MAX_N) are supported")
    if not torch.is_tensor(built) or tuple(built.shape) != (S, N) or built.dtype != torch.int32 or built.device != atoms.device:
        raise ValueError(f"built must be a [{S},{N}] int32 tensor on {atoms.device}, got "
                         f"{(tuple(built.shape), built.dtype, str(built.device)) if torch.is_tensor(built) else type(built).__name__}")
    links = _mask(link, "link", N, atoms.device)
    donors = None if donor is None else _mask(donor, "donor", N, atoms.device)
    return atoms.contiguous(), built.contiguous(), links, donors, S, N


def hbonds(atoms, built, link, donor=None, spec=None) -> Hbonds:
    """The two best hydrogen-bond partners of every residue in either role.  ``atoms`` [S,N,5,3] fp32 and ``built`` [S,N] int32 as
    ``backbone.build`` returns them (on the device), ``link`` [N] fp32 as it took it; ``donor`` [N] fp32 0 / 1, or None: every residue
    may donate (clear it for proline).  ``spec``: a ``Dssp``, ``"assign"`` / None for the default.  One launch, no host
    synchronisation, capturable."""
    spec = Dssp.of("assign" if spec is None else spec)
    atoms, built, links, donors, S, N = _inputs(atoms, built, link, donor)
    q, e_min, _, _ = spec.scalars()
    partner = torch.empty(S, N, 4, dtype=torch.int32, device=atoms.device)
    energy = torch.empty(S, N, 4, dtype=torch.float32, device=atoms.device)
    with torch.cuda.device(atoms.device):
        _check(lib().prd_dssp_hbonds(dptr(partner, torch.int32), dptr(energy), dptr(atoms), dptr(built, torch.int32), dptr(links), dptr(donors),
                                     q, e_min, S, N, stream()), "prd_dssp_hbonds")
    return Hbonds(partner, energy)


def assign(atoms, built, link, donor=None, spec=None) -> Assigned:
    """``hbonds``, then the DSSP classes of every residue (prd_dssp.h): three launches on the current stream, no host synchronisation,
    capturable.  Arguments as ``hbonds`` takes them."""
    spec = Dssp.of("assign" if spec is None else spec)
    hb = hbonds(atoms, built, link, donor, spec)
    atoms, built, links, _, S, N = _inputs(atoms, built, link, None)
    _, _, cutoff, cos_bend = spec.scalars()
    classes = torch.empty(S, N, dtype=torch.uint8, device=atoms.device)
    flags = torch.empty(S, N, dtype=torch.int32, device=atoms.device)
    bridge = torch.empty(S, N, 2, dtype=torch.int32, device=atoms.device)
    with torch.cuda.device(atoms.device):
        _check(lib().prd_dssp_assign(dptr(classes, torch.uint8), dptr(flags, torch.int32), dptr(bridge, torch.int32), dptr(hb.partner, torch.int32),
                                     dptr(hb.energy), dptr(atoms), dptr(built, torch.int32), dptr(links), cutoff, cos_bend, S, N, stream()),
               "prd_dssp_assign")
    return Assigned(classes, flags, bridge, hb.partner, hb.energy)


def three_state(classes):
    """0 other, 1 helix (H, G, I), 2 strand (B, E), elementwise, of a tensor or an array of class codes; the same kind comes back"""
    c = classes
    helix = (c == HELIX[0]) | (c == HELIX[1]) | (c == HELIX[2])
    strand = (c == STRAND[0]) | (c == STRAND[1])
    if torch.is_tensor(c):
        return helix.to(torch.uint8) + 2 * strand.to(torch.uint8)
    return helix.astype(np.uint8) + 2 * strand.astype(np.uint8)


def census(assigned: Assigned, mask, spec=None) -> dict:
    """Per sample, over the rows ``mask`` [N] marks (fp32 0 / 1, on the tensors' device): ``counts`` [S,8] (how many rows carry each
    class of ALPHABET), ``helix_fraction`` (H, G and I) and ``strand_fraction`` (E and B) of those rows, and ``hbonds`` [S], the bonds
    below the spec's cutoff counted from their donors.  Plain torch operations on the current stream: no kernel of this library, no
    host synchronisation."""
    spec = Dssp.of("assign" if spec is None else spec)
    rows = (mask > 0.5).unsqueeze(0)                                                         # [1,N]
    c = assigned.classes.to(torch.int64)
    counts = torch.stack([((c == k) & rows).sum(1) for k in range(len(ALPHABET))], 1)         # [S,8]
    total = rows.sum().clamp(min=1).to(torch.float32)
    three = three_state(assigned.classes)
    bonded = (assigned.partner[:, :, :2] >= 0) & (assigned.energy[:, :, :2] < spec.scalars()[2]) & rows.unsqueeze(-1)
    return {"counts": counts, "helix_fraction": ((three == 1) & rows).sum(1) / total, "strand_fraction": ((three == 2) & rows).sum(1) / total,
            "hbonds": bonded.sum((1, 2))}


def strings(classes) -> list:
    """one str of ALPHABET letters per structure, on the host: ``classes`` [S,N] as a tensor (copied to the host here) or an array"""
    c = classes.cpu().numpy() if torch.is_tensor(classes) else np.asarray(classes)
    if c.ndim != 2:
        raise ValueError(f"classes must be [S,N], got {c.shape}")
    letters = np.array(list(ALPHABET))
    return ["".join(letters[row]) for row in c.astype(np.int64)]
