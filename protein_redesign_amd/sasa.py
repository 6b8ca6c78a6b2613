"""Solvent accessibility of all-atom backbones and their ligand on the device: ctypes binding of libprd_sasa.so (include/prd_sasa.h) and
the public functions on top of it -- ``count`` (Shrake and Rupley's point count of every atom of every sample; one launch), ``area``
(the counts as areas in float64), ``measure`` (the backbone atoms of ``backbone.build`` and the ligand rows as one set of atoms, counted
twice: in the complex, and every partner alone; per-residue burial, the ligand's covered surface and the interface from the two),
``sphere`` (the point set) and the host spec ``Accessibility``.

The definition is the header's: P points on every atom's sphere of radius van der Waals + probe, a point buried when it lies strictly
inside another atom's such sphere, the test made in the frame centred on the atom, in fp32 in a stated operation order.  The points are
the Fibonacci lattice  z_k = 1 - (2k + 1) / P,  phi_k = k pi (3 - sqrt 5),  computed in float64 and rounded once to fp32.

WHAT IS CLAIMED: the counts are that definition, deterministic (two calls give equal bits), and equal to the same definition evaluated
in float64 on every point whose margin |p - d_j|^2 - reach_j^2 is farther than 1e-4 Angstrom^2 from zero.  The areas are quotients of
those integers, formed in float64.  What is NOT: anything about real proteins.  The builder's carbonyl oxygen is off by up to 1.2
Angstrom off its anchor conformations, and there are no side chains beyond CB (CB takes part on every built residue; the decoded
sequence is not consulted), so the absolute areas are those of a poly-alanine-like model and OVERESTIMATE exposure; ``relative`` is
normalised by the same model's extended chain (``REFERENCE_AREA``) and is a ranking within a sample, not a measured burial.  A lattice of
P points has a quadrature error of its own (about 0.02 of a sphere's exposed fraction at P = 256).

The lattice is not mirror-symmetric: the mirror image of a structure gets nearly the same counts, but not the same bits.  Unlike the
other post-sampling modules, this one makes no bit-exact reflection claim.

Everything runs on the current stream with no host synchronisation.  HIP only: a missing library or a CPU tensor raises."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ._lib import SideLibrary, dptr, stream, structures

_BINDING = SideLibrary("sasa", 100, "at most {MAX_A} atoms per structure (PRD_SASA_MAX_A), {MAX_S} structures per call (PRD_SASA_MAX_S) and "
                                    "{MAX_P} points per atom (PRD_SASA_MAX_P), the points a multiple of 64")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version      # 100: include/prd_sasa.h PRD_SASA_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_P, MAX_A, MAX_S = _DEFINES["MAX_P"], _DEFINES["MAX_A"], _DEFINES["MAX_S"]
ALL, SAME_GROUP = _DEFINES["ALL"], _DEFINES["SAME_GROUP"]
ATOMS = ("N", "CA", "C", "CB", "O")             # backbone.ATOMS: the atom order of ``atoms`` and the bits of ``built``
ELEMENTS = 119                                  # constants.ATOM_FEATURE_CARDS[0]: index e is atomic number e + 1, the last index "other"
PROTEIN, LIGAND = 0, 1                          # the groups of ``measure``
SCALAR_COLUMNS = ("total_area", "interface_area", "ligand_buried_fraction", "buried_residues", "burial_agreement")
# The area in Angstrom^2 of the five atoms of the central residue of a three-residue ideal beta chain (backbone.ideal_chain, phi = -120,
# psi = 130 degrees), by the float64 yardstick at the default spec (points = 256): what ``relative`` divides by.
# tests/test_sasa_cpu.py recomputes it and requires equality.
REFERENCE_AREA = 111.6890949477322


def _f32(v):
    return float(np.float32(v))


def _number(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(float(v)):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    if not lo <= float(v) <= hi:
        raise ValueError(f"{name} must lie between {lo} and {hi}, got {v!r}")
    return float(v)


@dataclasses.dataclass(frozen=True)
class Radii:
    """Van der Waals radii in Angstrom.  ``backbone``: of N, CA, C, CB and O, in the order ``ATOMS`` (united atoms: the hydrogens are in
    them).  ``ligand``: (atomic number, radius) pairs (Bondi's values); ``other``: every other element, and the "other" class."""
    backbone: tuple = (1.65, 1.87, 1.76, 1.87, 1.40)
    ligand: tuple = ((1, 1.20), (6, 1.70), (7, 1.55), (8, 1.52), (9, 1.47), (15, 1.80), (16, 1.80), (17, 1.75), (35, 1.85), (53, 1.98))
    other: float = 1.80

    def __post_init__(self):
        try:
            backbone = tuple(self.backbone)
            ligand = tuple((z, r) for z, r in self.ligand)
        except (TypeError, ValueError):
            raise ValueError(f"radii: backbone must be five radii and ligand (atomic number, radius) pairs, got {self.backbone!r} and {self.ligand!r}") from None
        if len(backbone) != len(ATOMS):
            raise ValueError(f"radii: backbone must hold the five radii of {ATOMS}, got {self.backbone!r}")
        object.__setattr__(self, "backbone", tuple(_number(f"radius of {a}", r, 0.5, 3.0) for a, r in zip(ATOMS, backbone)))
        for z, _ in ligand:
            if isinstance(z, bool) or not isinstance(z, (int, np.integer)) or not 1 <= int(z) < ELEMENTS:
                raise ValueError(f"radii: an atomic number must be an integer between 1 and {ELEMENTS - 1}, got {z!r}")
        if len({int(z) for z, _ in ligand}) != len(ligand):
            raise ValueError(f"radii: an atomic number is listed twice in {self.ligand!r}")
        object.__setattr__(self, "ligand", tuple(sorted((int(z), _number(f"radius of element {z}", r, 0.5, 3.0)) for z, r in ligand)))
        object.__setattr__(self, "other", _number("radius of other elements", self.other, 0.5, 3.0))

    def by_element(self) -> np.ndarray:
        """[119] float64: the radius of every element index of ``atom_feats[..., 0]``"""
        t = np.full(ELEMENTS, self.other, np.float64)
        for z, r in self.ligand:
            t[z - 1] = r
        return t


@dataclasses.dataclass(frozen=True)
class Accessibility:
    """What ``measure`` and ``pipeline.generate_samples(accessibility=...)`` take: ``probe``, the radius in Angstrom of the solvent
    sphere rolled over the atoms; ``points``, the number P of lattice points per atom (a multiple of 64, at most 1024); ``radii``, a
    ``Radii``; ``buried_below``, the relative area under which a residue is called buried.  ``"measure"`` is shorthand for
    ``Accessibility()``."""
    probe: float = 1.4
    points: int = 256
    radii: Radii = Radii()
    buried_below: float = 0.2

    def __post_init__(self):
        object.__setattr__(self, "probe", _number("probe", self.probe, 0.0, 5.0))
        p = self.points
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or p <= 0 or p % 64 != 0 or p > MAX_P:
            raise ValueError(f"points must be a positive multiple of 64, at most {MAX_P} (PRD_SASA_MAX_P), got {p!r}")
        object.__setattr__(self, "points", int(p))
        if not isinstance(self.radii, Radii):
            raise ValueError(f"radii must be a sasa.Radii, got {type(self.radii).__name__}")
        object.__setattr__(self, "buried_below", _number("buried_below", self.buried_below, 0.0, 1.0))

    @staticmethod
    def of(value) -> "Accessibility":
        """the spec behind an ``accessibility=`` argument: an Accessibility or ``"measure"``; TypeError / ValueError otherwise"""
        if isinstance(value, Accessibility):
            return value
        if isinstance(value, str):
            if value != "measure":
                raise ValueError(f"accessibility must be None, 'measure' or a sasa.Accessibility, got {value!r}")
            return Accessibility()
        raise TypeError(f"accessibility must be None, 'measure' or a sasa.Accessibility, got {type(value).__name__}")

    def reaches(self) -> tuple:
        """(backbone [5], by element [119]): radius + probe, float64 on the host rounded once to fp32, checked finite and positive"""
        bb = (np.asarray(self.radii.backbone, np.float64) + self.probe).astype(np.float32)
        el = (self.radii.by_element() + self.probe).astype(np.float32)
        check_reach(bb), check_reach(el)
        return bb, el

    def describe(self) -> dict:
        return {"probe": np.float64(self.probe), "points": np.int64(self.points), "buried_below": np.float64(self.buried_below),
                "backbone_radii": np.asarray(self.radii.backbone), "ligand_radii": self.radii.by_element(), "reference_area": np.float64(REFERENCE_AREA)}


def check_reach(reach) -> np.ndarray:
    """``reach`` (host values) as float32, or ValueError: the launch requires every reach finite and not negative (prd_sasa.h)"""
    r = np.array(reach, np.float32)                 # a copy: the caller's values may be read-only
    if r.ndim != 1 or not np.isfinite(r).all() or (r < 0).any():
        raise ValueError("reach must be a [A] sequence of finite radii that are not negative")
    return r


def sphere(P: int) -> np.ndarray:
    """[P,3] float32 unit vectors: the Fibonacci lattice z_k = 1 - (2k + 1) / P, phi_k = k pi (3 - sqrt 5), float64 rounded once"""
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or P <= 0:
        raise ValueError(f"the number of points must be a positive integer, got {P!r}")
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    r, phi = np.sqrt(1.0 - z * z), k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)


@dataclasses.dataclass(frozen=True)
class Uploaded:
    """A spec with its point set and its reach tables on a device.  Made by ``upload``."""
    spec: Accessibility
    sphere: torch.Tensor            # [P,3] float32
    backbone: torch.Tensor          # [5] float32: reach of N, CA, C, CB, O
    by_element: torch.Tensor        # [119] float32: reach of a ligand atom by its element index


_UPLOADED, _SPHERES = {}, {}


def _device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def sphere_on(P: int, device) -> torch.Tensor:
    """``sphere(P)`` on ``device``, made once per P and device and kept; the copy waits for the host"""
    key = (int(P), str(_device(device)))
    if key not in _SPHERES:
        _SPHERES[key] = torch.from_numpy(sphere(P)).to(_device(device))
    return _SPHERES[key]


def upload(spec="measure", device="cuda") -> Uploaded:
    """``spec`` with its tables on ``device``, made once per spec and device and kept.  The copies wait for the host: call this outside a
    captured or synchronisation-free region and hand the result (or the same spec) to ``measure``."""
    spec, device = Accessibility.of(spec), _device(device)
    key = (spec, str(device))
    if key not in _UPLOADED:
        bb, el = spec.reaches()
        _UPLOADED[key] = Uploaded(spec, sphere_on(spec.points, device), torch.from_numpy(bb).to(device), torch.from_numpy(el).to(device))
    return _UPLOADED[key]


def _ints(t, name, shape, device):
    if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != device:
        raise ValueError(f"{name} must be a {list(shape)} int32 tensor on {device}, got "
                         f"{(tuple(t.shape), t.dtype, str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    return t.contiguous()


def count(pos, reach, present, group=None, mode=ALL, points=256) -> torch.Tensor:
    """[S,A] int32: of the ``points`` lattice points of every atom, those that no other atom buries (prd_sasa.h).  ``pos`` [S,A,3] fp32 on
    the device (a strided view is taken as it is); ``reach`` [A] fp32, radius + probe of every atom -- a device tensor is taken as
    checked where it was built (``check_reach``), host values are checked and uploaded here, and that copy waits for the host;
    ``present`` [S,A] int32, 0 where the atom does not exist in that sample (its coordinates may then be anything); ``group`` [A] int32
    or None; ``mode``: ``ALL``, or ``SAME_GROUP`` -- only atoms of the atom's own group bury.  ``points``: a multiple of 64, at most
    1024, or a [P,3] device tensor of unit vectors of the caller's own.  One launch, no host synchronisation, capturable."""
    pos, ss, sa = structures(pos, "pos", runs="the accessibility count runs", letter="S")
    S, A = pos.shape[:2]
    if S > 1 and ss < (A - 1) * sa + 3:
        pos = pos.contiguous()
        ss, sa = pos.stride(0), pos.stride(1)
    if mode not in (ALL, SAME_GROUP):
        raise ValueError(f"mode must be sasa.ALL ({ALL}) or sasa.SAME_GROUP ({SAME_GROUP}), got {mode!r}")
    if mode == SAME_GROUP and group is None:
        raise ValueError("mode SAME_GROUP needs the group of every atom")
    if not torch.is_tensor(reach) or not reach.is_cuda:
        reach = torch.from_numpy(check_reach(reach.numpy() if torch.is_tensor(reach) else reach)).to(pos.device)
    if tuple(reach.shape) != (A,) or reach.dtype != torch.float32 or reach.device != pos.device:
        raise ValueError(f"reach must be a [{A}] float32 tensor on {pos.device}, got {(tuple(reach.shape), reach.dtype, str(reach.device))}")
    present = _ints(present, "present", (S, A), pos.device)
    group = None if group is None else _ints(group, "group", (A,), pos.device)
    dirs = points if torch.is_tensor(points) else sphere_on(points, pos.device)
    if dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.dtype != torch.float32 or dirs.device != pos.device:
        raise ValueError(f"points must be a number or a [P,3] float32 tensor on {pos.device}, got {(tuple(dirs.shape), dirs.dtype, str(dirs.device))}")
    P = dirs.shape[0]
    if A > MAX_A or S > MAX_S or P > MAX_P or P % 64 != 0:
        raise ValueError(f"pos: {S} structures of {A} atoms with {P} points each; {_BINDING.limit}")
    out = torch.empty(S, A, dtype=torch.int32, device=pos.device)
    with torch.cuda.device(pos.device):
        _check(lib().prd_sasa_count(dptr(out, torch.int32), pos.data_ptr(), ss, sa, dptr(reach.contiguous()), dptr(present, torch.int32),
                                    dptr(group, torch.int32), dptr(dirs.contiguous()), mode, S, A, P, stream()), "prd_sasa_count")
    return out


def area(count, reach, P):
    """4 pi reach^2 count / P in float64, Angstrom^2: ``count`` [..., A] integers, ``reach`` [A]; tensors give a tensor, arrays an array"""
    if torch.is_tensor(count):
        return count.to(torch.float64) * (reach.to(torch.float64) ** 2 * (4.0 * math.pi / P))
    return np.asarray(count, np.float64) * (np.asarray(reach, np.float64) ** 2 * (4.0 * math.pi / P))


def flatten(atoms, built, ligand_pos, ligand_elements, mask, up: Uploaded):
    """The atoms of ``measure`` as one set: (pos [S,A,3], reach [A], present [S,A] int32, group [A] int32), A = 5 nr + na -- the five
    atoms of every residue in the order ``ATOMS``, then the ligand atoms.  Plain torch, no synchronisation."""
    S, nr = atoms.shape[:2]
    na = ligand_pos.shape[1]
    dev = atoms.device
    pos = torch.cat([atoms.reshape(S, nr * 5, 3), ligand_pos.to(torch.float32)], 1)
    bits = (built.unsqueeze(-1) >> torch.arange(5, device=dev, dtype=torch.int32)) & 1                   # [S,nr,5]
    if mask is not None:
        bits = bits * (mask > 0.5).to(torch.int32)[None, :, None]
    present = torch.cat([bits.reshape(S, nr * 5).to(torch.int32), torch.ones(S, na, dtype=torch.int32, device=dev)], 1)
    reach = torch.cat([up.backbone.repeat(nr), up.by_element[ligand_elements.to(torch.int64).clamp(0, ELEMENTS - 1)]])
    group = torch.cat([torch.full((nr * 5,), PROTEIN, dtype=torch.int32, device=dev), torch.full((na,), LIGAND, dtype=torch.int32, device=dev)])
    return pos.contiguous(), reach.contiguous(), present.contiguous(), group


def measure(atoms, built, ligand_pos, ligand_elements, mask=None, spec=None) -> dict:
    """Burial of every residue and the protein-ligand interface of every sample.  ``atoms`` [S,nr,5,3] fp32 and ``built`` [S,nr] int32 as
    ``backbone.build`` returns them, over the residue rows; ``ligand_pos`` [S,na,3] fp32 and ``ligand_elements`` [na] (element indices,
    ``atom_feats[..., 0]``), na = 0 allowed; ``mask`` [nr] fp32 0 / 1 or None: the residues that exist.  ``spec``: an ``Accessibility``,
    ``"measure"`` / None for the default, or an ``Uploaded`` from ``upload`` -- a spec that has not been uploaded to the device of
    ``atoms`` yet is uploaded here, and those copies wait for the host.  Every atom whose bit of ``built`` is set takes part with its own
    radius: a residue that kept its C-alpha alone contributes that C-alpha, and CB takes part on every built residue (the decoded
    sequence is not consulted).  Two launches -- the complex (``ALL``), then every partner alone (``SAME_GROUP``, the protein group 0,
    the ligand group 1) -- and plain torch, no host synchronisation.  Returns device tensors, areas in float64 Angstrom^2:
    ``atom_area`` [S,nr,5], ``residue_area``, ``relative`` (residue_area / REFERENCE_AREA), ``buried`` (relative < buried_below, of
    residues with a C-alpha) and ``complete`` (N, CA, C and O present), each [S,nr]; ``ligand_area`` and ``ligand_area_free`` [S,na]
    (in the complex / alone); ``ligand_buried_fraction`` [S] (the share of the free ligand's area the protein covers; NaN without a
    ligand); ``interface_area`` [S] (what protein and ligand lose on complexation, summed); ``interface_residues`` [S,nr] (residues that
    lose area to the ligand); ``total_area`` [S] (of the complex); ``buried_residues`` [S]."""
    if not torch.is_tensor(atoms) or atoms.dim() != 4 or tuple(atoms.shape[2:]) != (5, 3) or atoms.shape[0] < 1 or atoms.shape[1] < 1:
        raise ValueError(f"atoms must be a [S,nr,5,3] tensor, got {tuple(atoms.shape) if torch.is_tensor(atoms) else type(atoms).__name__}")
    if atoms.dtype != torch.float32:
        raise ValueError(f"atoms must be float32, got {atoms.dtype}")
    S, nr = atoms.shape[:2]
    if not torch.is_tensor(built) or tuple(built.shape) != (S, nr) or built.dtype != torch.int32 or built.device != atoms.device:
        raise ValueError(f"built must be a [{S},{nr}] int32 tensor on {atoms.device}, got "
                         f"{(tuple(built.shape), built.dtype, str(built.device)) if torch.is_tensor(built) else type(built).__name__}")
    if not torch.is_tensor(ligand_pos) or ligand_pos.dim() != 3 or ligand_pos.shape[0] != S or ligand_pos.shape[2] != 3 or ligand_pos.device != atoms.device:
        raise ValueError(f"ligand_pos must be a [{S},na,3] tensor on {atoms.device}, got "
                         f"{(tuple(ligand_pos.shape), str(ligand_pos.device)) if torch.is_tensor(ligand_pos) else type(ligand_pos).__name__}")
    na = ligand_pos.shape[1]
    if not torch.is_tensor(ligand_elements) or tuple(ligand_elements.shape) != (na,) or ligand_elements.device != atoms.device:
        raise ValueError(f"ligand_elements must be a [{na}] tensor of element indices on {atoms.device}")
    if mask is not None and (not torch.is_tensor(mask) or tuple(mask.shape) != (nr,) or mask.device != atoms.device):
        raise ValueError(f"mask must be a [{nr}] tensor on {atoms.device}")
    up = spec if isinstance(spec, Uploaded) else upload("measure" if spec is None else spec, atoms.device)
    if up.sphere.device != atoms.device:
        raise ValueError(f"the tables are on {up.sphere.device}, the structures on {atoms.device}")
    spec, P = up.spec, up.spec.points
    pos, reach, present, group = flatten(atoms, built, ligand_pos, ligand_elements, mask, up)
    bound = area(count(pos, reach, present, None, ALL, up.sphere), reach, P)                  # [S,A]: in the complex
    free = area(count(pos, reach, present, group, SAME_GROUP, up.sphere), reach, P)           # every partner alone
    n5 = nr * 5
    atom_area = bound[:, :n5].reshape(S, nr, 5)
    residue_area, residue_free = atom_area.sum(2), free[:, :n5].reshape(S, nr, 5).sum(2)
    bits = present[:, :n5].reshape(S, nr, 5) != 0
    relative = residue_area / REFERENCE_AREA
    buried = (relative < spec.buried_below) & bits[:, :, 1]
    lig, lig_free = bound[:, n5:], free[:, n5:]
    lig_total = lig_free.sum(1)
    covered = torch.where(lig_total > 0, 1.0 - lig.sum(1) / lig_total.clamp(min=1e-300), torch.full_like(lig_total, float("nan")))
    return {"atom_area": atom_area, "residue_area": residue_area, "relative": relative, "buried": buried,
            "complete": bits[:, :, 0] & bits[:, :, 1] & bits[:, :, 2] & bits[:, :, 4], "ligand_area": lig, "ligand_area_free": lig_free,
            "ligand_buried_fraction": covered, "interface_area": (residue_free - residue_area).sum(1) + (lig_free - lig).sum(1),
            "interface_residues": residue_free > residue_area, "total_area": bound.sum(1), "buried_residues": buried.sum(1)}
