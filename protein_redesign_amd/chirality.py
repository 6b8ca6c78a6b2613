"""Which hand a generated sample has, read off the sample itself on the device: ctypes binding of libprd_chirality.so
(include/prd_chirality.h) and the public functions on top of it -- ``census`` (the local handedness of the C-alpha trace and of the
ligand's stereocentres, with a verdict per sample), ``reflect`` / ``fix`` (the exact reflection of the samples judged mirrored) and the
host helpers that lay a collated batch out for them (``trace_links``, ``ligand_centres``, ``centre_reference``).

The denoiser is equivariant under reflections, so a sample is as likely to be the mirror image of a protein as the right way round, and
the mirror image of a sample is an equally valid sample.  ``quality.py`` cannot see the difference (distances only) and
``alignment["mirrored"]`` needs a reference structure; this module needs neither.  The evidence is local: the virtual dihedral of four
consecutive C-alphas is about +50 degrees in a right-handed alpha-helix and about -50 in its mirror image, strands twist the other
way, and the signed volume at a tetrahedral centre of the ligand changes sign under reflection.

WHAT IS CLAIMED: the launches compute the definitions of the header, exactly antisymmetric under reflection and deterministic.  What is
NOT: how often a real sample is decided, or whether the default windows and vote minima are well chosen -- they sit round the literature
peaks of the C-alpha virtual geometry and were fitted to nothing.

Everything runs on the current stream with no host synchronisation.  HIP only: a missing library or a CPU tensor raises."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from ._lib import SideLibrary, dptr, position_mask as _mask, stream, structures

_BINDING = SideLibrary("chirality", 100, "at most {MAX_N} positions per structure (PRD_CHIRALITY_MAX_N), {MAX_S} structures per call and "
                                         "{MAX_C} ligand centres (PRD_CHIRALITY_MAX_C)")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version      # 100: include/prd_chirality.h PRD_CHIRALITY_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_N, MAX_S, MAX_C = _DEFINES["MAX_N"], _DEFINES["MAX_S"], _DEFINES["MAX_C"]
_structures = functools.partial(structures, runs="the handedness census runs", letter="S", bounds=_BINDING)
BASIS = {_DEFINES["BASIS_NONE"]: "none", _DEFINES["BASIS_HELIX"]: "helix", _DEFINES["BASIS_CENTRES"]: "centres", _DEFINES["BASIS_EXTENDED"]: "extended"}
COUNT_COLUMNS = ("helix_right", "helix_left", "extended_native", "extended_mirror", "quads", "centres_kept", "centres_inverted", "centres_flat")
MIRROR_COLUMNS = (1, 0, 3, 2, 4, 6, 5, 7)       # counts[:, MIRROR_COLUMNS] is the census of the mirror image
# the column order of sample_handedness.txt, and what generate_samples calls the three centre counts in its dict
TEXT_COLUMNS = ("verdict", "basis", "flipped") + COUNT_COLUMNS
RESULT_NAMES = {"centres_kept": "ligand_kept", "centres_inverted": "ligand_inverted", "centres_flat": "ligand_flat"}
BOND, VMIN, MIN_HELIX, MIN_EXTENDED = (3.3, 4.3), 0.5, 4, 12     # Angstrom (quality.CA_STEP +- CA_STEP_TOLERANCE), Angstrom^3, votes


def _window(pair, name, least, most):
    try:
        lo, hi = (float(v) for v in pair)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a (lo, hi) pair of degrees, got {pair!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and least <= lo < hi <= most):
        raise ValueError(f"{name} must be a window {least} <= lo < hi <= {most} of degrees, got ({lo}, {hi})")
    return lo, hi


def _f32(v):
    return float(np.float32(v))


@dataclasses.dataclass(frozen=True)
class Windows:
    """The class windows of a trace quad in degrees, all edges strict: the angles at the two inner C-alphas and the MAGNITUDE of the
    virtual dihedral.  Right helical: theta in ``helix_theta`` and tau in +``helix_tau``; left helical: -``helix_tau``; extended with
    the native twist: theta in ``extended_theta`` and tau in -``extended_tau``; with the mirror twist: +``extended_tau``."""
    helix_theta: tuple = (75.0, 110.0)
    helix_tau: tuple = (30.0, 80.0)
    extended_theta: tuple = (105.0, 150.0)
    extended_tau: tuple = (120.0, 180.0)

    def __post_init__(self):
        for name in ("helix_theta", "helix_tau", "extended_theta", "extended_tau"):
            object.__setattr__(self, name, _window(getattr(self, name), name, 0.0, 180.0))

    def edges(self):
        """the eight arguments of the launch: per class the cosine window of theta (cos hi, cos lo) and the tau window in radians, each
        computed in float64 and rounded once to fp32"""
        out = []
        for theta, tau in ((self.helix_theta, self.helix_tau), (self.extended_theta, self.extended_tau)):
            out += [_f32(math.cos(math.radians(theta[1]))), _f32(math.cos(math.radians(theta[0]))), _f32(math.radians(tau[0])), _f32(math.radians(tau[1]))]
        return tuple(out)


def _thresholds(bond, vmin, min_helix, min_extended):
    try:
        lo, hi = (float(v) for v in bond)
    except (TypeError, ValueError):
        raise ValueError(f"bond must be a (lo, hi) pair of Angstrom, got {bond!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError(f"bond must be a window 0 < lo < hi of Angstrom, got ({lo}, {hi})")
    vmin = float(vmin)
    if not (math.isfinite(vmin) and vmin > 0.0):
        raise ValueError(f"vmin must be a positive, finite volume in Angstrom^3, got {vmin!r}")
    for name, v in (("min_helix", min_helix), ("min_extended", min_extended)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"{name} must be a non-negative int, got {v!r}")
    return (lo, hi), vmin, int(min_helix), int(min_extended)


@dataclasses.dataclass(frozen=True)
class Handedness:
    """What ``pipeline.generate_samples(handedness=...)`` takes: the thresholds of ``census`` and whether the samples judged mirrored are
    reflected (``fix``).  ``"report"`` and ``"fix"`` are shorthands for ``Handedness()`` and ``Handedness(fix=True)``."""
    fix: bool = False
    windows: Windows = Windows()
    bond: tuple = BOND
    vmin: float = VMIN
    min_helix: int = MIN_HELIX
    min_extended: int = MIN_EXTENDED

    def __post_init__(self):
        if not isinstance(self.fix, bool):
            raise ValueError(f"fix must be a bool, got {self.fix!r}")
        if not isinstance(self.windows, Windows):
            raise ValueError(f"windows must be a chirality.Windows, got {type(self.windows).__name__}")
        bond, vmin, mh, me = _thresholds(self.bond, self.vmin, self.min_helix, self.min_extended)
        for name, v in (("bond", bond), ("vmin", vmin), ("min_helix", mh), ("min_extended", me)):
            object.__setattr__(self, name, v)

    @staticmethod
    def of(value) -> "Handedness":
        """the spec behind a ``handedness=`` argument: a Handedness, ``"report"`` or ``"fix"``; TypeError / ValueError otherwise"""
        if isinstance(value, Handedness):
            return value
        if isinstance(value, str):
            if value not in ("report", "fix"):
                raise ValueError(f"handedness must be None, 'report', 'fix' or a chirality.Handedness, got {value!r}")
            return Handedness(fix=value == "fix")
        raise TypeError(f"handedness must be None, 'report', 'fix' or a chirality.Handedness, got {type(value).__name__}")

    def thresholds(self) -> dict:
        return dict(windows=self.windows, bond=self.bond, vmin=self.vmin, min_helix=self.min_helix, min_extended=self.min_extended)


@dataclasses.dataclass(frozen=True)
class Centres:
    """The ligand's centre list in both places the library wants it (prd_chirality.h, "who validates the rows"): ``host`` [C,4] int32 on
    the CPU, which the call checks against N before it launches, and ``device``, the copy the kernel reads.  Made by ``upload``."""
    host: torch.Tensor
    device: torch.Tensor


def upload(centres, device) -> Centres:
    """``centres`` ([C,4] int32 / int64 rows (c, n1, n2, n3), a CPU tensor or an array) with its copy on ``device``.  The copy waits for
    the host: make it once, outside a captured or synchronisation-free region, and hand the result to ``census``."""
    host = torch.as_tensor(np.asarray(centres.cpu() if torch.is_tensor(centres) else centres)).to(torch.int32).reshape(-1, 4).contiguous()
    if host.shape[0] > MAX_C:
        raise ValueError(f"{host.shape[0]} ligand centres, at most {MAX_C} (PRD_CHIRALITY_MAX_C) are supported")
    return Centres(host, host.to(device))


@dataclasses.dataclass(frozen=True)
class Census:
    """Device tensors, as the launch wrote them (prd_chirality.h)."""
    counts: torch.Tensor            # [S,8] int32, columns COUNT_COLUMNS
    verdict: torch.Tensor           # [S] int32: +1 natural hand, -1 mirror image, 0 undecided
    basis: torch.Tensor             # [S] int32: the rule that decided, BASIS names them
    tau: torch.Tensor               # [S,N] float32 radians, NaN where a row starts no quad
    classes: torch.Tensor           # [S,N] int32: 1 right helical, 2 left helical, 3 extended native, 4 extended mirror, 0 none
    volume: torch.Tensor            # [S,C] float32 Angstrom^3

    def __getattr__(self, name):    # helix_right ... centres_flat: the columns of counts
        if name in COUNT_COLUMNS:
            return self.counts[:, COUNT_COLUMNS.index(name)]
        raise AttributeError(name)

    @property
    def helix_fraction(self):
        """[S] float64: the helical quads of either hand over the quads; NaN without a quad"""
        return (self.counts[:, 0] + self.counts[:, 1]).double() / self.counts[:, 4].double()

    @property
    def extended_fraction(self):
        """[S] float64: the extended quads of either twist over the quads; NaN without a quad"""
        return (self.counts[:, 2] + self.counts[:, 3]).double() / self.counts[:, 4].double()


def census(x, mask, link, *, centres=None, centre_ref=None, windows: Windows = Windows(), bond=BOND, vmin: float = VMIN,
           min_helix: int = MIN_HELIX, min_extended: int = MIN_EXTENDED) -> Census:
    """The handedness census of every structure of ``x`` [S,N,3] (fp32, Angstrom, on the device; a strided view is taken as it is).
    ``mask`` [N] marks the C-alpha rows and ``link`` [N] the rows followed by the next residue of the same chain (``trace_links``).
    ``centres``: the ligand's stereocentres as rows (c, n1, n2, n3) of the structure -- a ``Centres`` from ``upload``, or a [C,4] CPU
    tensor / array, which is uploaded here (that copy waits for the host; ``upload`` once to avoid it); the rows are checked against N on
    the host, inside the library, before anything is launched.  ``centre_ref`` [C] fp32 on the device: the signed volumes of the same
    centres in a reference structure (``centre_reference``), or None.  One launch, no host synchronisation, capturable."""
    if not isinstance(windows, Windows):
        raise ValueError(f"windows must be a chirality.Windows, got {type(windows).__name__}")
    bond, vmin, min_helix, min_extended = _thresholds(bond, vmin, min_helix, min_extended)
    x, xs, xr = _structures(x, "x")
    S, N = x.shape[:2]
    rows, links = _mask(mask, "mask", N, x.device), _mask(link, "link", N, x.device)
    if centres is not None and not isinstance(centres, Centres):
        centres = upload(centres, x.device)
    C = 0 if centres is None else int(centres.host.shape[0])
    if C and centres.device.device != x.device:
        raise ValueError(f"centres are on {centres.device.device}, the structures on {x.device}")
    if centre_ref is not None:
        if not C:
            raise ValueError("centre_ref needs centres")
        if not torch.is_tensor(centre_ref) or centre_ref.shape != (C,) or centre_ref.dtype != torch.float32:
            raise ValueError(f"centre_ref must be a [{C}] float32 tensor")
        if centre_ref.device != x.device:
            raise ValueError(f"centre_ref is on {centre_ref.device}, the structures on {x.device}")
        centre_ref = centre_ref.contiguous()
    counts = torch.empty(S, len(COUNT_COLUMNS), dtype=torch.int32, device=x.device)
    verdict, basis = torch.empty(S, dtype=torch.int32, device=x.device), torch.empty(S, dtype=torch.int32, device=x.device)
    tau, cls = torch.empty(S, N, dtype=torch.float32, device=x.device), torch.empty(S, N, dtype=torch.int32, device=x.device)
    volume = torch.empty(S, C, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().prd_chirality_census(dptr(counts, torch.int32), dptr(verdict, torch.int32), dptr(basis, torch.int32), dptr(tau), dptr(cls, torch.int32),
                                          dptr(volume) if C else None, x.data_ptr(), xs, xr, dptr(rows), dptr(links),
                                          dptr(centres.device, torch.int32) if C else None, centres.host.data_ptr() if C else None,
                                          dptr(centre_ref) if C else None, C, *windows.edges(), bond[0], bond[1], vmin, min_helix, min_extended,
                                          S, N, stream()), "prd_chirality_census")
    return Census(counts, verdict, basis, tau, cls, volume)


def reflect(x, flip):
    """Negate coordinate 0 of every structure of ``x`` [S,N,3] whose ``flip`` [S] (a bool or integer device tensor) is set, IN PLACE;
    returns ``x``.  The negation is exact: twice is the identity, and every distance keeps its bits.  ``x`` must be writable where it
    lies (fp32, on the device, last stride 1): a tensor that would have to be copied first is refused."""
    if torch.is_tensor(x) and x.dim() == 3 and (x.stride(2) != 1 or x.stride(1) < 3 or x.stride(0) < 0):
        raise ValueError(f"x with strides {tuple(x.stride())} cannot be reflected in place: the last stride must be 1 and the row stride at least 3")
    t, xs, xr = _structures(x, "x")
    S, N = t.shape[:2]
    if not torch.is_tensor(flip) or flip.shape != (S,) or flip.dtype.is_floating_point or flip.dtype.is_complex:
        raise ValueError(f"flip must be a [{S}] bool or integer tensor")
    if flip.device != t.device:
        raise ValueError(f"flip is on {flip.device}, the structures on {t.device}")
    flags = flip.to(torch.int32).contiguous()
    with torch.cuda.device(t.device):
        _check(lib().prd_chirality_reflect(t.data_ptr(), xs, xr, dptr(flags, torch.int32), S, N, stream()), "prd_chirality_reflect")
    return x


def fix(x, result: Census):
    """``reflect(x, result.verdict < 0)``: the samples judged mirror images, reflected in place"""
    return reflect(x, result.verdict < 0)


# ---- host helpers: the rows of a collated batch -----------------------------------------------------------------------------------------

def trace_links(batch, index: int = 0, num_atoms=None, num_residues=None):
    """(``mask`` [N], ``link`` [N]) fp32 over the collated row of complex ``index`` (ligand rows first, residues after; the layout of
    ``pipeline.collate_fn``), on the batch's device.  ``mask``: the C-alpha mask ``quality.assess`` builds -- residue rows whose C-alpha
    is marked in ``residue_atom_mask[:, :, 1]``.  ``link[i]``: rows i and i + 1 are both masked residues, their ``residue_chain_index`` is
    equal and their ``residue_index`` differs by exactly 1.  ``num_atoms`` / ``num_residues`` as Python ints (default: read from the
    batch, which waits for the device when the batch lives there)."""
    ram = batch["residue_atom_mask"]
    N, dev = ram.shape[1], ram.device
    na = int(batch["num_atoms"][index]) if num_atoms is None else int(num_atoms)
    nr = int(batch["num_residues"][index]) if num_residues is None else int(num_residues)
    if na < 0 or nr < 0 or na + nr > N:
        raise ValueError(f"{na} ligand atoms and {nr} residues do not fit the {N} rows of the batch")
    rows = torch.arange(N, device=dev)
    ca = (rows >= na) & (rows < na + nr) & (ram[index, :, 1] > 0.5)
    ri, ch = batch["residue_index"][index].to(dev), batch["residue_chain_index"][index].to(dev)
    link = torch.zeros(N, dtype=torch.bool, device=dev)
    link[:-1] = ca[1:] & ca[:-1] & (ch[1:] == ch[:-1]) & (ri[1:] - ri[:-1] == 1)
    return ca.float(), link.float()


def ligand_centres(batch, index: int = 0):
    """(``centres`` [C,4] int32, ``atoms`` [C] int64) on the host: the ligand atoms of complex ``index`` that ``atom_feats[:, 1]`` tags as
    tetrahedral stereocentres (1 / 2: CHI_TETRAHEDRAL_CW / CCW) and that have at least 3 neighbours at ``bond_distance == 1``, each with
    its three lowest neighbour indices in ascending order.  Implicit hydrogens are not rows of the complex: a centre with 3 heavy
    neighbours uses exactly those.  The tag only SELECTS the centres -- the neighbour order it refers to is not in the features -- the
    sign comes from coordinates (``centre_reference``).  Reads the batch on the host (a batch on the device is copied)."""
    na = int(batch["num_atoms"][index])
    if na < 1:
        return torch.zeros(0, 4, dtype=torch.int32), torch.zeros(0, dtype=torch.int64)
    tag = batch["atom_feats"][index, :na, 1].cpu()
    bonded = (batch["bond_distance"][index, :na, :na].cpu() == 1)
    bonded = bonded | bonded.T                  # taken as symmetric, as quality.assess does
    bonded.fill_diagonal_(False)
    rows = []
    for c in torch.nonzero((tag == 1) | (tag == 2)).flatten().tolist():
        nb = torch.nonzero(bonded[c]).flatten().tolist()
        if len(nb) >= 3:
            rows.append([c] + nb[:3])
    centres = torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)
    return centres, centres[:, 0].to(torch.int64)


def signed_volumes(pos, centres):
    """float64 [..., C]: V = (x_n1 - x_c) . ((x_n2 - x_c) x (x_n3 - x_c)) of ``centres`` [C,4] in ``pos`` [..., N, 3], on the host"""
    p = np.asarray(pos.cpu() if torch.is_tensor(pos) else pos, dtype=np.float64)
    c = np.asarray(centres.cpu() if torch.is_tensor(centres) else centres, dtype=np.int64).reshape(-1, 4)
    a, b, d = (p[..., c[:, k], :] - p[..., c[:, 0], :] for k in (1, 2, 3))
    return np.einsum("...k,...k->...", a, np.cross(b, d))


def centre_reference(pos, centres, vmin: float = VMIN):
    """The hand of every centre in a reference structure ``pos`` [N,3] (a tensor or an array; the same rows the samples have): its
    signed volumes in float64, rounded once to fp32.  A centre whose reference is itself flat (|V| < ``vmin``) says nothing and is
    dropped.  Returns (the kept subset of ``centres`` [C',4] int32, their volumes [C'] float32), both on the host."""
    vmin = _thresholds(BOND, vmin, 0, 0)[1]
    centres = torch.as_tensor(np.asarray(centres.cpu() if torch.is_tensor(centres) else centres)).to(torch.int32).reshape(-1, 4)
    v = signed_volumes(pos, centres)
    keep = torch.from_numpy(np.abs(v) >= vmin)
    return centres[keep], torch.from_numpy(v.astype(np.float32))[keep]
