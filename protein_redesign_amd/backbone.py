"""A full backbone from a C-alpha trace, on the device: ctypes binding of libprd_backbone.so (include/prd_backbone.h) and the public
functions on top of it -- ``build`` (N, CA, C, CB and O of every residue of every sample, one launch), the host specs ``Geometry``
(the planar trans peptide and the CB formula), ``Orientation`` (the table that turns the C-alpha virtual dihedral into the peptide
plane's rotation about the CA-CA axis) and ``Backbone`` (both, with the validity thresholds), and ``ideal_chain``, the float64 NeRF
builder the default table is measured on.

The samples of this project are C-alpha traces.  Side-chain packing, inverse folding, structure prediction and secondary-structure
assignment all want N, C and O as well.  The definition is the header's: each peptide is a rigid planar trans unit laid along the
virtual bond between two C-alphas and rotated about it by an angle read off a 73-entry periodic table of the virtual dihedral; the two
ends of a chain are continued by the dyad that maps a regular helix or strand onto itself.  CB is placed with a NEGATIVE coefficient on
(CA - N) x (C - CA), so the residues are L-residues whatever the trace: a backbone built on a mirror-image trace is wrong chemistry, which
is what ``chirality`` / ``generate_samples(handedness="fix")`` are for.

WHAT IS CLAIMED: the launch computes the definition of the header, deterministically, and on ideal chains of the six anchor
conformations the table was measured on it reproduces N and C to 0.02 Angstrom and O to 0.1 Angstrom RMS.  What is NOT: any accuracy
on real proteins -- the table has six knots, was fitted to no structure, and off the anchors the carbonyl oxygen is off by up to
about an Angstrom.

Everything runs on the current stream with no host synchronisation.  HIP only: a missing library or a CPU tensor raises."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from ._lib import SideLibrary, dptr, position_mask as _mask, stream, structures

_BINDING = SideLibrary("backbone", 100, "at most {MAX_N} positions per structure (PRD_BACKBONE_MAX_N) and {MAX_S} structures per call "
                                        "(PRD_BACKBONE_MAX_S)")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version      # 100: include/prd_backbone.h PRD_BACKBONE_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_N, MAX_S, TABLE = _DEFINES["MAX_N"], _DEFINES["MAX_S"], _DEFINES["TABLE"]
_structures = functools.partial(structures, runs="the backbone builder runs", letter="S", bounds=_BINDING)
ATOMS = ("N", "CA", "C", "CB", "O")             # the atom order of ``atoms`` and the bits of ``built``: atom37 indices 0 .. 4
BOND, MIN_ANGLE = (3.3, 4.3), 10.0              # Angstrom (chirality.BOND), degrees
# the six conformations the default table is measured on, (phi, psi) in degrees: alpha, 3-10, beta, antiparallel beta, PPII, left alpha
ANCHORS = ((-57.0, -47.0), (-49.0, -26.0), (-120.0, 130.0), (-139.0, 135.0), (-75.0, 145.0), (57.0, 47.0))


def _f32(v):
    return float(np.float32(v))


def _unit(v):
    return v / np.linalg.norm(v)


@dataclasses.dataclass(frozen=True)
class Geometry:
    """The ideal peptide geometry (bond lengths in Angstrom, angles in degrees; Engh and Huber's values) and the three coefficients of
    CB = CA + ka (b x c) + kb b + kc c, b = CA - N, c = C - CA.  ``n_ca_c`` is used by ``ideal_chain`` alone: the built backbone's own
    N-CA-C angle is whatever the trace makes it."""
    n_ca: float = 1.458
    ca_c: float = 1.525
    c_n: float = 1.329
    c_o: float = 1.231
    ca_c_n: float = 116.2
    c_n_ca: float = 121.7
    ca_c_o: float = 120.5
    n_ca_c: float = 111.0
    cb: tuple = (-0.58273431, 0.56802827, -0.54067466)

    def __post_init__(self):
        for name in ("n_ca", "ca_c", "c_n", "c_o"):
            v = float(getattr(self, name))
            if not (math.isfinite(v) and 0.5 < v < 3.0):
                raise ValueError(f"{name} must be a bond length in Angstrom between 0.5 and 3, got {getattr(self, name)!r}")
            object.__setattr__(self, name, v)
        for name in ("ca_c_n", "c_n_ca", "ca_c_o", "n_ca_c"):
            v = float(getattr(self, name))
            if not (math.isfinite(v) and 90.0 < v < 150.0):
                raise ValueError(f"{name} must be an angle in degrees between 90 and 150, got {getattr(self, name)!r}")
            object.__setattr__(self, name, v)
        try:
            cb = tuple(float(v) for v in self.cb)
        except (TypeError, ValueError):
            cb = ()
        if len(cb) != 3 or not all(math.isfinite(v) for v in cb) or not cb[0] < 0.0:
            raise ValueError(f"cb must be three finite coefficients (ka, kb, kc) with ka < 0 (L-residues), got {self.cb!r}")
        object.__setattr__(self, "cb", cb)

    def plane(self) -> dict:
        """The planar trans peptide between two C-alphas in float64: ``L0`` = |CA - CA'| and the in-plane coordinates (along the CA-CA'
        axis, across it towards the carbonyl carbon) of ``C`` and ``O`` from CA and of ``N`` from CA'."""
        a1, a2, a3 = (math.radians(v) for v in (self.ca_c_n, self.c_n_ca, self.ca_c_o))
        c, n = np.zeros(2), np.array([self.c_n, 0.0])           # C at the origin, N along x; CA above, CA' below (trans)
        ca = self.ca_c * np.array([math.cos(a1), math.sin(a1)])
        ca2 = n + self.n_ca * np.array([-math.cos(a2), -math.sin(a2)])
        o = self.c_o * np.array([math.cos(a1 + a3), math.sin(a1 + a3)])
        l0 = float(np.linalg.norm(ca2 - ca))
        u = (ca2 - ca) / l0
        p = np.array([-u[1], u[0]])
        if np.dot(c - ca, p) < 0.0:
            p = -p
        at = lambda q, origin: (float(np.dot(q - origin, u)), float(np.dot(q - origin, p)))      # noqa: E731
        return {"L0": l0, "C": at(c, ca), "O": at(o, ca), "N": at(n, ca2)}

    def scalars(self) -> tuple:
        """the ten geometry arguments of the launch -- L0, aC, rC, aO, rO, aN, rN, ka, kb, kc -- float64 rounded once to fp32"""
        g = self.plane()
        return tuple(_f32(v) for v in (g["L0"], *g["C"], *g["O"], *g["N"], *self.cb))


def _place(a, b, c, length, angle, dihedral):
    """the point d with |c d| = length, angle (b, c, d) = angle and dihedral (a, b, c, d) = dihedral (radians)"""
    bc = _unit(c - b)
    n = _unit(np.cross(b - a, bc))
    m = np.cross(n, bc)
    return c + length * (-math.cos(angle) * bc + math.sin(angle) * (math.cos(dihedral) * m + math.sin(dihedral) * n))


def ideal_chain(phi, psi, geometry: Geometry = Geometry()) -> np.ndarray:
    """[L,5,3] float64, atoms in the order ``ATOMS``: the chain of ideal bond lengths and angles, omega = 180 degrees, whose backbone
    dihedrals are ``phi`` [L] and ``psi`` [L] in degrees (phi[0] and psi[L-1] have no four atoms and only place what nothing depends
    on), built atom by atom by the natural extension of a reference frame (NeRF).  CB by the formula of ``geometry.cb``."""
    phi, psi = np.atleast_1d(np.asarray(phi, np.float64)), np.atleast_1d(np.asarray(psi, np.float64))
    if phi.shape != psi.shape or phi.ndim != 1 or len(phi) < 1:
        raise ValueError(f"phi and psi must be two [L] sequences of degrees, got shapes {phi.shape} and {psi.shape}")
    g, L = geometry, len(phi)
    rad = math.radians
    out = np.zeros((L, 5, 3))
    n, ca = np.zeros(3), np.array([g.n_ca, 0.0, 0.0])
    c = ca + g.ca_c * np.array([-math.cos(rad(g.n_ca_c)), math.sin(rad(g.n_ca_c)), 0.0])
    for i in range(L):
        out[i, 0], out[i, 1], out[i, 2] = n, ca, c
        out[i, 4] = _place(n, ca, c, g.c_o, rad(g.ca_c_o), rad(psi[i] + 180.0))
        b, d = ca - n, c - ca
        out[i, 3] = ca + g.cb[0] * np.cross(b, d) + g.cb[1] * b + g.cb[2] * d
        if i + 1 < L:
            n2 = _place(n, ca, c, g.c_n, rad(g.ca_c_n), rad(psi[i]))
            ca2 = _place(ca, c, n2, g.n_ca, rad(g.c_n_ca), math.pi)
            c2 = _place(c, n2, ca2, g.ca_c, rad(g.n_ca_c), rad(phi[i + 1]))
            n, ca, c = n2, ca2, c2
    return out


def measure(chain, j: int):
    """(tau, xi) in degrees, tau in [0, 360), of the peptide between residues j and j + 1 of ``chain`` [L,5,3] (1 <= j <= L - 3): the
    virtual dihedral of the C-alphas j - 1 .. j + 2 and the rotation of the true peptide plane about the CA-CA axis, as the header
    defines both"""
    p = np.asarray(chain, np.float64)[:, 1]
    bm, b, bp = p[j] - p[j - 1], p[j + 1] - p[j], p[j + 2] - p[j + 1]
    u, n = _unit(b), _unit(np.cross(bm, b))
    m = np.cross(u, n)
    tau = math.atan2(np.linalg.norm(b) * np.dot(bm, np.cross(b, bp)), np.dot(np.cross(bm, b), np.cross(b, bp)))
    q = chain[j, 2] - p[j]
    return math.degrees(tau) % 360.0, math.degrees(math.atan2(np.dot(q, m), np.dot(q, n)))


_IDEAL = {}


def _wrap(d):
    """an angle difference in degrees taken to [-180, 180): the shorter arc"""
    return (d + 180.0) % 360.0 - 180.0


@dataclasses.dataclass(frozen=True)
class Orientation:
    """Xi(tau): the rotation of the peptide plane about the CA-CA axis as a function of the C-alpha virtual dihedral, both in degrees.
    ``knots``: (tau, xi) pairs; they are sorted by tau (taken to [0, 360)), neighbours -- the last and the first + 360 included -- are
    joined linearly along the SHORTER arc of xi, and ``table()`` samples the curve every 5 degrees.  The curve must close: a set of knots
    whose shorter arcs wind xi once round on the way round tau is refused."""
    knots: tuple

    def __post_init__(self):
        try:
            knots = sorted((float(t) % 360.0, float(x)) for t, x in self.knots)
        except (TypeError, ValueError):
            raise ValueError(f"knots must be (tau, xi) pairs of degrees, got {self.knots!r}") from None
        if not knots or not all(math.isfinite(t) and math.isfinite(x) for t, x in knots):
            raise ValueError(f"knots must be at least one finite (tau, xi) pair of degrees, got {self.knots!r}")
        if any(b[0] - a[0] < 1e-9 for a, b in zip(knots, knots[1:])):
            raise ValueError(f"two knots share a tau: {knots!r}")
        wind = sum(_wrap(b[1] - a[1]) for a, b in zip(knots, knots[1:] + knots[:1]))
        if abs(wind) > 1e-6:
            raise ValueError(f"the shorter arcs between the knots wind xi by {wind:.0f} degrees on the way round tau: the table cannot close")
        object.__setattr__(self, "knots", tuple(knots))

    @staticmethod
    def constant(xi) -> "Orientation":
        """the same rotation ``xi`` (degrees) whatever the dihedral"""
        return Orientation(knots=((0.0, float(xi)),))

    @staticmethod
    def ideal(geometry: Geometry = Geometry()) -> "Orientation":
        """the default: (tau, xi) measured on an ideal chain (``ideal_chain``) of each of the six ``ANCHORS``; made once per geometry"""
        if geometry not in _IDEAL:
            _IDEAL[geometry] = Orientation(knots=tuple(measure(ideal_chain([phi] * 6, [psi] * 6, geometry), 2) for phi, psi in ANCHORS))
        return _IDEAL[geometry]

    def curve(self, tau) -> float:
        """xi in degrees at ``tau`` degrees, on the piecewise-linear curve itself (not the table); unwrapped, so it may leave (-180, 180]"""
        tau, k = float(tau) % 360.0, self.knots
        xi = [k[0][1]]
        for a, b in zip(k, k[1:]):
            xi.append(xi[-1] + _wrap(b[1] - a[1]))               # unwrapped along the shorter arcs: continuous
        ts = [t for t, _ in k] + [k[0][0] + 360.0]
        xi.append(xi[0])                                        # closes: the winding is zero
        if tau < ts[0]:
            tau += 360.0
        for i in range(len(k)):
            if ts[i] <= tau <= ts[i + 1]:
                f = (tau - ts[i]) / (ts[i + 1] - ts[i])
                return xi[i] + f * (xi[i + 1] - xi[i])
        raise AssertionError("unreachable")

    def table(self) -> np.ndarray:
        """[73] float32 radians at tau = 0, 5, ..., 360 degrees; table[72] == table[0]"""
        t = np.array([math.radians(self.curve(5.0 * g)) for g in range(TABLE - 1)], np.float64).astype(np.float32)
        return np.concatenate([t, t[:1]])


def _thresholds(bond, min_angle):
    try:
        lo, hi = (float(v) for v in bond)
    except (TypeError, ValueError):
        raise ValueError(f"bond must be a (lo, hi) pair of Angstrom, got {bond!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError(f"bond must be a window 0 < lo < hi of Angstrom, got ({lo}, {hi})")
    try:
        min_angle = float(min_angle)
    except (TypeError, ValueError):
        raise ValueError(f"min_angle must be an angle in degrees, got {min_angle!r}") from None
    if not (math.isfinite(min_angle) and 0.0 <= min_angle < 90.0):
        raise ValueError(f"min_angle must be an angle 0 <= min_angle < 90 of degrees, got {min_angle!r}")
    return (lo, hi), min_angle


@dataclasses.dataclass(frozen=True)
class Backbone:
    """What ``build`` and ``pipeline.generate_samples(backbone=...)`` take: the peptide geometry, the orientation table (None: the
    ideal one of the geometry) and the validity thresholds of the header -- the window of a virtual bond in Angstrom and the least angle
    in degrees by which three consecutive points must differ from a straight or folded-back line.  ``"build"`` is shorthand for
    ``Backbone()``."""
    geometry: Geometry = Geometry()
    orientation: Orientation = None
    bond: tuple = BOND
    min_angle: float = MIN_ANGLE

    def __post_init__(self):
        if not isinstance(self.geometry, Geometry):
            raise ValueError(f"geometry must be a backbone.Geometry, got {type(self.geometry).__name__}")
        if self.orientation is None:
            object.__setattr__(self, "orientation", Orientation.ideal(self.geometry))
        if not isinstance(self.orientation, Orientation):
            raise ValueError(f"orientation must be a backbone.Orientation, got {type(self.orientation).__name__}")
        bond, min_angle = _thresholds(self.bond, self.min_angle)
        object.__setattr__(self, "bond", bond)
        object.__setattr__(self, "min_angle", min_angle)

    @staticmethod
    def of(value) -> "Backbone":
        """the spec behind a ``backbone=`` argument: a Backbone or ``"build"``; TypeError / ValueError otherwise"""
        if isinstance(value, Backbone):
            return value
        if isinstance(value, str):
            if value != "build":
                raise ValueError(f"backbone must be None, 'build' or a backbone.Backbone, got {value!r}")
            return Backbone()
        raise TypeError(f"backbone must be None, 'build' or a backbone.Backbone, got {type(value).__name__}")

    def scalars(self) -> tuple:
        """the thirteen scalar arguments of the launch: ``geometry.scalars()``, then the squares of the bond window's edges and of the
        sine of ``min_angle``, each squared in float64 and rounded once to fp32"""
        return self.geometry.scalars() + (_f32(self.bond[0] ** 2), _f32(self.bond[1] ** 2), _f32(math.sin(math.radians(self.min_angle)) ** 2))

    def describe(self) -> dict:
        """the table and the geometry as numpy values, for a result dict or an .npz"""
        g = self.geometry.plane()
        return {"table": self.orientation.table(), "L0": np.float64(g["L0"]), "plane_C": np.array(g["C"]), "plane_O": np.array(g["O"]),
                "plane_N": np.array(g["N"]), "cb": np.array(self.geometry.cb), "bond": np.array(self.bond), "min_angle": np.float64(self.min_angle)}


@dataclasses.dataclass(frozen=True)
class Uploaded:
    """A spec with its table on a device.  Made by ``upload``."""
    spec: Backbone
    table: torch.Tensor             # [73] float32 radians


_UPLOADED = {}


def upload(spec="build", device="cuda") -> Uploaded:
    """``spec`` with its orientation table on ``device``, made once per spec and device and kept.  The copy waits for the host: call this
    outside a captured or synchronisation-free region and hand the result (or the same spec) to ``build``."""
    spec, device = Backbone.of(spec), torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (spec, str(device))
    if key not in _UPLOADED:
        _UPLOADED[key] = Uploaded(spec, torch.from_numpy(spec.orientation.table()).to(device))
    return _UPLOADED[key]


@dataclasses.dataclass(frozen=True)
class Built:
    """Device tensors, as the launch wrote them (prd_backbone.h)."""
    atoms: torch.Tensor             # [S,N,5,3] float32 Angstrom, atoms in the order ATOMS; an atom that is not built is zeros
    built: torch.Tensor             # [S,N] int32: bit k set when atom ATOMS[k] is built (CA: wherever mask is set)

    @property
    def flags(self):
        """[S,N,5] bool: ``built`` spread over the atoms"""
        return (self.built.unsqueeze(-1) >> torch.arange(len(ATOMS), device=self.built.device, dtype=torch.int32)) % 2 == 1


def build(x, mask, link, spec=None) -> Built:
    """N, CA, C, CB and O of every row of every structure of ``x`` [S,N,3] (fp32, Angstrom, on the device; a strided view is taken as it
    is).  ``mask`` [N] marks the C-alpha rows and ``link`` [N] the rows followed by the next residue of the same chain
    (``chirality.trace_links``).  ``spec``: a ``Backbone``, ``"build"`` / None for the default, or an ``Uploaded`` from ``upload`` -- a
    spec that has not been uploaded to the device of ``x`` yet is uploaded here, and that copy waits for the host.  One launch, no host
    synchronisation, capturable."""
    x, xs, xr = _structures(x, "x")
    S, N = x.shape[:2]
    rows, links = _mask(mask, "mask", N, x.device), _mask(link, "link", N, x.device)
    up = spec if isinstance(spec, Uploaded) else upload("build" if spec is None else spec, x.device)
    if up.table.device != x.device:
        raise ValueError(f"the table is on {up.table.device}, the structures on {x.device}")
    atoms = torch.empty(S, N, len(ATOMS), 3, dtype=torch.float32, device=x.device)
    built = torch.empty(S, N, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().prd_backbone_build(dptr(atoms), dptr(built, torch.int32), x.data_ptr(), xs, xr, dptr(rows), dptr(links), dptr(up.table),
                                        *up.spec.scalars(), S, N, stream()), "prd_backbone_build")
    return Built(atoms, built)
