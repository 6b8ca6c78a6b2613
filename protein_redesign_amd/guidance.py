"""Guided sampling: distance restraints and clash repulsion that steer the coordinates the network is still free to move
(``Restraint``, ``Guidance``), the ctypes binding of libprd_guide.so (include/prd_guide.h) whose one kernel adds the gradient of their
energy to the predicted noise of a step, and a torch restatement of what that launch computes.

Every step of the reverse process has a clean-structure estimate ``x0 = q (z - r eps)`` with ``q = 1 / sqrt(abar_t)`` and
``r = sqrt(1 - abar_t)``.  An energy ``E(x0)`` -- ``w / 2 max(0, floor - d)^2`` for every pair closer than its class's floor,
``w / 2 (max(0, d - hi)^2 + max(0, lo - d)^2)`` for every restraint -- is evaluated on it, and ``eps <- eps + lam dE/dx0`` (capped per
position) is what the step boundary then consumes.  ``schedule="sigma"`` sets ``lam = scale q r``: classifier guidance of
``exp(-E(x0))``, ``eps - r grad_z log p``, with the Jacobian of ``eps`` dropped; ``"constant"`` sets ``lam = scale``.

Lengths are given in Angstrom and converted ONCE, on the host, to the nanometres of the state; weights multiply squared nanometres.
The thresholds are those of ``quality.assess``: 3.0 / 2.5 / 2.0 Angstrom for residue-residue, residue-ligand and ligand-ligand pairs, the
last only between atoms 4 or more bonds apart.

The loop itself is ``diffusion_model.ReverseDiffusion(..., guidance=...)``; this module holds the spec, the tables, the launcher and the
restatement.  ``restate_guide`` says in torch what the launch computes: the tests hold the kernel against it; the model never calls it
(there is no CPU fallback).  Nothing here says how much guidance improves a sample, or which ``scale`` is sensible."""
from __future__ import annotations

import math
import operator
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from ._lib import SideLibrary, dptr, stream
from .quality import CA_CLASH, CA_STEP, LIGAND_CLASH, LIGAND_SELF_CLASH, SELF_CLASH_MIN_BONDS
from .solver import alphas_cumprod64

_BINDING = SideLibrary("guide", 100, "at most {MAX_B} samples per call (PRD_GUIDE_MAX_B) of {MAX_N} positions (PRD_GUIDE_MAX_N), {MAX_R} "
                       "restraint entries (PRD_GUIDE_MAX_R: two per restraint) and {MAX_ROWS} table rows (PRD_GUIDE_MAX_ROWS)")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version    # 100: include/prd_guide.h PRD_GUIDE_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_N, MAX_R, TABLE_STRIDE = _DEFINES["MAX_N"], _DEFINES["MAX_R"], _DEFINES["TABLE_STRIDE"]
SCHEDULES = ("sigma", "constant")
NM = 0.1                                # nanometres per Angstrom
COINCIDENT = 1e-12                      # nm^2: a pair closer than this contributes nothing (the kernel's GD_COINCIDENT)
CLASH_DEFAULTS = dict(rr=CA_CLASH, rl=LIGAND_CLASH, ll=LIGAND_SELF_CLASH, weight=1.0)


def _number(value, name, positive=False):
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not math.isfinite(v) or v < 0.0 or (positive and v == 0.0):
        raise ValueError(f"{name} must be a {'positive' if positive else 'non-negative'}, finite number, got {value!r}")
    return v


@dataclass(frozen=True, eq=False)
class Restraint:
    """The distance between rows ``i`` and ``j`` of the complex (ligand atoms first, residues after: a residue is its C-alpha) is to lie
    in ``[lo, hi]`` Angstrom; ``None`` leaves that side open, one of them must be given.  ``weight`` multiplies the term."""
    i: int
    j: int
    lo: Optional[float] = None
    hi: Optional[float] = None
    weight: float = 1.0

    def __post_init__(self):
        for name in ("i", "j"):
            v = getattr(self, name)
            try:
                k = -1 if isinstance(v, bool) else operator.index(v)
            except TypeError:
                k = -1
            if k < 0:
                raise ValueError(f"Restraint: {name} must be a non-negative integer row index, got {v!r}")
            object.__setattr__(self, name, k)
        if self.i == self.j:
            raise ValueError(f"Restraint: the two rows must differ, got {self.i} twice")
        if self.lo is None and self.hi is None:
            raise ValueError("Restraint: give lo, hi or both (Angstrom)")
        for name in ("lo", "hi"):
            if getattr(self, name) is not None:
                object.__setattr__(self, name, _number(getattr(self, name), f"Restraint: {name}"))
        if self.lo is not None and self.hi is not None and self.lo > self.hi:
            raise ValueError(f"Restraint: lo must not exceed hi, got [{self.lo}, {self.hi}]")
        object.__setattr__(self, "weight", _number(self.weight, "Restraint: weight", positive=True))

    def __repr__(self):
        return f"Restraint({self.i}, {self.j}, lo={self.lo}, hi={self.hi}, weight={self.weight})"


def chain(batch, tol: float = 0.5, index: int = 0, weight: float = 1.0) -> Tuple[Restraint, ...]:
    """Consecutive C-alphas at 3.8 +- ``tol`` Angstrom: one restraint per pair of rows of complex ``index`` of the collated ``batch``
    that ``quality.assess`` counts as a chain step (both C-alphas marked, one chain, ``residue_index`` differing by 1).  Reads the batch
    on the host."""
    tol = _number(tol, "chain: tol")
    ca = (batch["residue_mask"][index].cpu() > 0.5) & (batch["residue_atom_mask"][index, :, 1].cpu() > 0.5)
    ri, ch = batch["residue_index"][index].cpu(), batch["residue_chain_index"][index].cpu()
    step = ca[1:] & ca[:-1] & (ch[1:] == ch[:-1]) & (ri[1:] - ri[:-1] == 1)
    return tuple(Restraint(int(k), int(k) + 1, max(CA_STEP - tol, 0.0), CA_STEP + tol, weight) for k in torch.nonzero(step).flatten())


def bonds(batch, lo: float = 0.9, hi: float = 2.1, index: int = 0, weight: float = 1.0) -> Tuple[Restraint, ...]:
    """The bonded ligand pairs (``bond_distance == 1`` between two ligand atoms, taken as symmetric) at ``[lo, hi]`` Angstrom, the
    range of ``quality.assess``'s ``ligand_bond_outliers``.  Reads the batch on the host."""
    am = batch["atom_mask"][index].cpu() > 0.5
    bd = batch["bond_distance"][index].cpu()
    bonded = ((bd == 1) | (bd.t() == 1)) & am[:, None] & am[None, :]
    return tuple(Restraint(int(i), int(j), lo, hi, weight) for i, j in torch.nonzero(bonded.triu(1)))


@dataclass(frozen=True, eq=False)
class Guidance:
    """What steers the coordinates of ``sample()``.  Immutable and deterministic, validated on construction (ValueError), keyword
    only: there is no model attribute.

    * ``restraints``: a sequence of ``Restraint`` (``chain(batch)`` and ``bonds(batch)`` build the usual ones);
    * ``clash``: True (the floors of ``quality.assess``: 3.0 / 2.5 / 2.0 Angstrom, weight 1), False, or a dict with any of ``rr``,
      ``rl``, ``ll`` (Angstrom) and ``weight``; ligand-ligand pairs fewer than 4 bonds apart take no part;
    * ``scale``: the strength; ``schedule="sigma"``: ``lam = scale q r`` per level, ``"constant"``: ``lam = scale``;
    * ``cap``: the largest change of ``eps`` at one position in one step;
    * ``from_level``: ``lam = 0`` at every level above it (None: guided from the first step).

    ``inert``: nothing can ever be added (no term, or ``scale == 0``); such a spec launches nothing and uploads nothing."""
    restraints: Sequence[Restraint] = ()
    clash: object = True
    scale: float = 1.0
    cap: float = 0.5
    from_level: Optional[int] = None
    schedule: str = "sigma"

    def __post_init__(self):
        rs = tuple(self.restraints) if not isinstance(self.restraints, Restraint) else (self.restraints,)
        if any(not isinstance(r, Restraint) for r in rs):
            raise ValueError("Guidance: restraints must be a sequence of guidance.Restraint")
        object.__setattr__(self, "restraints", rs)
        clash = self.clash
        if isinstance(clash, bool):
            clash = dict(CLASH_DEFAULTS) if clash else None
        elif isinstance(clash, dict):
            unknown = set(clash) - set(CLASH_DEFAULTS)
            if unknown:
                raise ValueError(f"Guidance: clash takes the keys {sorted(CLASH_DEFAULTS)}, got {sorted(unknown)}")
            clash = {k: _number(clash.get(k, v), f"Guidance: clash[{k!r}]") for k, v in CLASH_DEFAULTS.items()}
            if clash["weight"] == 0.0 or max(clash["rr"], clash["rl"], clash["ll"]) == 0.0:
                clash = None
        else:
            raise ValueError(f"Guidance: clash must be True, False or a dict, got {self.clash!r}")
        object.__setattr__(self, "clash", clash)
        object.__setattr__(self, "scale", _number(self.scale, "Guidance: scale"))
        object.__setattr__(self, "cap", _number(self.cap, "Guidance: cap", positive=True))
        if self.schedule not in SCHEDULES:
            raise ValueError(f"Guidance: schedule must be one of {SCHEDULES}, got {self.schedule!r}")
        if self.from_level is not None:
            if isinstance(self.from_level, bool) or int(self.from_level) != self.from_level or int(self.from_level) < 0:
                raise ValueError(f"Guidance: from_level must be a non-negative integer level, got {self.from_level!r}")
            object.__setattr__(self, "from_level", int(self.from_level))

    @property
    def inert(self) -> bool:
        return self.scale == 0.0 or (not self.restraints and self.clash is None)

    @property
    def floors_nm(self) -> Tuple[float, float, float]:
        """the floors of the pair classes residue-residue, residue-ligand, ligand-ligand in nanometres (zeros without a clash term)"""
        c = self.clash
        return (c["rr"] * NM, c["rl"] * NM, c["ll"] * NM) if c is not None else (0.0, 0.0, 0.0)

    @property
    def clash_weights(self) -> Tuple[float, float, float]:
        w = self.clash["weight"] if self.clash is not None else 0.0
        return (w, w, w)

    def tables(self, T: int, schedule: str, levels=None) -> torch.Tensor:
        """[rows,4] fp32 = {q, r, lam, cap} per counter on the host, computed in float64 from ``solver.alphas_cumprod64`` and rounded
        once: ``rows`` is T, or with ``levels`` (the ascending levels a solver visits) their rows, picked without arithmetic."""
        ab = alphas_cumprod64(T, schedule)
        q, r = 1.0 / torch.sqrt(ab), torch.sqrt(1.0 - ab)
        lam = self.scale * q * r if self.schedule == "sigma" else torch.full_like(q, self.scale)
        if self.from_level is not None:
            lam = torch.where(torch.arange(T) > self.from_level, torch.zeros_like(lam), lam)
        out = torch.stack([q, r, lam, torch.full_like(q, self.cap)], dim=1).to(torch.float32)
        if levels is not None:
            out = out[torch.as_tensor(levels, dtype=torch.int64)]
        return out.contiguous()

    def check_rows(self, rows: int, what: str = "the sample's valid rows") -> None:
        """ValueError when a restraint names a row outside ``[0, rows)`` or there are more than MAX_R entries (host only)"""
        if 2 * len(self.restraints) > MAX_R:
            raise ValueError(f"Guidance: {len(self.restraints)} restraints make {2 * len(self.restraints)} list entries, at most {MAX_R} "
                             f"(PRD_GUIDE_MAX_R: two per restraint) are supported")
        for r in self.restraints:
            if max(r.i, r.j) >= rows:
                raise ValueError(f"Guidance: {r!r} names a row outside {what} [0, {rows})")

    def csr(self, batch):
        """(rs_ptr [b,N+1] int32, rs_j [R] int32, rs_par [R,4] fp32 {lo, hi, w, 0} in nanometres) on the host, or None without
        restraints: every restraint listed under both of its ends, a row's entries in the order of ``restraints``.  Every sample of the
        batch is the same complex and shares the entries: R = 2 len(restraints), the rows of rs_ptr are equal."""
        if not self.restraints:
            return None
        b, N = batch["atom_mask"].shape
        self.check_rows(N, "the batch's rows")
        own = [[] for _ in range(N)]
        for r in self.restraints:
            par = (r.lo * NM if r.lo is not None else 0.0, r.hi * NM if r.hi is not None else float("inf"), r.weight, 0.0)
            own[r.i].append((r.j, par))
            own[r.j].append((r.i, par))
        ptr, js, pars = [0], [], []
        for entries in own:
            js += [j for j, _ in entries]
            pars += [p for _, p in entries]
            ptr.append(len(js))
        rs_ptr = torch.tensor(ptr, dtype=torch.int32).unsqueeze(0).repeat(b, 1).contiguous()
        return rs_ptr, torch.tensor(js, dtype=torch.int32), torch.tensor(pars, dtype=torch.float64).to(torch.float32).reshape(-1, 4)

    def classes(self, batch) -> torch.Tensor:
        """cls [b,N] int32 on the batch's device, without a host synchronisation: 2 at a ligand atom, 1 at a residue whose C-alpha is
        marked, 0 elsewhere -- and 0 everywhere without a clash term"""
        am, rm = batch["atom_mask"], batch["residue_mask"]
        if self.clash is None:
            return torch.zeros(am.shape, dtype=torch.int32, device=am.device)
        ca = (rm > 0.5) & (batch["residue_atom_mask"][:, :, 1] > 0.5)
        return ((am > 0.5).to(torch.int32) * 2 + (ca & ~(am > 0.5)).to(torch.int32)).contiguous()

    def exclusions(self, batch) -> Optional[torch.Tensor]:
        """exclude [b,N,N] uint8 on the batch's device, without a host synchronisation: the ligand-ligand pairs fewer than 4 bonds
        apart in ``bond_distance`` (the comparison ``quality.assess`` makes); None without a clash term"""
        if self.clash is None:
            return None
        am = batch["atom_mask"] > 0.5
        bd = batch["bond_distance"]
        close = (bd < SELF_CLASH_MIN_BONDS) | (bd.transpose(1, 2) < SELF_CLASH_MIN_BONDS)
        return (close & am.unsqueeze(2) & am.unsqueeze(1)).to(torch.uint8).contiguous()

    def terms(self, batch, upload=None) -> dict:
        """The step-invariant arguments of the launch for the PREPARED ``batch`` on its device: ``cls``, ``floors``, ``wclash``,
        ``exclude``, ``csr``.  ``upload``: how a host tensor goes up (default ``.to(device)``); nothing here waits for the device."""
        dev = batch["atom_mask"].device
        up = upload if upload is not None else (lambda x: x.to(dev))
        csr = self.csr(batch)
        return dict(cls=self.classes(batch), floors=up(torch.tensor(self.floors_nm, dtype=torch.float32)),
                    wclash=up(torch.tensor(self.clash_weights, dtype=torch.float32)), exclude=self.exclusions(batch),
                    csr=tuple(up(x) for x in csr) if csr is not None else None)

    def describe(self) -> dict:
        """the spec's terms as numpy-friendly values: what ``generate_samples`` returns and writes"""
        import numpy as np
        c = self.clash or dict(rr=0.0, rl=0.0, ll=0.0, weight=0.0)
        rs = self.restraints
        return {"restraints": np.array([[r.i, r.j] for r in rs], dtype=np.int64).reshape(-1, 2),
                "restraint_bounds": np.array([[r.lo if r.lo is not None else 0.0, r.hi if r.hi is not None else np.inf, r.weight] for r in rs],
                                             dtype=np.float64).reshape(-1, 3),
                "clash": np.array([c["rr"], c["rl"], c["ll"], c["weight"]], dtype=np.float64), "scale": self.scale, "cap": self.cap,
                "from_level": -1 if self.from_level is None else self.from_level, "schedule": self.schedule}

    def __repr__(self):
        return (f"Guidance({len(self.restraints)} restraints, clash={self.clash}, scale={self.scale}, cap={self.cap}, "
                f"from_level={self.from_level}, schedule={self.schedule!r})")


def check_guidance(guidance) -> None:
    if not isinstance(guidance, Guidance):
        raise TypeError(f"guidance must be a guidance.Guidance, got {type(guidance).__name__}")


def guide_eps_(z, eps_raw, eps_out, mask, counter, table, cls, floors, wclash, exclude=None, csr=None, e_out=None):
    """One launch of prd_guide_eps (include/prd_guide.h) on the current stream, no host synchronisation: ``eps_out`` [b,N,3] becomes
    ``eps_raw`` plus the capped, scaled gradient of the energy on ``x0 = q (z - r eps)``, (q, r, lam, cap) being row ``counter[s]`` of
    ``table`` [rows,4] (``counter=None``: row 0).  ``csr``: (rs_ptr, rs_j, rs_par) or None; ``e_out`` [b,N,2] or None."""
    b, N, _ = z.shape
    if tuple(eps_raw.shape) != (b, N, 3) or tuple(eps_out.shape) != (b, N, 3) or tuple(mask.shape) != (b, N) or tuple(cls.shape) != (b, N):
        raise ValueError(f"guide_eps_: z, eps_raw and eps_out must be [{b},{N},3], mask and cls [{b},{N}]")
    if table.dim() != 2 or table.shape[1] != TABLE_STRIDE:
        raise ValueError(f"table must be [rows,{TABLE_STRIDE}] = (q, r, lam, cap) per counter, got {tuple(table.shape)}")
    if counter is not None and tuple(counter.shape) != (b,):
        raise ValueError(f"counter must be a [{b}] int64 tensor, got {tuple(counter.shape)}")
    if exclude is not None and tuple(exclude.shape) != (b, N, N):
        raise ValueError(f"exclude must be a [{b},{N},{N}] uint8 tensor, got {tuple(exclude.shape)}")
    if e_out is not None and tuple(e_out.shape) != (b, N, 2):
        raise ValueError(f"e_out must be [{b},{N},2], got {tuple(e_out.shape)}")
    if floors.numel() != 3 or wclash.numel() != 3:
        raise ValueError("floors and wclash hold one entry per pair class: residue-residue, residue-ligand, ligand-ligand")
    ptr = js = par = None
    R = 0
    if csr is not None:
        ptr, js, par = csr
        R = js.shape[0]
        if tuple(ptr.shape) != (b, N + 1) or tuple(par.shape) != (R, 4):
            raise ValueError(f"the restraint lists must be rs_ptr [{b},{N + 1}], rs_j [R], rs_par [R,4]; got {tuple(ptr.shape)}, "
                             f"{tuple(js.shape)}, {tuple(par.shape)}")
    with torch.cuda.device(z.device):
        _check(lib().prd_guide_eps(dptr(z), dptr(eps_raw), dptr(eps_out), dptr(mask), dptr(counter, torch.int64), dptr(table),
                                   dptr(cls, torch.int32), dptr(floors), dptr(wclash), dptr(exclude, torch.uint8), dptr(ptr, torch.int32),
                                   dptr(js, torch.int32), dptr(par), dptr(e_out), b, N, table.shape[0], R, stream()), "prd_guide_eps")


def energy(x, batch, spec: Guidance) -> torch.Tensor:
    """[S,2] float64 on the device: the clash and the restraint energy of the finished structures ``x`` [S,N,3] (Angstrom, the rows of
    the collated ``batch``, whose complexes are S or one for all).  ONE launch with q = 1, r = 0, lam = 0 -- nothing is moved --, then a
    float64 sum of ``e_out`` over the rows."""
    check_guidance(spec)
    if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != 3:
        raise ValueError(f"x must be a [S,N,3] tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    S, N, _ = x.shape
    b = batch["atom_mask"].shape[0]
    if batch["atom_mask"].shape[1] != N or b not in (1, S):
        raise ValueError(f"x has {S} structures of {N} rows, the batch {b} complexes of {batch['atom_mask'].shape[1]}")
    z = (NM * x.to(torch.float32)).contiguous()
    t = spec.terms(batch)
    grow = lambda v: v if v is None or v.shape[0] == S else v.expand(S, *v.shape[1:]).contiguous()     # noqa: E731
    mask = grow((batch["atom_mask"] + batch["residue_mask"]).to(torch.float32).contiguous())
    csr = (grow(t["csr"][0]),) + t["csr"][1:] if t["csr"] is not None else None
    table = torch.tensor([[1.0, 0.0, 0.0, spec.cap]], dtype=torch.float32).to(z.device)
    eps, out, e = torch.zeros_like(z), torch.empty_like(z), torch.empty(S, N, 2, dtype=torch.float32, device=z.device)
    guide_eps_(z, eps, out, mask, None, table, grow(t["cls"]), t["floors"], t["wclash"], grow(t["exclude"]), csr, e)
    return e.double().sum(dim=1)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _entries(ptr_row, N):
    """(owning row, entry index) of every list entry of one sample, in list order"""
    own, idx = [], []
    for i in range(N):
        lo, hi = int(ptr_row[i]), int(ptr_row[i + 1])
        own += [i] * max(hi - lo, 0)
        idx += list(range(lo, hi))
    return torch.tensor(own, dtype=torch.int64), torch.tensor(idx, dtype=torch.int64)


def restate_rows(x, mask, cls, floors, wclash, exclude=None, csr=None):
    """Energy shares and gradient of ONE structure ``x`` [N,3] (nanometres, any floating dtype), differentiable in ``x``:
    (e [N,2], g [N,3]) with ``e[i]`` half of every pair term row i takes part in and ``g`` the analytic ``dE/dx`` of ``E = e.sum()``
    (for a symmetric ``exclude`` and both-ended lists).  ``csr``: (rs_ptr row [N+1], rs_j, rs_par)."""
    N, dt = x.shape[0], x.dtype
    c = torch.where((mask > 0.5) & ((cls == 1) | (cls == 2)), cls, torch.zeros_like(cls)).to(torch.int64)
    diff = x.unsqueeze(1) - x.unsqueeze(0)                                          # x_i - x_j
    d2 = (diff * diff).sum(-1)
    live = d2 >= COINCIDENT
    d = torch.sqrt(torch.where(live, d2, torch.ones_like(d2)))
    part = (c.unsqueeze(1) != 0) & (c.unsqueeze(0) != 0) & live & ~torch.eye(N, dtype=torch.bool)
    if exclude is not None:
        part = part & (exclude == 0)
    pc = (c.unsqueeze(1) + c.unsqueeze(0) - 2).clamp(0, 2)
    f, w = floors.to(dt)[pc], wclash.to(dt)[pc]
    h = torch.clamp(f - d, min=0.0) * part.to(dt)
    e_clash = (0.25 * w * h * h).sum(1)
    g = ((-(w * h) / d).unsqueeze(-1) * diff).sum(1)
    e_rest = torch.zeros(N, dtype=dt)
    if csr is not None:
        ptr, js, par = csr
        own, idx = _entries(ptr, N)
        keep = (idx >= 0) & (idx < js.shape[0])
        own, idx = own[keep], idx[keep]
        jj = js[idx].to(torch.int64)
        keep = (jj >= 0) & (jj < N) & (jj != own)
        own, idx, jj = own[keep], idx[keep], jj[keep]
        lo, hi, wr = (par[idx, k].to(dt) for k in range(3))
        dr = x[own] - x[jj]
        r2 = (dr * dr).sum(-1)
        ok = (r2 >= COINCIDENT).to(dt)
        rd = torch.sqrt(torch.where(r2 >= COINCIDENT, r2, torch.ones_like(r2)))
        over, under = torch.clamp(rd - hi, min=0.0) * ok, torch.clamp(lo - rd, min=0.0) * ok
        e_rest = e_rest.index_add(0, own, 0.25 * wr * (over * over + under * under))
        g = g.index_add(0, own, (wr * (over - under) / rd).unsqueeze(-1) * dr)
    return torch.stack([e_clash, e_rest], dim=1), g


def restate_guide(z, eps_raw, mask, counter, table, cls, floors, wclash, exclude=None, csr=None, dtype=torch.float64):
    """What ``guide_eps_`` computes, in torch on the host in ``dtype``, NOT in place: a dict with ``eps_out`` [b,N,3], ``e_out``
    [b,N,2], ``x`` (the estimate), ``g`` (dE/dx) and ``live`` [b], the samples whose counter lay in [0, rows).  The launch leaves every
    other sample alone; here its rows of ``eps_out`` are ``eps_raw`` and the others zero, and mean nothing."""
    f = lambda v: v.detach().cpu().to(dtype)          # noqa: E731
    b, N, _ = z.shape
    kh = [0] * b if counter is None else counter.cpu().tolist()
    z, eps_raw, mask, tab, floors, wclash = (f(v) for v in (z, eps_raw, mask, table, floors, wclash))
    cls = cls.detach().cpu()
    exclude = exclude.detach().cpu() if exclude is not None else None
    if csr is not None:
        csr = (csr[0].detach().cpu(), csr[1].detach().cpu(), f(csr[2]))
    out = dict(eps_out=eps_raw.clone(), e_out=torch.zeros(b, N, 2, dtype=dtype), x=torch.zeros_like(z), g=torch.zeros_like(z),
               live=torch.zeros(b, dtype=torch.bool))
    for s in range(b):
        kk = kh[s]
        if not 0 <= kk < tab.shape[0]:
            continue
        out["live"][s] = True
        q, r, lam, cap = tab[kk]
        m = mask[s].unsqueeze(-1)
        eps = eps_raw[s] - m * ((m * eps_raw[s]).sum(0) / m.sum())
        x = q * (z[s] - r * eps)
        e, g = restate_rows(x, mask[s], cls[s], floors, wclash, exclude[s] if exclude is not None else None,
                            (csr[0][s], csr[1], csr[2]) if csr is not None else None)
        delta = lam * g
        nrm = delta.norm(dim=-1, keepdim=True)
        delta = torch.where(nrm > cap, delta * (cap / torch.where(nrm > 0, nrm, torch.ones_like(nrm))), delta)
        out["x"][s], out["g"][s], out["e_out"][s] = x, g, e
        if float(lam) != 0.0:
            out["eps_out"][s] = eps_raw[s] + m * delta
    return out
