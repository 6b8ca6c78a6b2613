"""Sequence rules of sampling: which residue classes a position may take and an additive bias on its logits (``SequenceRules``), how
the final logits are decoded (``Decode``), the ctypes binding of libprd_sequence.so (include/prd_sequence.h) that applies the rules
inside the reverse-diffusion loop, decodes on the device and counts what the decoded samples share, and a torch restatement of each.

The method.  The loop feeds ``seq_t = 2 softmax(seq_pred) - 1`` back to the network at every step.  With rules, the rows they rule are
rewritten after every step boundary: the softmax is retaken over the ALLOWED classes of ``seq_pred + bias``, and a banned class is
exactly -1, so the network is never told that a banned residue is likely.  A class is banned where its bias is at or below ``BANNED``
(PRD_SEQUENCE_BANNED, -32768, the reference's own mask fill): a test on the bias, not an addition -- a fill of -32768 added to a logit
of +40000 would win the softmax.  The loop itself is ``diffusion_model.ReverseDiffusion(..., sequence_rules=...)``; this module holds
the specs, the launchers and the restatements.  ``restate_constrain`` / ``restate_decode`` / ``restate_census`` say in torch what the
launches compute -- the ``logits + bias`` addition in fp32, everything after it in float64: the tests hold the kernels against them; the
model never calls them (there is no CPU fallback)."""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass, field
from typing import Mapping, Optional

import torch

from ._lib import HERE, SideLibrary, dptr, stream
from .conditioning import _tensor as _checked
from .constants import RESIDUE_TYPES

_BINDING = SideLibrary("sequence", 100, "rows of {N_CLS} classes (PRD_SEQUENCE_N_CLS), at most {MAX_B} samples per constrain call "
                       "(PRD_SEQUENCE_MAX_B), {MAX_S} per decode or census call (PRD_SEQUENCE_MAX_S), of {MAX_N} positions (PRD_SEQUENCE_MAX_N)")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version    # 100: include/prd_sequence.h PRD_SEQUENCE_VERSION
lib, _check = _BINDING.lib, _BINDING.check
N_CLS = _DEFINES["N_CLS"]
with open(os.path.join(os.path.dirname(HERE), "include", "prd_sequence.h")) as _f:       # the one float among the header's constants
    BANNED = float(re.search(r"^#define\s+PRD_SEQUENCE_BANNED\s+\(?(-?[\d.]+)f?\)?", _f.read(), flags=re.M).group(1))
BATCH_KEY = "sequence_rules_rows"   # where a loop with rules leaves the rows it ruled, [b,N] 0/1, in the prepared batch
ALPHABET = "X" + "".join(RESIDUE_TYPES)     # class c of the logits is ALPHABET[c] (pipeline.predict_seq)


def _tensor(t, name, shape, like, dtype=torch.float32):
    return _checked(t, name, shape, like, dtype, runs="the sequence rules run", ref="the logits")


def _logits_and_bias(logits, bias, what):
    """(samples, N, n_cls, bias_b) of checked ``logits`` [samples,N,n_cls] and ``bias`` [1 or samples,N,n_cls] or None"""
    if not torch.is_tensor(logits) or logits.dim() != 3:
        raise ValueError(f"{what}: logits must be a [samples,N,{N_CLS}] tensor, got {tuple(logits.shape) if torch.is_tensor(logits) else type(logits).__name__}")
    S, N, n_cls = logits.shape
    bias_b = 1
    if bias is not None:
        if not torch.is_tensor(bias) or bias.dim() != 3 or bias.shape[0] not in (1, S):
            raise ValueError(f"{what}: bias must be a [1 or {S},{N},{n_cls}] tensor, got {tuple(bias.shape) if torch.is_tensor(bias) else type(bias).__name__}")
        bias_b = bias.shape[0]
    _tensor(logits, "logits", (S, N, n_cls), None)
    if bias is not None:
        _tensor(bias, "bias", (bias_b, N, n_cls), logits)
    return S, N, n_cls, bias_b


def constrain_rows_(seq_t, logits, bias, rows):
    """One launch of prd_sequence_constrain (include/prd_sequence.h) on the current stream, in place, no host synchronisation: the rows
    of ``seq_t`` [b,N,21] marked in ``rows`` [b,N] (>= 0.5) become ``2 p - 1`` with ``p`` the softmax of ``logits + bias`` over the
    classes whose ``bias`` [1 or b,N,21] is above ``BANNED``; a banned class becomes exactly -1.  ``rows`` None: nothing is done.  Every
    argument is checked here: shape, dtype, device, contiguity."""
    b, N, n_cls, bias_b = _logits_and_bias(logits, bias, "constrain_rows_")
    _tensor(seq_t, "seq_t", (b, N, n_cls), logits)
    if rows is not None:
        _tensor(rows, "rows", (b, N), logits)
    with torch.cuda.device(logits.device):
        _check(lib().prd_sequence_constrain(dptr(seq_t), dptr(logits), dptr(bias), dptr(rows), b, N, n_cls, bias_b, stream()),
               "prd_sequence_constrain")


def decode(logits, rows, bias=None, gumbel=None, temperature: float = 0.0):
    """One launch of prd_sequence_decode: (tokens [S,N] int32, logp [S,N], entropy [S,N]) of ``logits`` [S,N,21] on the rows marked in
    ``rows`` [S,N], under the ban rule of ``bias`` [1 or S,N,21] (None: no bias, no ban).  ``gumbel`` None: the argmax of ``logits +
    bias``, the lowest index on a tie; otherwise ``gumbel`` [S,N,21] holds Gumbel noise and the token maximises ``(logits + bias) /
    temperature + gumbel`` (temperature > 0).  ``logp`` is the log-probability of the token and ``entropy`` the entropy in nats of the
    softmax at temperature 1 over the allowed classes.  Unmarked rows: -1 / 0 / 0."""
    S, N, n_cls, bias_b = _logits_and_bias(logits, bias, "decode")
    _tensor(rows, "rows", (S, N), logits)
    inv_t = 1.0
    if gumbel is not None:
        if not (isinstance(temperature, (int, float)) and temperature > 0.0 and math.isfinite(temperature)):
            raise ValueError(f"decode: with gumbel noise the temperature must be a positive, finite number, got {temperature!r}")
        _tensor(gumbel, "gumbel", (S, N, n_cls), logits)
        inv_t = 1.0 / float(temperature)
    tokens = torch.empty(S, N, dtype=torch.int32, device=logits.device)
    logp, entropy = torch.empty(S, N, device=logits.device), torch.empty(S, N, device=logits.device)
    with torch.cuda.device(logits.device):
        _check(lib().prd_sequence_decode(dptr(tokens, torch.int32), dptr(logp), dptr(entropy), dptr(logits), dptr(bias), dptr(rows),
                                         dptr(gumbel), inv_t, S, N, n_cls, bias_b, stream()), "prd_sequence_decode")
    return tokens, logp, entropy


def census(tokens, mask, ref_tokens=None, out=None):
    """One launch of prd_sequence_census: (identity [S,S], recovery [S] or None, profile [N,21]), int32 counts over the positions marked
    in ``mask`` [N] of ``tokens`` [S,N] int32 (a token < 0 never matches): the positions two samples share, those a sample shares with
    ``ref_tokens`` [N] int32 (None: no recovery), and per position how many samples carry each class.  ``out``: the three tensors to
    write into (recovery None without a reference); they need not be zeroed."""
    if not torch.is_tensor(tokens) or tokens.dim() != 2:
        raise ValueError(f"census: tokens must be a [S,N] int32 tensor, got {tuple(tokens.shape) if torch.is_tensor(tokens) else type(tokens).__name__}")
    S, N = tokens.shape
    if not torch.is_tensor(mask) or tuple(mask.shape) != (N,):
        raise ValueError(f"mask must be a tensor of shape {(N,)}, got {tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__}")
    _tensor(tokens, "tokens", (S, N), None, torch.int32)
    _tensor(mask, "mask", (N,), tokens)
    if ref_tokens is not None:
        _tensor(ref_tokens, "ref_tokens", (N,), tokens, torch.int32)
    if out is None:
        new = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=tokens.device)     # noqa: E731
        out = (new(S, S), new(S) if ref_tokens is not None else None, new(N, N_CLS))
    identity, recovery, profile = out
    _tensor(identity, "identity", (S, S), tokens, torch.int32), _tensor(profile, "profile", (N, N_CLS), tokens, torch.int32)
    if (recovery is None) != (ref_tokens is None):
        raise ValueError("census: recovery is written with ref_tokens and only with them")
    if recovery is not None:
        _tensor(recovery, "recovery", (S,), tokens, torch.int32)
    i32 = torch.int32
    with torch.cuda.device(tokens.device):
        _check(lib().prd_sequence_census(dptr(identity, i32), dptr(recovery, i32), dptr(profile, i32), dptr(tokens, i32), dptr(ref_tokens, i32),
                                         dptr(mask), S, N, N_CLS, stream()), "prd_sequence_census")
    return identity, recovery, profile


# ---- the restatements: logits + bias in fp32, everything after it in float64 ----------------------------------------------------------

def _ruled(logits, bias):
    """(x float64 with -inf at the banned entries, allowed bool), both [S,N,n_cls]"""
    if bias is None:
        return logits.to(torch.float32).double(), torch.ones_like(logits, dtype=torch.bool)
    bias = bias.to(torch.float32).expand_as(logits)
    allowed = bias > BANNED
    x = (logits.to(torch.float32) + torch.where(allowed, bias, torch.zeros_like(bias))).double()
    return torch.where(allowed, x, torch.full_like(x, -math.inf)), allowed


def _softmax64(x, allowed):
    """(p, log p) over the allowed entries in float64; a row with none gives p = 0, log p = -inf throughout (no NaN)"""
    m = x.amax(dim=-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(allowed, torch.exp(x - m), torch.zeros_like(x))
    total = e.sum(dim=-1, keepdim=True)
    p = torch.where(total > 0, e / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(e))
    logp = torch.where(allowed, x - m - torch.log(torch.where(total > 0, total, torch.ones_like(total))), torch.full_like(x, -math.inf))
    return p, logp


def restate_constrain(seq_t, logits, bias, rows):
    """What ``constrain_rows_`` computes, in torch on any device, NOT in place: seq_t after the launch, float32 (the ruled rows rounded
    once from float64)."""
    out = seq_t.clone()
    if rows is None:
        return out
    p, _ = _softmax64(*_ruled(logits, bias))
    new = (2.0 * p - 1.0).to(torch.float32)
    marked = rows >= 0.5
    out[marked] = new[marked]
    return out


def restate_decode(logits, rows, bias=None, gumbel=None, temperature: float = 0.0):
    """What ``decode`` computes: (tokens int32, logp float64, entropy float64).  The key that is maximised is taken in float64 from the
    fp32 ``logits + bias``; the lowest index wins a tie."""
    x, allowed = _ruled(logits, bias)
    key = x if gumbel is None else torch.where(allowed, x / float(temperature) + gumbel.double(), x)
    top = key.amax(dim=-1, keepdim=True)
    idx = torch.arange(x.shape[-1], device=x.device).expand_as(x)
    tokens = torch.where((key == top) & allowed, idx, torch.full_like(idx, x.shape[-1])).amin(dim=-1)
    some = allowed.any(dim=-1) & (rows >= 0.5)
    p, lp = _softmax64(x, allowed)
    logp = torch.gather(lp, -1, tokens.clamp(max=x.shape[-1] - 1).unsqueeze(-1)).squeeze(-1)
    plogp = torch.where(p > 0, p * torch.where(p > 0, lp, torch.zeros_like(lp)), torch.zeros_like(p))
    entropy = -plogp.sum(dim=-1)
    zero = torch.zeros_like(entropy)
    return (torch.where(some, tokens, torch.full_like(tokens, -1)).to(torch.int32), torch.where(some, logp, zero), torch.where(some, entropy, zero))


def restate_census(tokens, mask, ref_tokens=None):
    """What ``census`` computes: (identity [S,S], recovery [S] or None, profile [N,21]) as int32 counts"""
    on = (mask >= 0.5) & (tokens >= 0)                                                  # [S,N]
    same = (tokens[:, None, :] == tokens[None, :, :]) & on[:, None, :]
    identity = same.sum(dim=-1).to(torch.int32)
    recovery = ((tokens == ref_tokens[None]) & on).sum(dim=-1).to(torch.int32) if ref_tokens is not None else None
    classes = torch.arange(N_CLS, device=tokens.device)
    profile = ((tokens[:, :, None] == classes) & (mask >= 0.5)[None, :, None]).sum(dim=0).to(torch.int32)
    return identity, recovery, profile


# ---- the specs ------------------------------------------------------------------------------------------------------------------------

def _letters(text, what):
    if not isinstance(text, str):
        raise ValueError(f"SequenceRules: {what} must be a string of one-letter residue codes, got {type(text).__name__}")
    for ch in text:
        if ch not in RESIDUE_TYPES:
            raise ValueError(f"SequenceRules: {what} names {ch!r}, which is none of the residue types {''.join(RESIDUE_TYPES)}")
    return [ALPHABET.index(ch) for ch in text]


@dataclass(frozen=True, eq=False)
class SequenceRules:
    """Which classes the ruled rows of the sequence may take and the additive bias on their logits.  Immutable and deterministic,
    validated on construction (ValueError), keyword only: there is no model attribute.

    * ``bias``: fp32 [N,21] or [b,N,21] over the collated row (ligand atoms first, residues after, as every other spec); an entry at or
      below ``BANNED`` bans the class at that position, every other entry is added to the logit (finite, above ``BANNED``);
    * ``scope="design"``: the ruled rows are the residues being redesigned (``residue_inv_extra_mask`` of the prepared batch);
      ``scope="all"``: every residue (``residue_mask``).  Rows that are no residue are never ruled.

    ``SequenceRules.for_residues`` builds the table from letters.  None of it synchronises with the host.  ``inert``: the table holds no
    ban and no bias at all, so the spec rules no row by construction -- the loop then launches nothing for it."""
    bias: torch.Tensor
    scope: str = "design"
    inert: bool = field(default=False, init=False, repr=False)

    def __post_init__(self):
        if self.scope not in ("design", "all"):
            raise ValueError(f"SequenceRules: scope must be 'design' or 'all', got {self.scope!r}")
        if not torch.is_tensor(self.bias):
            raise ValueError(f"SequenceRules: bias must be a tensor [N,{N_CLS}] or [b,N,{N_CLS}], got {type(self.bias).__name__}")
        t = self.bias.detach()
        if t.dim() not in (2, 3) or t.shape[-1] != N_CLS or t.numel() == 0:
            raise ValueError(f"SequenceRules: bias must be [N,{N_CLS}] or [b,N,{N_CLS}], got shape {tuple(t.shape)}")
        t = t.to(torch.float32)
        banned = t <= BANNED
        if not bool((torch.isfinite(t) | banned).all()) or bool(torch.isnan(t).any()):
            raise ValueError("SequenceRules: a bias must be finite (a ban: an entry at or below BANNED)")
        if bool((~banned).sum(dim=-1).eq(0).any()):
            raise ValueError("SequenceRules: a row of the bias table is left with no allowed class")
        object.__setattr__(self, "bias", torch.where(banned, torch.full_like(t, BANNED), t).clone().contiguous())
        object.__setattr__(self, "inert", not bool((t != 0).any()))

    @classmethod
    def for_residues(cls, num_atoms: int, num_residues: int, omit: str = "", allow: Optional[Mapping[int, str]] = None,
                     bias: Optional[Mapping] = None, unknown: bool = False, scope: str = "design") -> "SequenceRules":
        """The table of a complex of ``num_atoms`` ligand atoms and ``num_residues`` residues, built on the host.  ``omit="CM"`` bans
        those residues everywhere; ``allow={i: "AVLI"}`` permits only those at residue ``i`` (0-based); ``bias={"G": 1.5}`` or
        ``{(i, "G"): 1.5}`` adds to the logit of a residue everywhere or at residue ``i``; ``unknown=False`` bans class 0 (``X``)."""
        na, nr = int(num_atoms), int(num_residues)
        if na < 0 or nr < 1:
            raise ValueError(f"SequenceRules.for_residues: num_atoms >= 0 and num_residues >= 1, got {num_atoms!r}, {num_residues!r}")
        table = torch.zeros(na + nr, N_CLS)
        rows = table[na:]

        def residue(i):
            if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < nr:
                raise ValueError(f"SequenceRules: residue index {i!r} is out of range for {nr} residues (0-based)")
            return i
        for key, value in (bias or {}).items():
            where, letter = key if isinstance(key, tuple) else (None, key)
            c = _letters(letter, "bias")
            if len(c) != 1:
                raise ValueError(f"SequenceRules: a bias is keyed by one letter or (residue, letter), got {key!r}")
            value = float(value)
            if not math.isfinite(value):
                raise ValueError(f"SequenceRules: the bias of {key!r} must be finite, got {value!r}")
            if value <= BANNED:
                raise ValueError(f"SequenceRules: the bias of {key!r} is at or below BANNED ({BANNED}); ban a residue with omit= or allow=")
            if where is None:
                rows[:, c[0]] += value
            else:
                rows[residue(where), c[0]] += value
        if bool((rows <= BANNED).any()):
            raise ValueError(f"SequenceRules: biases add up to a value at or below BANNED ({BANNED})")
        if not unknown:
            rows[:, 0] = BANNED
        for c in _letters(omit, "omit"):
            rows[:, c] = BANNED
        for i, letters in (allow or {}).items():
            keep = _letters(letters, f"allow[{i!r}]")
            off = torch.ones(N_CLS, dtype=torch.bool)
            off[keep] = False
            off[0] = False                      # X is ``unknown=``'s to say
            rows[residue(i), off] = BANNED
        empty = torch.nonzero((rows > BANNED).sum(dim=1) == 0).flatten().tolist()
        if empty:
            raise ValueError(f"SequenceRules: residues {empty} are left with no allowed class")
        return cls(table, scope)

    def to(self, device) -> "SequenceRules":
        """The spec with its table on ``device``"""
        if self.bias.device == torch.device(device):
            return self
        moved = object.__new__(SequenceRules)   # validated already: no second look at the values, which would wait for the device
        object.__setattr__(moved, "bias", self.bias.to(device))
        object.__setattr__(moved, "scope", self.scope)
        object.__setattr__(moved, "inert", self.inert)
        return moved

    def table(self, batch) -> torch.Tensor:
        """The [bias_b,N,21] bias tensor (bias_b 1 or b) on the device of the PREPARED ``batch``; ValueError if it does not fit"""
        rm = batch["residue_mask"]
        b, N = rm.shape
        t = self.bias if self.bias.dim() == 3 else self.bias.unsqueeze(0)
        if t.shape[1] != N or t.shape[0] not in (1, b):
            raise ValueError(f"SequenceRules: a bias table of shape {tuple(self.bias.shape)} does not fit a batch of shape {(b, N)}")
        if t.device != rm.device:
            t = (t.pin_memory() if rm.is_cuda and t.device.type == "cpu" else t).to(rm.device, non_blocking=True)
        return t.contiguous()

    def rows(self, batch) -> torch.Tensor:
        """The ruled rows [b,N] 0/1 on the device of the PREPARED ``batch``, built without a host synchronisation"""
        return batch["residue_inv_extra_mask" if self.scope == "design" else "residue_mask"].to(torch.float32).contiguous()

    def apply(self, logits: torch.Tensor, table: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
        """``logits`` with the rules applied on the marked rows -- ``logits + bias`` where allowed, exactly ``BANNED`` where banned --
        and as they are elsewhere: one elementwise expression, what ``ReverseDiffusion.result()`` returns."""
        ruled = torch.where(table > BANNED, logits + table, torch.full_like(logits, BANNED))
        return torch.where(rows.unsqueeze(-1) >= 0.5, ruled, logits)

    def __repr__(self):
        banned = int((self.bias <= BANNED).sum())
        biased = int(((self.bias > BANNED) & (self.bias != 0)).sum())
        return f"SequenceRules(<{banned} banned, {biased} biased of {tuple(self.bias.shape)}>, scope={self.scope!r})"


@dataclass(frozen=True)
class Decode:
    """How ``pipeline.generate_samples`` decodes the logits on the device: ``temperature == 0`` the argmax, otherwise a Gumbel-max draw
    from softmax(logits / temperature) with the sample's own keyed noise; ``against="input"`` also counts the recovery of the input's
    sequence."""
    temperature: float = 0.0
    against: Optional[str] = None

    def __post_init__(self):
        t = self.temperature
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not (t >= 0.0 and math.isfinite(t)):
            raise ValueError(f"Decode: temperature must be a non-negative, finite number, got {t!r}")
        object.__setattr__(self, "temperature", float(t))
        if self.against not in (None, "input"):
            raise ValueError(f"Decode: against must be None or 'input', got {self.against!r}")
