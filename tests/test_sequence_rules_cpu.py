"""CPU: sequence rules as far as they go without a GPU -- the ``SequenceRules`` / ``Decode`` specs and their refusals, ``table`` and ``rows``
on a prepared batch, the torch restatements against straight float64 formulas, the header / build / export list / resources of
libprd_sequence.so, the refusals the library makes on the host, the Python-side argument checks, and the ``sequence_rules`` / ``decode``
arguments of pipeline.generate_samples with stub models (what they return, where, what they write, and that nothing changes without
them)."""
import contextlib
import ctypes
import math
import os
import warnings
from unittest import mock

import numpy as np
import pytest
import torch

from conftest import ROOT
from protein_redesign_amd import _lib, build
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd import sequence as SQ
from protein_redesign_amd.conditioning import Scaffold
from protein_redesign_amd.constants import RESIDUE_TYPES, make_args
from protein_redesign_amd.sequence import BANNED, Decode, SequenceRules
from protein_redesign_amd.synthetic import NoiseSource
from sample_stubs import _NoDevice, _Stub, header_entries
from test_conditioning_cpu import _ScaffoldStub
from test_generate_samples_combinations_cpu import NA, NR, complex_data, fakes, redesign_spec

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))


# ---- the specs ------------------------------------------------------------------------------------------------------------------------

def test_for_residues_builds_the_table():
    assert BANNED == -32768.0 and SQ.ALPHABET == "X" + "".join(RESIDUE_TYPES) and SQ.N_CLS == 21
    r = SequenceRules.for_residues(3, 5, omit="CM", allow={1: "AVLI"}, bias={"G": 1.5, (2, "A"): -2.0})
    cls = SQ.ALPHABET.index
    assert r.scope == "design" and r.bias.shape == (8, 21) and r.bias.dtype == torch.float32 and r.bias.is_contiguous()
    assert float(r.bias[:3].abs().max()) == 0.0                                 # ligand rows: no rule
    assert bool((r.bias[3:, 0] == BANNED).all())                                # unknown=False bans X on the residue rows
    assert bool((r.bias[3:, [cls("C"), cls("M")]] == BANNED).all())
    assert sorted(torch.nonzero(r.bias[4] > BANNED).flatten().tolist()) == sorted(cls(ch) for ch in "AVLI")
    assert float(r.bias[5, cls("A")]) == -2.0 and float(r.bias[5, cls("G")]) == 1.5 and float(r.bias[3, cls("G")]) == 1.5
    assert float(r.bias[4, cls("G")]) == BANNED                                 # not among the allowed of residue 1
    u = SequenceRules.for_residues(0, 2, unknown=True, scope="all")
    assert u.scope == "all" and float(u.bias.abs().max()) == 0.0
    both = SequenceRules.for_residues(0, 2, bias={"G": 1.0, (1, "G"): 0.5})
    assert float(both.bias[0, cls("G")]) == 1.0 and float(both.bias[1, cls("G")]) == 1.5
    assert "banned" in repr(r) and "design" in repr(r)
    assert u.inert and SequenceRules(torch.zeros(4, 21)).inert and not r.inert and not both.inert and not SequenceRules.for_residues(0, 2).inert


def test_specs_are_validated_on_construction_and_immutable():
    r = SequenceRules.for_residues(1, 4)
    with pytest.raises(Exception):              # frozen
        r.scope = "all"
    t = torch.zeros(5, 21)
    spec = SequenceRules(t)
    t[0, 0] = 3.0
    assert float(spec.bias[0, 0]) == 0.0 and spec.to("cpu") is spec              # a copy: the caller's tensor is not the spec's
    assert SequenceRules(torch.zeros(2, 5, 21)).bias.shape == (2, 5, 21)
    assert float(SequenceRules(torch.full((1, 21), -1e9).index_fill(1, torch.tensor([3]), 0.0)).bias.min()) == BANNED
    for bad in ("B", "x", "AZ", "X"):
        with pytest.raises(ValueError, match="residue types"):
            SequenceRules.for_residues(1, 4, omit=bad)
    with pytest.raises(ValueError, match="residue types"):
        SequenceRules.for_residues(1, 4, allow={0: "A1"})
    with pytest.raises(ValueError, match="residue types"):
        SequenceRules.for_residues(1, 4, bias={"J": 1.0})
    for bad in (4, -1, 1.0, True, "0"):
        with pytest.raises(ValueError, match="out of range"):
            SequenceRules.for_residues(1, 4, allow={bad: "A"})
    with pytest.raises(ValueError, match="out of range"):
        SequenceRules.for_residues(1, 4, bias={(7, "A"): 1.0})
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            SequenceRules.for_residues(1, 4, bias={"A": bad})
    for bad in (BANNED, BANNED - 1.0, -1e9):
        with pytest.raises(ValueError, match="at or below BANNED"):
            SequenceRules.for_residues(1, 4, bias={"A": bad})
    with pytest.raises(ValueError, match="one letter"):
        SequenceRules.for_residues(1, 4, bias={"AG": 1.0})
    with pytest.raises(ValueError, match=r"residues \[2\] are left with no allowed class"):
        SequenceRules.for_residues(1, 4, omit="AV", allow={2: "AV"})
    with pytest.raises(ValueError, match="no allowed class"):
        SequenceRules.for_residues(1, 4, omit="".join(RESIDUE_TYPES))
    with pytest.raises(ValueError, match="scope"):
        SequenceRules.for_residues(1, 4, scope="pocket")
    with pytest.raises(ValueError, match="num_residues"):
        SequenceRules.for_residues(1, 0)
    for bad in (torch.zeros(5, 20), torch.zeros(21), torch.zeros(0, 21), torch.zeros(1, 2, 3, 21)):
        with pytest.raises(ValueError, match="bias must be"):
            SequenceRules(bad)
    with pytest.raises(ValueError, match="bias must be"):
        SequenceRules([[0.0] * 21])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            SequenceRules(torch.full((2, 21), bad))
    with pytest.raises(ValueError, match="no allowed class"):
        SequenceRules(torch.full((2, 21), BANNED))
    assert Decode() == Decode(0.0, None) and Decode(1, "input").temperature == 1.0
    for bad in (-0.1, float("nan"), float("inf"), "0", True):
        with pytest.raises(ValueError, match="temperature"):
            Decode(bad)
    with pytest.raises(ValueError, match="against"):
        Decode(against="first")
    with pytest.raises(Exception):
        Decode().temperature = 1.0


def test_table_and_rows_on_a_prepared_batch():
    rm = torch.tensor([[0.0, 0, 1, 1, 1, 0], [0.0, 1, 1, 1, 1, 1]])
    inv = rm * torch.tensor([0.0, 0, 1, 0, 1, 1])
    batch = {"residue_mask": rm, "residue_inv_extra_mask": inv, "residue_extra_mask": rm - inv}
    d, a = SequenceRules(torch.zeros(6, 21)), SequenceRules(torch.zeros(6, 21), scope="all")
    assert torch.equal(d.rows(batch), inv) and torch.equal(a.rows(batch), rm) and d.rows(batch).dtype == torch.float32
    assert d.table(batch).shape == (1, 6, 21) and SequenceRules(torch.zeros(2, 6, 21)).table(batch).shape == (2, 6, 21)
    assert SequenceRules(torch.zeros(1, 6, 21)).table(batch).shape == (1, 6, 21) and d.table(batch).is_contiguous()
    for bad in (torch.zeros(5, 21), torch.zeros(3, 6, 21)):
        with pytest.raises(ValueError, match="does not fit"):
            SequenceRules(bad).table(batch)
    # what result() returns: logits + bias where allowed, BANNED where banned, on the ruled rows alone
    table = torch.zeros(1, 6, 21)
    table[0, :, 4], table[0, :, 5] = BANNED, 2.0
    logits = torch.randn(2, 6, 21)
    got = d.apply(logits, table, inv)
    on = inv > 0.5
    assert torch.equal(got[~on], logits[~on]) and bool((got[on][:, 4] == BANNED).all())
    assert torch.equal(got[on][:, 5], logits[on][:, 5] + 2.0) and torch.equal(got[on][:, :4], logits[on][:, :4])


def test_the_model_refuses_rules_it_cannot_serve():
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    model = ProteinReDiffModel(make_args(single_dim=128, pair_dim=64, num_blocks=1, esm_dim=64, num_steps=4))
    r = SequenceRules.for_residues(1, 4)
    assert model._rules_spec(None) is None and model._rules_spec(r) is r and not hasattr(model, "sequence_rules")
    with pytest.raises(TypeError, match="SequenceRules"):
        model._rules_spec("C")
    with pytest.raises(TypeError, match="SequenceRules"):
        model.sample({}, sources=[], sequence_rules=Scaffold())
    model.training_mode = True
    with pytest.raises(ValueError, match="training_mode"):
        model.sample({}, sources=[], sequence_rules=r)


# ---- the restatements against straight float64 formulas ----------------------------------------------------------------------------------

def case(S, N, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    logits, bias = scale * torch.randn(S, N, 21, generator=g), torch.randn(1, N, 21, generator=g)
    bias[torch.rand(1, N, 21, generator=g) < 0.3] = BANNED
    bias[0, 0] = BANNED                          # a row with nothing allowed
    rows = (torch.rand(S, N, generator=g) < 0.7).float()
    rows[:, 0] = 1.0
    return logits, bias, rows, torch.randn(S, N, 21, generator=g), g


@pytest.mark.parametrize("scale", [1.0, 400.0, 1e4])
def test_restate_constrain_against_float64(scale):
    logits, bias, rows, seq_t, _ = case(3, 17, 1, scale)
    got = SQ.restate_constrain(seq_t, logits, bias, rows)
    assert got is not seq_t and got.dtype == torch.float32 and torch.equal(SQ.restate_constrain(seq_t, logits, bias, None), seq_t)
    for s in range(3):
        for i in range(17):
            if rows[s, i] < 0.5:
                assert torch.equal(got[s, i], seq_t[s, i])
                continue
            on = [c for c in range(21) if float(bias[0, i, c]) > BANNED]
            x = {c: float(logits[s, i, c] + bias[0, i, c]) for c in on}        # the fp32 sum, then Python floats: float64
            m = max(x.values(), default=0.0)
            total = sum(math.exp(v - m) for v in x.values())
            for c in range(21):
                want = 2.0 * math.exp(x[c] - m) / total - 1.0 if c in x else -1.0
                assert abs(float(got[s, i, c]) - want) <= 2.0 ** -24 and (c in x or float(got[s, i, c]) == -1.0), (s, i, c)
    assert bool((got[:, 0] == -1.0).all()) and bool(torch.isfinite(got).all())


@pytest.mark.parametrize("temperature", [0.0, 0.5, 2.0])
def test_restate_decode_against_float64(temperature):
    logits, bias, rows, _, g = case(2, 19, 2)
    gumbel = -torch.log(-torch.log(torch.rand(2, 19, 21, generator=g))) if temperature > 0 else None
    tokens, logp, entropy = SQ.restate_decode(logits, rows, bias, gumbel, temperature)
    assert tokens.dtype == torch.int32 and logp.dtype == entropy.dtype == torch.float64
    for s in range(2):
        for i in range(19):
            on = [c for c in range(21) if float(bias[0, i, c]) > BANNED]
            if rows[s, i] < 0.5 or not on:
                assert (int(tokens[s, i]), float(logp[s, i]), float(entropy[s, i])) == (-1, 0.0, 0.0)
                continue
            x = {c: float(logits[s, i, c] + bias[0, i, c]) for c in on}
            key = {c: x[c] / temperature + float(gumbel[s, i, c]) if temperature > 0 else x[c] for c in on}
            tok = min(c for c in on if key[c] == max(key.values()))
            m = max(x.values())
            lse = m + math.log(sum(math.exp(v - m) for v in x.values()))
            p = {c: math.exp(x[c] - lse) for c in on}
            assert int(tokens[s, i]) == tok and abs(float(logp[s, i]) - (x[tok] - lse)) <= 1e-12
            assert abs(float(entropy[s, i]) + sum(v * math.log(v) for v in p.values() if v > 0)) <= 1e-12
    none = SQ.restate_decode(logits, rows)          # no bias: no ban
    assert torch.equal(none[0][rows >= 0.5], logits.argmax(-1).to(torch.int32)[rows >= 0.5])
    tie = torch.zeros(1, 2, 21)
    tie[0, 1, [4, 9]] = 1.0
    assert SQ.restate_decode(tie, torch.ones(1, 2))[0].tolist() == [[0, 4]]


def test_restate_census_against_loops():
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(-1, 5, (4, 23), generator=g, dtype=torch.int32)
    mask, ref = (torch.rand(23, generator=g) < 0.7).float(), torch.randint(-1, 5, (23,), generator=g, dtype=torch.int32)
    identity, recovery, profile = SQ.restate_census(tokens, mask, ref)
    assert identity.dtype == recovery.dtype == profile.dtype == torch.int32 and profile.shape == (23, 21)
    for s in range(4):
        for r in range(4):
            assert int(identity[s, r]) == sum(1 for i in range(23) if mask[i] >= 0.5 and tokens[s, i] >= 0 and tokens[s, i] == tokens[r, i])
        assert int(recovery[s]) == sum(1 for i in range(23) if mask[i] >= 0.5 and tokens[s, i] >= 0 and tokens[s, i] == ref[i])
    for i in range(23):
        for c in range(21):
            assert int(profile[i, c]) == (sum(1 for s in range(4) if tokens[s, i] == c) if mask[i] >= 0.5 else 0)
    assert SQ.restate_census(tokens, mask)[1] is None


def test_gumbel_comes_from_the_keyed_source_after_the_other_draws():
    a, b = NoiseSource(3, 1), NoiseSource(3, 1)
    assert torch.equal(a.randn(4, 3), b.randn(4, 3))
    g = a.gumbel(5, 21)
    u = torch.rand(5, 21, generator=b.g).clamp_(min=torch.finfo(torch.float32).tiny)
    assert g.shape == (5, 21) and torch.equal(g, -torch.log(-torch.log(u))) and bool(torch.isfinite(g).all())


# ---- header, build, export list -------------------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    from protein_redesign_amd import align, conditioning, quality, tmalign
    e = header_entries("sequence")
    assert sorted(e) == ["prd_sequence_census", "prd_sequence_constrain", "prd_sequence_decode", "prd_sequence_version"]
    assert all(x.inject is None and x.restype is _lib.ci for x in e.values())
    assert e["prd_sequence_constrain"].argtypes == [_lib.vp] * 4 + [_lib.ci] * 4 + [_lib.vp]
    assert e["prd_sequence_decode"].argtypes == [_lib.vp] * 7 + [_lib.cf] + [_lib.ci] * 4 + [_lib.vp]
    assert e["prd_sequence_census"].argtypes == [_lib.vp] * 6 + [_lib.ci] * 3 + [_lib.vp] and e["prd_sequence_version"].argtypes == []
    assert SQ.ENTRIES == e
    assert not set(e) & (set(_lib.ENTRIES) | set(align.ENTRIES) | set(tmalign.ENTRIES) | set(quality.ENTRIES) | set(conditioning.ENTRIES))
    assert SQ.ABI_VERSION == SQ._DEFINES["VERSION"] == 100 and SQ._DEFINES["ERR_ARG"] == -1 and SQ._DEFINES["ERR_UNSUPPORTED"] == -3
    assert (SQ._DEFINES["MAX_B"], SQ._DEFINES["MAX_N"], SQ._DEFINES["MAX_S"]) == (65535, 16777216, 4096)
    with open(os.path.join(ROOT, "protein_redesign_amd", "csrc", "prd_sequence.hip")) as f:
        assert '#include "prd_launch.h"' in f.read()         # the host half of its launch is the project's one


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_new_kernels():
    """hipcc 7 for gfx950, committed flags: constrain_kernel 11 VGPR, decode_kernel 16 VGPR, census_kernel 12 VGPR; each 0 AGPR, no
    scratch, no LDS, 8 waves per SIMD."""
    mine = build.resource_usage(sources=build.SIDE_LIBS["sequence"].sources)
    assert sorted(mine) == ["census_kernel", "constrain_kernel", "decode_kernel"]
    for name, u in mine.items():
        print(f"{name}: {u}")
        assert u["scratch"] == 0 and u["agprs"] == 0 and u["lds"] == 0 and u["occupancy"] == 8 and u["vgprs"] <= 32, name


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_library_refuses_on_the_host_before_any_device_call():
    """the refusals of prd_sequence.h are host code that runs before the first HIP call: every one of them is reachable without a GPU,
    with pointers that are never followed"""
    build.build_side("sequence", verbose=False)
    L, D = SQ.lib(), SQ._DEFINES
    assert L.prd_sequence_version() == 100
    p = ctypes.c_void_p(4096)

    def constrain(seq_t=p, logits=p, bias=p, rows=p, b=2, N=5, n_cls=21, bias_b=2):
        return L.prd_sequence_constrain(seq_t, logits, bias, rows, b, N, n_cls, bias_b, None)

    def decode(tokens=p, logp=p, entropy=p, logits=p, bias=p, rows=p, gumbel=p, S=2, N=5, n_cls=21, bias_b=1):
        return L.prd_sequence_decode(tokens, logp, entropy, logits, bias, rows, gumbel, 1.0, S, N, n_cls, bias_b, None)

    def census(identity=p, recovery=p, profile=p, tokens=p, ref=p, mask=p, S=2, N=5, n_cls=21):
        return L.prd_sequence_census(identity, recovery, profile, tokens, ref, mask, S, N, n_cls, None)
    for kw in (dict(b=0), dict(b=-1), dict(N=0), dict(N=-4), dict(seq_t=None), dict(logits=None), dict(bias_b=3), dict(bias_b=0)):
        assert constrain(**kw) == D["ERR_ARG"], kw
    for kw in (dict(n_cls=20), dict(n_cls=22), dict(n_cls=0), dict(b=D["MAX_B"] + 1), dict(N=D["MAX_N"] + 1)):
        assert constrain(**kw) == D["ERR_UNSUPPORTED"], kw
    assert constrain(rows=None) == 0 and constrain(rows=None, seq_t=None, logits=None, bias=None, bias_b=7) == 0     # the no-op
    for kw in (dict(S=0), dict(S=-1), dict(N=0), dict(tokens=None), dict(logp=None), dict(entropy=None), dict(logits=None), dict(rows=None),
               dict(bias_b=3), dict(bias_b=0)):
        assert decode(**kw) == D["ERR_ARG"], kw
    for kw in (dict(n_cls=20), dict(n_cls=22), dict(S=D["MAX_S"] + 1), dict(N=D["MAX_N"] + 1)):
        assert decode(**kw) == D["ERR_UNSUPPORTED"], kw
    for kw in (dict(S=0), dict(N=0), dict(N=-1), dict(identity=None), dict(profile=None), dict(tokens=None), dict(mask=None),
               dict(recovery=None), dict(ref=None)):
        assert census(**kw) == D["ERR_ARG"], kw
    for kw in (dict(n_cls=20), dict(S=D["MAX_S"] + 1), dict(N=D["MAX_N"] + 1)):
        assert census(**kw) == D["ERR_UNSUPPORTED"], kw


def test_host_argument_checks_of_the_python_side():
    b, N = 2, 5
    seq, logits, bias, rows = torch.zeros(b, N, 21), torch.zeros(b, N, 21), torch.zeros(1, N, 21), torch.ones(b, N)
    tokens, mask = torch.zeros(b, N, dtype=torch.int32), torch.ones(N)
    with pytest.raises(RuntimeError, match="GPU only"):
        SQ.constrain_rows_(seq, logits, bias, rows)
    with pytest.raises(RuntimeError, match="GPU only"):
        SQ.decode(logits, rows)
    with pytest.raises(RuntimeError, match="GPU only"):
        SQ.census(tokens, mask)
    with pytest.raises(ValueError, match="float32"):
        SQ.constrain_rows_(seq, logits.double(), bias, rows)
    with pytest.raises(ValueError, match="logits must be"):
        SQ.constrain_rows_(seq, logits[0], bias, rows)
    with pytest.raises(ValueError, match="bias must be"):
        SQ.decode(logits, rows, bias=torch.zeros(3, N, 21))
    with pytest.raises(ValueError, match="bias must be"):
        SQ.decode(logits, rows, bias=torch.zeros(N, 21))
    with pytest.raises(ValueError, match="int32"):
        SQ.census(tokens.long(), mask)
    with pytest.raises(ValueError, match="tokens must be"):
        SQ.census(tokens[0], mask)
    with pytest.raises(ValueError, match=r"shape \(5,\)"):
        SQ.census(tokens, torch.ones(N + 1))
    assert "there is no CPU fallback" in SQ.__doc__


# ---- pipeline.generate_samples(sequence_rules=..., decode=...) ------------------------------------------------------------------------

class _RulesStub(_ScaffoldStub):
    """``_ScaffoldStub`` with the ``sequence_rules`` keyword: what it was given is recorded and applied to the stub's logits"""

    def __init__(self):
        super().__init__()
        self.rules = []

    def sample(self, batch, sources, redesign=None, scaffold=None, sequence_rules=None):
        self.rules.append(sequence_rules)
        pos, logits = super().sample(batch, sources, redesign=redesign, scaffold=scaffold)
        if sequence_rules is not None:
            batch.setdefault("residue_inv_extra_mask", batch["residue_mask"])
            logits = sequence_rules.apply(logits, sequence_rules.table(batch), sequence_rules.rows(batch))
        return pos, logits


def device_stand_ins():
    """the launchers of sequence.py replaced by their restatements: what generate_samples does with the numbers is what is under test"""
    def decode(logits, rows, bias=None, gumbel=None, temperature=0.0):
        tokens, logp, entropy = SQ.restate_decode(logits, rows, bias, gumbel, temperature)
        return tokens, logp.float(), entropy.float()

    def census(tokens, mask, ref_tokens=None, out=None):
        return SQ.restate_census(tokens, mask, ref_tokens)
    return {(SQ, "decode"): decode, (SQ, "census"): census}


def _generate(model, tmp, data=None, **kw):
    with warnings.catch_warnings(), contextlib.ExitStack() as stack:
        warnings.simplefilter("ignore", UserWarning)
        for (module, name), fn in list(fakes([]).items()) + list(device_stand_ins().items()):
            stack.enter_context(mock.patch.object(module, name, fn))
        return PL.generate_samples(model, complex_data() if data is None else data, num_samples=3, batch_size=2, seed=1, output_dir=tmp, **kw)


def test_sequence_options_are_refused_on_host_data_before_the_model_is_touched():
    full = complex_data()
    for rows in (NA + NR - 1, NA + NR + 1, NR):
        with pytest.raises(ValueError, match="does not fit"):
            PL.generate_samples(_NoDevice(), full, num_samples=2, sequence_rules=SequenceRules(torch.zeros(rows, 21)))
    with pytest.raises(TypeError, match="SequenceRules"):
        PL.generate_samples(_NoDevice(), full, num_samples=2, sequence_rules="C")
    with pytest.raises(TypeError, match="Decode"):
        PL.generate_samples(_NoDevice(), full, num_samples=2, decode="argmax")
    unknown = dict(full, residue_type=torch.full((NR,), -1, dtype=torch.long))
    with pytest.raises(ValueError, match="all unknown|is unknown"):
        PL.generate_samples(_NoDevice(), unknown, num_samples=2, decode=Decode(against="input"))
    with pytest.raises(AssertionError, match="the model was touched"):           # served: the model is reached
        PL.generate_samples(_NoDevice(), unknown, num_samples=2, decode=Decode())
    with pytest.raises(AssertionError, match="the model was touched"):
        PL.generate_samples(_NoDevice(), full, num_samples=2, sequence_rules=SequenceRules.for_residues(NA, NR), decode=Decode(0.5, "input"))
    with pytest.raises(ValueError, match="assess must be"):                     # the refusals that were there speak first
        PL.generate_samples(_NoDevice(), full, num_samples=2, assess="reference", sequence_rules=SequenceRules(torch.zeros(3, 21)))


def test_the_trailing_dict_comes_after_every_other_trailing_value_and_the_files_are_written(tmp_path):
    rules = SequenceRules.for_residues(NA, NR, omit="CM", allow={3: "AVLI"}, scope="all")
    spec = Scaffold(torch.ones(NA + NR), start=2)
    model = _RulesStub()
    full = _generate(model, tmp_path / "all", redesign=redesign_spec(), align_to="input", assess="input", scaffold=spec,
                     sequence_rules=rules, decode=Decode(0.7, "input"))
    assert len(full) == 9 and model.rules == [rules, rules] and model.seen == [spec, spec]
    used_mask, alignment, quality, kept, seqs = full[4:]
    assert used_mask.shape == (NA + NR,) and "tmscore" in alignment and "lddt_ca" in quality and "keep" in kept
    assert sorted(seqs) == ["diversity", "entropy", "identity", "logp", "profile", "recovery", "recovery_design", "sequences", "tokens"]
    tokens, logits = seqs["tokens"], full[1]
    assert tokens.shape == (3, NR) and tokens.dtype == np.int32 and seqs["logp"].shape == seqs["entropy"].shape == (3, NR)
    off = [SQ.ALPHABET.index(ch) for ch in "XCM"]
    assert (logits[:, NA:][:, :, off] == BANNED).all() and not np.isin(tokens, off).any() and (tokens >= 0).all()
    assert all(SQ.ALPHABET[c] in "AVLI" for c in tokens[:, 3])
    assert seqs["sequences"] == ["".join(SQ.ALPHABET[c] for c in row) for row in tokens]
    for k, prot in enumerate(full[2]):
        assert np.array_equal(prot.aatype, tokens[k].astype(np.int64) - 1)
    same = np.array([[(tokens[s] == tokens[r]).mean() for r in range(3)] for s in range(3)])
    assert seqs["identity"].dtype == np.float64 and np.array_equal(seqs["identity"], same)
    assert seqs["diversity"] == 1.0 - (same.sum() - 3.0) / 6.0
    assert np.array_equal(seqs["profile"], np.stack([(tokens == c).sum(0) for c in range(21)], 1)) and seqs["profile"].shape == (NR, 21)
    truth = np.asarray(complex_data()["residue_type"]) + 1
    assert (truth > 0).all() and np.array_equal(seqs["recovery"], (tokens == truth[None]).mean(1))
    design = used_mask[NA:] > 0.5
    assert int(design.sum()) == 3 and np.array_equal(seqs["recovery_design"], (tokens[:, design] == truth[design][None]).mean(1))
    assert sorted(os.listdir(tmp_path / "all")) == ["sample_alignment.npz", "sample_ligand_pos.npy", "sample_protein.pdb", "sample_quality.npz",
                                                    "sample_quality.txt", "sample_redesign_mask.npy", "sample_scaffold.npz",
                                                    "sample_sequences.fasta", "sample_sequences.npz", "sample_tmscores.txt"]
    fasta = (tmp_path / "all" / "sample_sequences.fasta").read_text().splitlines()
    assert fasta[1::2] == seqs["sequences"] and len(fasta) == 6
    assert fasta[0] == f">sample_0 mean_logp={float(seqs['logp'][0].mean()):.4f} recovery={seqs['recovery'][0]:.4f}"
    with np.load(tmp_path / "all" / "sample_sequences.npz") as z:
        assert sorted(z.files) == sorted(seqs) and np.array_equal(z["tokens"], tokens) and list(z["sequences"]) == seqs["sequences"]
    # every other value is what the same call returns without decode=; the proteins differ in their sequence alone
    plain = _generate(_RulesStub(), tmp_path / "plain", redesign=redesign_spec(), align_to="input", assess="input", scaffold=spec, sequence_rules=rules)
    assert len(plain) == 8 and "sample_sequences.npz" not in os.listdir(tmp_path / "plain")
    for a, b in zip(full[:2] + (full[3], full[4]), plain[:2] + (plain[3], plain[4])):
        assert np.array_equal(a, b)
    assert all(np.array_equal(alignment[k], plain[5][k]) for k in alignment) and np.array_equal(kept["keep"], plain[7]["keep"])
    # the same seed gives the same sequences; temperature 0 is the host argmax of the returned logits, which is what plain decodes
    again = _generate(_RulesStub(), tmp_path / "again", redesign=redesign_spec(), sequence_rules=rules, decode=Decode(0.7, "input"))
    assert len(again) == 6 and again[5]["sequences"] == seqs["sequences"]
    cold = _generate(_RulesStub(), tmp_path / "cold", sequence_rules=rules, decode=Decode())
    assert len(cold) == 5 and "recovery" not in cold[4] and np.array_equal(cold[4]["tokens"], cold[1][:, NA: NA + NR].argmax(-1))
    assert all(np.array_equal(cold[2][k].aatype, plain[2][k].aatype) for k in range(3))
    assert "recovery=" not in (tmp_path / "cold" / "sample_sequences.fasta").read_text()
    one = PL.generate_samples                   # S = 1: no pair to compare
    with contextlib.ExitStack() as stack, warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        for (module, name), fn in device_stand_ins().items():
            stack.enter_context(mock.patch.object(module, name, fn))
        single = one(_RulesStub(), complex_data(), num_samples=1, decode=Decode())
    assert math.isnan(single[4]["diversity"]) and single[4]["identity"].shape == (1, 1)


def test_without_the_keywords_nothing_reaches_the_model_and_nothing_changes(tmp_path):
    """sample_stubs._Stub has no ``sequence_rules`` parameter: a call without one (and one with None) must not pass the keyword, and
    returns and writes what it did; the gumbel draw of decode= comes after sample() has returned, so the samples are what they were"""
    want = torch.stack([torch.randn(NA + NR, 3, generator=NoiseSource(1, k).g) for k in range(3)]).numpy()
    for kw in ({}, dict(sequence_rules=None, decode=None)):
        out = _generate(_Stub(), tmp_path / "x", **kw)
        assert len(out) == 4 and np.array_equal(out[0], want)
        assert sorted(os.listdir(tmp_path / "x")) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
    with pytest.raises(TypeError, match="sequence_rules"):      # ... and with one it does reach it
        _generate(_Stub(), tmp_path / "y", sequence_rules=SequenceRules.for_residues(NA, NR))
    hot = _generate(_Stub(), tmp_path / "z", decode=Decode(1.5))
    assert len(hot) == 5 and np.array_equal(hot[0], want) and np.array_equal(hot[1], _generate(_Stub(), tmp_path / "w")[1])


def test_sample_sharded_and_predict_step_pass_the_keyword_only_when_given():
    from protein_redesign_amd.distributed import sample_sharded
    from protein_redesign_amd.synthetic import synthetic_batch
    batch = synthetic_batch([(NA, NR)], esm_dim=16, seed=8)
    seen = []

    def sampler(bt, sources, **kw):
        seen.append(kw)
        n = bt["atom_mask"].shape[1]
        return torch.zeros(len(sources), n, 3), torch.zeros(len(sources), n, 21)
    rules = SequenceRules.for_residues(NA, NR)
    sample_sharded(sampler, batch, 1)
    sample_sharded(sampler, batch, 1, sequence_rules=rules)
    sample_sharded(sampler, batch, 1, redesign=redesign_spec(), scaffold=Scaffold(), sequence_rules=rules)
    assert seen[0] == {} and seen[1] == {"sequence_rules": rules} and sorted(seen[2]) == ["redesign", "scaffold", "sequence_rules"]
    import inspect
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel, ReverseDiffusion
    for fn in (ProteinReDiffModel.sample, ProteinReDiffModel.predict_step, ReverseDiffusion.__init__, sample_sharded, PL.generate_samples):
        p = inspect.signature(fn).parameters
        assert "scaffold" in p and p["sequence_rules"].default is None, fn
