"""CPU: structure-conditioned sampling as far as it goes without a GPU -- the ``Scaffold`` spec and its refusals, the torch restatement
of the kernel against a float64 evaluation, the level table against the oracle's schedule, the header / build / export list of
libprd_condition.so, the refusals the library makes on the host, and the ``scaffold`` argument of pipeline.generate_samples with stub
models (what it returns, where, what it writes, and that nothing changes without it)."""
import contextlib
import ctypes
import os
import warnings
from unittest import mock

import numpy as np
import pytest
import torch

import prd_oracle as O
from conftest import ROOT
from protein_redesign_amd import _lib, build, conditioning, schedule
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.conditioning import Scaffold
from protein_redesign_amd.constants import make_args
from protein_redesign_amd.masking import Redesign
from protein_redesign_amd.synthetic import NoiseSource, synthetic_sample
from sample_stubs import _NoDevice, _Stub, header_entries
from test_generate_samples_combinations_cpu import NA, NR, complex_data, fakes, redesign_spec

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))


# ---- the spec ------------------------------------------------------------------------------------------------------------------------

def test_spec_is_validated_on_construction_and_immutable():
    s = Scaffold()
    assert (s.keep, s.ligand, s.sequence, s.start, s.radius) == ("outside", False, False, None, None) and not s.needs_ligand
    assert Scaffold("outside", ligand=True).needs_ligand and Scaffold.beyond(8).needs_ligand and Scaffold.beyond(0.0).radius == 0.0
    b = Scaffold.beyond(12.5, ligand=True, sequence=True, start=3)
    assert (b.radius, b.ligand, b.sequence, b.start) == (12.5, True, True, 3)
    m = torch.tensor([0, 1, 1, 0])
    t = Scaffold(m, start=0)
    assert t.keep.dtype == torch.float32 and t.keep.tolist() == [0, 1, 1, 0] and t.start == 0
    m[0] = 1
    assert t.keep.tolist() == [0, 1, 1, 0]                      # a copy: the caller's tensor is not the spec's
    assert Scaffold(torch.ones(2, 4)).keep.shape == (2, 4)
    p = Scaffold(None, start=5, sequence=True)
    assert p.keep is None and p.start == 5 and p.sequence
    with pytest.raises(Exception):                              # frozen
        s.start = 2
    assert t.to("cpu") is t and s.to("cpu") is s
    for bad in (torch.tensor([0.0, 0.5]), torch.tensor([0.0, 2.0]), torch.tensor([float("nan"), 1.0]), torch.tensor([-1.0, 1.0])):
        with pytest.raises(ValueError, match="only 0 and 1"):
            Scaffold(bad)
    with pytest.raises(ValueError, match=r"\[N\] or \[b, N\]"):
        Scaffold(torch.ones(2, 3, 4))
    for bad in (float("nan"), -1.0, float("inf"), -0.001):
        with pytest.raises(ValueError, match="radius"):
            Scaffold.beyond(bad)
    for bad in (-1, -7, 1.5, True):
        with pytest.raises(ValueError, match="start"):
            Scaffold("outside", start=bad)
    with pytest.raises(ValueError, match="keep=None"):
        Scaffold(None)
    with pytest.raises(ValueError, match="keep=None"):
        Scaffold(keep=None, sequence=True)
    with pytest.raises(ValueError, match="'outside'"):
        Scaffold("inside")


def test_rows_of_a_spec_on_a_prepared_batch():
    """K on host tensors for the kinds that need no kernel: 'outside', a mask (residues only), the ligand flag, nothing"""
    am = torch.tensor([[1.0, 1, 0, 0, 0, 0], [1.0, 0, 0, 0, 0, 0]])
    rm = torch.tensor([[0.0, 0, 1, 1, 1, 0], [0.0, 1, 1, 1, 1, 1]])
    extra = rm * torch.tensor([1.0, 1, 1, 0, 1, 1])
    batch = {"atom_mask": am, "residue_mask": rm, "residue_extra_mask": extra}
    assert torch.equal(Scaffold().rows(batch), extra)
    assert torch.equal(Scaffold("outside", ligand=True).rows(batch), extra + am)
    m = torch.tensor([1.0, 1, 1, 0, 0, 1])                     # ligand rows and padding marked: ignored
    assert torch.equal(Scaffold(m).rows(batch), rm * m)
    assert torch.equal(Scaffold(m, ligand=True).rows(batch), rm * m + am)
    assert torch.equal(Scaffold(torch.stack([m, 1 - m])).rows(batch), rm * torch.stack([m, 1 - m]))
    assert Scaffold(None, start=1).rows(batch) is None
    assert torch.equal(Scaffold(None, start=1, ligand=True).rows(batch), am)
    with pytest.raises(ValueError, match="does not fit"):
        Scaffold(torch.ones(5)).rows(batch)
    with pytest.raises(ValueError, match="does not fit"):
        Scaffold(torch.ones(3, 6)).rows(batch)


def test_the_model_refuses_a_scaffold_it_cannot_serve():
    """decided before any device work: the type, training mode, a start at or beyond num_steps"""
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    args = make_args(single_dim=128, pair_dim=64, num_blocks=1, esm_dim=64, num_steps=4)
    model = ProteinReDiffModel(args)
    assert model._scaffold_spec(None) is None and not hasattr(model, "scaffold")
    s = Scaffold(None, start=3)
    assert model._scaffold_spec(s) is s
    for start in (4, 5, 64):
        with pytest.raises(ValueError, match="start"):
            model._scaffold_spec(Scaffold("outside", start=start))
    with pytest.raises(TypeError, match="Scaffold"):
        model._scaffold_spec("outside")
    with pytest.raises(TypeError, match="Scaffold"):
        model.sample({}, sources=[], scaffold=Redesign.within(8.0))
    model.training_mode = True
    with pytest.raises(ValueError, match="training_mode"):
        model._scaffold_spec(Scaffold())
    with pytest.raises(ValueError, match="training_mode"):
        model.sample({}, sources=[], scaffold=Scaffold())


# ---- the restatement and the level table ------------------------------------------------------------------------------------------------

def restate_case(b, N, levels, T, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)       # noqa: E731
    tab = schedule.schedule_tables(T, "linear")
    return dict(z=r(b, N, 3), seq_t=r(b, N, 21), x0c=3.0 * r(b, N, 3), noise=r(levels, b, N, 3), level=conditioning.level_table(tab),
                seq0=r(b, N, 21), keep_z=(torch.rand(b, N, generator=g) < 0.6).float(), keep_seq=(torch.rand(b, N, generator=g) < 0.4).float())


def test_restatement_against_float64():
    """Every level of a schedule: the kept rows equal A x0c + S eps evaluated in float64 from the same fp32 operands to within the three
    fp32 roundings of the restatement -- 2^-24 (|A x| + |S e| + |sum|) <= 2^-23 (|A x| + |S e|), ONE ulp at the magnitude of the terms,
    by construction --, level -1 gives x0c itself, a level the noise table does not hold leaves the sample alone, and every other row
    is untouched."""
    b, N, levels, T = 4, 37, 6, 8
    c = restate_case(b, N, levels, T, 3)
    kw = {k: c[k] for k in ("x0c", "keep_z", "noise", "level", "seq0", "keep_seq")}
    for base in range(-1, levels + 1):
        t = torch.tensor([base, -1, levels - 1, levels + 2])
        z, seq = conditioning.restate_rows(c["z"], c["seq_t"], t, **kw)
        assert z is not c["z"] and seq is not c["seq_t"]
        for s in range(b):
            rows, l = c["keep_z"][s] >= 0.5, int(t[s])
            assert torch.equal(z[s, ~rows], c["z"][s, ~rows])
            if l >= levels:
                assert torch.equal(z[s], c["z"][s])
            elif l < 0:
                assert torch.equal(z[s, rows], c["x0c"][s, rows])
            else:
                a = c["level"][l, 0].double() * c["x0c"][s, rows].double()
                n = c["level"][l, 1].double() * c["noise"][l, s, rows].double()
                err = (z[s, rows].double() - (a + n)).abs()
                assert bool((err <= 2.0 ** -23 * (a.abs() + n.abs())).all()), (l, float(err.max()))
        ks = c["keep_seq"] >= 0.5
        assert torch.equal(seq[ks], c["seq0"][ks]) and torch.equal(seq[~ks], c["seq_t"][~ks])
    # each half alone; what is not asked for comes back as it went in
    t = torch.zeros(b, dtype=torch.int64)
    z, seq = conditioning.restate_rows(c["z"], c["seq_t"], t, seq0=c["seq0"], keep_seq=c["keep_seq"])
    assert torch.equal(z, c["z"]) and not torch.equal(seq, c["seq_t"])
    z, seq = conditioning.restate_rows(c["z"], None, t, x0c=c["x0c"], keep_z=c["keep_z"], noise=c["noise"], level=c["level"])
    assert seq is None and not torch.equal(z, c["z"])


@pytest.mark.parametrize("kind", ["linear", "cosine"])
@pytest.mark.parametrize("T", [1, 4, 64])
def test_level_table_equals_the_oracle_schedule(kind, T):
    want = O.schedule_tables(T, kind)
    got = conditioning.level_table(schedule.schedule_tables(T, kind))
    assert got.shape == (T, 2) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got[:, 0], want["sqrt_alphas_cumprod"]) and torch.equal(got[:, 1], want["sqrt_one_minus_alphas_cumprod"])


# ---- header, build, export list -------------------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    from protein_redesign_amd import align, quality, tmalign
    e = header_entries("condition")
    assert sorted(e) == ["prd_condition_rows", "prd_condition_version"]
    assert all(x.inject is None and x.restype is _lib.ci for x in e.values())
    assert e["prd_condition_rows"].argtypes == [_lib.vp] * 9 + [_lib.ci] * 4 + [_lib.vp] and e["prd_condition_version"].argtypes == []
    assert conditioning.ENTRIES == e
    assert not set(e) & (set(_lib.ENTRIES) | set(align.ENTRIES) | set(tmalign.ENTRIES) | set(quality.ENTRIES))
    assert conditioning.ABI_VERSION == conditioning._DEFINES["VERSION"] == 100 and conditioning.N_CLS == 21
    assert conditioning._DEFINES["ERR_ARG"] == -1 and conditioning._DEFINES["ERR_UNSUPPORTED"] == -3
    with open(os.path.join(ROOT, "protein_redesign_amd", "csrc", "prd_condition.hip")) as f:
        assert '#include "prd_launch.h"' in f.read()         # the host half of its launch is the project's one


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_new_kernel():
    mine = build.resource_usage(sources=build.SIDE_LIBS["condition"].sources)
    assert sorted(mine) == ["condition_rows_kernel"]
    u = mine["condition_rows_kernel"]
    assert u["scratch"] == 0 and u["agprs"] == 0 and u["lds"] == 0 and u["occupancy"] == 8


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_library_refuses_on_the_host_before_any_device_call():
    """the refusals of prd_condition.h are host code that runs before the first HIP call: every one of them is reachable without a GPU,
    with pointers that are never followed"""
    build.build_side("condition", verbose=False)
    L, D = conditioning.lib(), conditioning._DEFINES
    assert L.prd_condition_version() == 100
    p = ctypes.c_void_p(4096)

    def rows(z=p, seq_t=p, t=p, x0c=p, keep_z=p, noise=p, level=p, seq0=p, keep_seq=p, b=2, N=5, n_cls=21, levels=3):
        return L.prd_condition_rows(z, seq_t, t, x0c, keep_z, noise, level, seq0, keep_seq, b, N, n_cls, levels, None)
    for kw in (dict(b=0), dict(b=-1), dict(N=0), dict(N=-4), dict(levels=0), dict(levels=-1), dict(t=None), dict(z=None), dict(x0c=None),
               dict(noise=None), dict(level=None), dict(seq_t=None), dict(seq0=None)):
        assert rows(**kw) == D["ERR_ARG"], kw
    for kw in (dict(n_cls=20), dict(n_cls=22), dict(n_cls=0), dict(b=D["MAX_B"] + 1), dict(N=D["MAX_N"] + 1)):
        assert rows(**kw) == D["ERR_UNSUPPORTED"], kw
    # nothing to hold: a successful no-op, whatever n_cls and the tensors of the absent masks are
    assert rows(keep_z=None, keep_seq=None, z=None, seq_t=None, x0c=None, noise=None, level=None, seq0=None, n_cls=7) == 0


def test_host_argument_checks_of_the_python_side():
    b, N = 2, 5
    z, seq, t = torch.zeros(b, N, 3), torch.zeros(b, N, 21), torch.zeros(b, dtype=torch.int64)
    keep = torch.ones(b, N)
    with pytest.raises(RuntimeError, match="GPU only"):
        conditioning.condition_rows_(z, seq, t, seq0=seq, keep_seq=keep)
    with pytest.raises(ValueError, match="int64"):
        conditioning.condition_rows_(z, seq, t.int(), seq0=seq, keep_seq=keep)
    with pytest.raises(ValueError, match=r"shape \(2,\)"):
        conditioning.condition_rows_(z, seq, torch.zeros(3, dtype=torch.int64), seq0=seq, keep_seq=keep)
    with pytest.raises(ValueError, match="must be given"):
        conditioning.condition_rows_(None, None, t)
    with pytest.raises(ValueError, match="needs noise"):
        conditioning.condition_rows_(z, seq, t, x0c=z, keep_z=keep)
    assert "there is no\nCPU fallback" in conditioning.__doc__ and "doubles" in __import__(
        "protein_redesign_amd.diffusion_model", fromlist=["ReverseDiffusion"]).ReverseDiffusion.__doc__


# ---- pipeline.generate_samples(scaffold=...) ------------------------------------------------------------------------------------------

class _ScaffoldStub(_Stub):
    """``_Stub`` with the ``scaffold`` keyword: what it was given is recorded, and the kept rows are left in the batch where the real loop
    leaves them"""

    def __init__(self):
        self.seen = []

    def sample(self, batch, sources, redesign=None, scaffold=None):
        self.seen.append(scaffold)
        out = super().sample(batch, sources, redesign=redesign)
        if scaffold is not None:
            keep = scaffold.rows(dict(batch, residue_extra_mask=batch["residue_mask"] - batch.get("residue_inv_extra_mask", 0)))
            batch[conditioning.BATCH_KEY] = keep if keep is not None else torch.zeros_like(batch["residue_mask"])
        return out


def test_scaffold_is_refused_on_host_data_before_the_model_is_touched():
    full = complex_data()
    lig = {k: v for k, v in full.items() if k.startswith(("atom_", "bond_")) or k == "num_atoms"}
    bare = PL.protein_to_data(PL.protein_from_sequence("ACDEFGHIK"), **lig)
    for spec in (Scaffold(), Scaffold(None, start=2), Scaffold.beyond(8.0), Scaffold(torch.ones(NA + NR), ligand=True)):
        with pytest.raises(ValueError, match="coordinates"):
            PL.generate_samples(_NoDevice(), bare, num_samples=2, scaffold=spec)
        with pytest.raises(ValueError, match="C-alpha"):
            PL.generate_samples(_NoDevice(), dict(full, residue_atom_mask=torch.zeros(NR, 37)), num_samples=2, scaffold=spec)
    no_ligand = {k: v for k, v in full.items() if k != "atom_pos"}
    for data in (no_ligand, dict(full, num_atoms=0)):
        for spec in (Scaffold("outside", ligand=True), Scaffold.beyond(8.0), Scaffold(None, start=1, ligand=True)):
            with pytest.raises(ValueError, match="ligand"):
                PL.generate_samples(_NoDevice(), data, num_samples=2, scaffold=spec)
    with pytest.raises(TypeError, match="Scaffold"):
        PL.generate_samples(_NoDevice(), full, num_samples=2, scaffold="outside")
    with pytest.raises(AssertionError, match="the model was touched"):           # without ligand positions 'outside' alone is served
        PL.generate_samples(_NoDevice(), no_ligand, num_samples=2, redesign=redesign_spec(), scaffold=Scaffold())
    # the refusals that were there speak first
    with pytest.raises(ValueError, match="assess must be"):
        PL.generate_samples(_NoDevice(), bare, num_samples=2, assess="reference", scaffold=Scaffold())
    with pytest.raises(ValueError, match="align_to='input'"):
        PL.generate_samples(_NoDevice(), bare, num_samples=2, align_to="input", scaffold=Scaffold())
    with pytest.raises(ValueError, match="Redesign.within"):                   # and a pocket is still refused where the scaffold is served
        PL.generate_samples(_NoDevice(), dict(full, num_atoms=0), num_samples=2, redesign=Redesign.within(8.0), scaffold=Scaffold())


def _generate(model, tmp, **kw):
    with warnings.catch_warnings(), contextlib.ExitStack() as stack:
        warnings.simplefilter("ignore", UserWarning)
        for (module, name), fn in fakes([]).items():
            stack.enter_context(mock.patch.object(module, name, fn))
        return PL.generate_samples(model, complex_data(), num_samples=3, batch_size=2, seed=1, output_dir=tmp, **kw)


def test_the_trailing_dict_comes_after_every_other_trailing_value_and_the_file_is_written(tmp_path):
    keep = torch.zeros(NA + NR)
    keep[[0, NA + 1, NA + 2, NA + NR - 1]] = 1                  # a ligand atom (ignored) and three residues
    spec = Scaffold(keep, ligand=True, sequence=True, start=7)
    model = _ScaffoldStub()
    full = _generate(model, tmp_path / "all", redesign=redesign_spec(), align_to="input", assess="input", scaffold=spec)
    assert len(full) == 8 and model.seen == [spec, spec]        # two batches, the spec as it was given
    used_mask, alignment, quality, kept = full[4:]
    assert used_mask.shape == (NA + NR,) and "tmscore" in alignment and "lddt_ca" in quality
    want = np.zeros(NA + NR, np.float32)
    want[:NA] = 1
    want[[NA + 1, NA + 2, NA + NR - 1]] = 1
    assert sorted(kept) == ["keep", "ligand", "sequence", "start"]
    assert np.array_equal(kept["keep"], want) and kept["keep"].dtype == np.float32
    assert (kept["ligand"], kept["sequence"], kept["start"]) == (True, True, 7)
    assert sorted(os.listdir(tmp_path / "all")) == ["sample_alignment.npz", "sample_ligand_pos.npy", "sample_protein.pdb", "sample_quality.npz",
                                                    "sample_quality.txt", "sample_redesign_mask.npy", "sample_scaffold.npz", "sample_tmscores.txt"]
    with np.load(tmp_path / "all" / "sample_scaffold.npz") as z:
        assert sorted(z.files) == ["keep", "ligand", "sequence", "start"] and np.array_equal(z["keep"], want)
        assert bool(z["ligand"]) and bool(z["sequence"]) and int(z["start"]) == 7
    # every other value is what the same call returns without a scaffold
    plain = _generate(_ScaffoldStub(), tmp_path / "plain", redesign=redesign_spec(), align_to="input", assess="input")
    assert len(plain) == 7 and "sample_scaffold.npz" not in os.listdir(tmp_path / "plain")
    for a, b in zip(full[:2] + (full[4],), plain[:2] + (plain[4],)):
        assert np.array_equal(a, b)
    assert all(np.array_equal(alignment[k], plain[5][k]) for k in alignment) and all(np.array_equal(quality[k], plain[6][k], equal_nan=True) for k in quality)
    # alone: right after the four values; 'outside' follows the design region, start None is -1 in the file
    alone = _generate(_ScaffoldStub(), tmp_path / "alone", scaffold=Scaffold())
    assert len(alone) == 5 and alone[4]["start"] is None and np.array_equal(alone[4]["keep"], np.r_[np.zeros(NA), np.ones(NR)].astype(np.float32))
    with np.load(tmp_path / "alone" / "sample_scaffold.npz") as z:
        assert int(z["start"]) == -1 and not bool(z["ligand"])
    region = _generate(_ScaffoldStub(), tmp_path / "region", redesign=redesign_spec(), scaffold=Scaffold())
    assert len(region) == 6 and np.array_equal(region[5]["keep"][NA:], 1 - region[4][NA:]) and not region[5]["keep"][:NA].any()
    nothing = _generate(_ScaffoldStub(), tmp_path / "partial", scaffold=Scaffold(None, start=0))
    assert not nothing[4]["keep"].any() and nothing[4]["start"] == 0


def test_without_a_scaffold_the_keyword_does_not_reach_the_model(tmp_path):
    """sample_stubs._Stub has no ``scaffold`` parameter: a call without one (and one with scaffold=None) must not pass the keyword, and
    returns and writes what it did"""
    data = synthetic_sample(NA, NR, esm_dim=16, seed=8)
    want = torch.stack([torch.randn(NA + NR, 3, generator=NoiseSource(1, k).g) for k in range(3)]).numpy()
    for kw in ({}, dict(scaffold=None)):
        out = _generate(_Stub(), tmp_path, **kw)
        assert len(out) == 4 and np.array_equal(out[0], want)
        assert sorted(os.listdir(tmp_path)) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
    a = _generate(_Stub(), tmp_path / "a", redesign=redesign_spec(), assess="self")
    b = _generate(_Stub(), tmp_path / "b", redesign=redesign_spec(), assess="self", scaffold=None)
    assert len(a) == len(b) == 6 and all(np.array_equal(x, y) for x, y in zip(a[:2] + (a[4],), b[:2] + (b[4],)))
    with pytest.raises(TypeError, match="scaffold"):            # ... and with one it does reach it
        _generate(_Stub(), tmp_path / "c", scaffold=Scaffold())


def test_sample_sharded_passes_the_keyword_only_when_given():
    from protein_redesign_amd.distributed import sample_sharded
    from protein_redesign_amd.synthetic import synthetic_batch
    batch = synthetic_batch([(NA, NR)], esm_dim=16, seed=8)
    seen = []

    def sampler(bt, sources, **kw):
        seen.append(kw)
        n = bt["atom_mask"].shape[1]
        return torch.zeros(len(sources), n, 3), torch.zeros(len(sources), n, 21)
    spec = Scaffold()
    sample_sharded(sampler, batch, 2)
    sample_sharded(sampler, batch, 2, scaffold=spec)
    sample_sharded(sampler, batch, 2, redesign=redesign_spec(), scaffold=spec)
    assert seen[:2] == [{}, {}] and seen[2:4] == [{"scaffold": spec}] * 2 and sorted(seen[4]) == ["redesign", "scaffold"]
