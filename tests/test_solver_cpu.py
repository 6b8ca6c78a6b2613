"""CPU: few-step sampling as far as it goes without a GPU -- the ``Solver`` spec, its levels and refusals, its tables against the
float64 restatement of tests/solver_ref.py, the identities between the kinds, the draws a solver loop makes, the header / build of
libprd_solver.so and its host refusals, the ``solver=`` keyword through pipeline.generate_samples and distributed.sample_sharded, and
the oracle's own fp32 run of every loop the GPU test uses against its float64 run."""
import ctypes
import os

import numpy as np
import pytest
import torch

import solver_ref as R
from conftest import ROOT, rel_l2
from protein_redesign_amd import _lib, build, diffusion_model, schedule, solver
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.conditioning import Scaffold
from protein_redesign_amd.constants import make_args
from protein_redesign_amd.solver import Solver
from protein_redesign_amd.synthetic import NoiseSource
from sample_stubs import _NoDevice, _Stub, header_entries
from test_conditioning_cpu import _generate
from test_generate_samples_combinations_cpu import NA, NR

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))


# ---- levels ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [2, 16, 1000])
def test_spacing_rule_end_points_and_monotonicity(T):
    tops = sorted({T - 1, (T - 1) // 2, 1})
    for top in tops:
        for K in range(1, top + 2):
            lv = solver.spaced_levels(K, top)
            assert lv == R.levels(K, top) and len(lv) == K and lv[-1] == top
            assert K == 1 or lv[0] == 0
            assert all(a < b for a, b in zip(lv, lv[1:])), (T, top, K)
    assert Solver.ancestral(T).levels(T) == list(range(T)) == Solver.ddim(T).levels(T)
    assert Solver.ddim(1).levels(T) == [T - 1]
    with pytest.raises(ValueError, match="do not fit"):
        Solver.ddim(T + 1).levels(T)
    with pytest.raises(ValueError, match="do not fit"):
        Solver.ancestral(3).levels(T, top=1)


def test_spec_is_validated_and_immutable():
    s = Solver.ddim(50)
    assert (s.kind, s.eta, s.steps, s.timesteps, s.K, s.stochastic) == ("ddim", 0.0, 50, None, 50, False)
    a = Solver.ancestral(50, variance="posterior")
    assert (a.kind, a.variance, a.stochastic) == ("ancestral", "posterior", True)
    e = Solver(timesteps=[15, 9, 2], kind="ddim", eta=0.25)
    assert e.timesteps == (15, 9, 2) and e.K == 3 and e.stochastic and e.levels(16) == [2, 9, 15]
    assert Solver(timesteps=torch.tensor([7, 3])).levels(16) == [3, 7]
    assert not Solver.ancestral(1).stochastic and not Solver(timesteps=[4]).stochastic and Solver.ddim(2, eta=1.0).stochastic
    with pytest.raises(Exception):                              # frozen
        s.eta = 1.0
    for bad in ([3, 3], [2, 9], [5, -1], [], [1.5, 0]):
        with pytest.raises(ValueError, match="timesteps"):
            Solver(timesteps=bad)
    with pytest.raises(ValueError, match=r"lie in \[0, 15\]"):
        Solver(timesteps=[16, 3]).levels(16)
    with pytest.raises(ValueError, match="first of the timesteps must be 9"):
        Solver(timesteps=[15, 9, 2], kind="ddim").levels(16, top=9)
    assert Solver(timesteps=[9, 2], kind="ddim").levels(16, top=9) == [2, 9]
    for kw, what in ((dict(kind="heun"), "kind"), (dict(variance="fixed"), "variance"), (dict(kind="ddim", eta=-0.1), "eta"),
                     (dict(kind="ddim", eta=float("nan")), "eta"), (dict(eta=0.5), "eta belongs"),
                     (dict(kind="ddim", variance="posterior"), "variance belongs")):
        with pytest.raises(ValueError, match=what):
            Solver(timesteps=[3, 1], **kw)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            Solver.ddim(bad)
    with pytest.raises(ValueError, match="not both or neither"):
        Solver()
    with pytest.raises(ValueError, match="not both or neither"):
        Solver(timesteps=[3, 1], steps=2)
    assert "ddim" in repr(s) and "posterior" in repr(a)


def test_the_model_refuses_a_solver_it_cannot_serve():
    """decided before any device work or library call: the type, training mode, the time embedding, levels outside the schedule"""
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    model = ProteinReDiffModel(make_args(single_dim=128, pair_dim=64, num_blocks=1, esm_dim=64, num_steps=4))
    s = Solver.ddim(3)
    assert model._solver_spec(None) is None and model._solver_spec(s) is s and not hasattr(model, "solver")
    with pytest.raises(TypeError, match="Solver"):
        model._solver_spec("ddim")
    with pytest.raises(TypeError, match="Solver"):
        model.sample({}, sources=[], solver=50)
    with pytest.raises(ValueError, match="do not fit"):
        model.sample({}, sources=[], solver=Solver.ddim(5))
    with pytest.raises(ValueError, match="do not fit"):
        model._solver_spec(Solver.ddim(3), Scaffold(None, start=1))
    with pytest.raises(ValueError, match="first of the timesteps"):
        model._solver_spec(Solver(timesteps=[3, 0]), Scaffold(None, start=2))
    model.training_mode = True
    with pytest.raises(ValueError, match="training_mode"):
        model.sample({}, sources=[], solver=s)
    wide = ProteinReDiffModel(make_args(single_dim=128, pair_dim=64, num_blocks=1, esm_dim=64, num_steps=4, time_dim=1024))
    with pytest.raises(ValueError, match=r"solver.*time_dim.*512.*time_dim = 1024"):
        wide.sample({}, sources=[], solver=s)


# ---- tables ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["linear", "cosine"])
@pytest.mark.parametrize("T", [2, 16, 1000])
def test_full_length_ancestral_rows_are_the_models_own(T, kind):
    """the special case: (w, a, c) of Solver.ancestral(T) are the rows of schedule.reverse_coefficients, bit for bit; the float64
    formulas agree with them to fp32 rounding, and the other two columns are the formulas'"""
    coef = schedule.reverse_coefficients(schedule.schedule_tables(T, kind))
    lv, tab = Solver.ancestral(T).tables(T, kind, coef=coef)
    assert lv.dtype == torch.int64 and lv.tolist() == list(range(T)) and tab.shape == (T, 8) and tab.dtype == torch.float32
    assert torch.equal(tab[:, :3], coef[:, :3]) and float(tab[:, 5:].abs().max()) == 0.0
    assert torch.equal(Solver.ancestral(T).tables(T, kind)[1], tab)            # computed as the model computes it when not handed over
    c64 = Solver.ancestral(T).coefficients64(T, kind)
    want = torch.tensor(R.coefficients(list(range(T)), R.abar(T, kind), "ancestral"), dtype=torch.float64)
    assert float((c64 - want).abs().max()) <= 1e-12
    assert torch.equal(tab[:, 3:5], c64[:, 3:5].float())
    assert float((c64[1:, :3] - coef[1:, :3].double()).abs().max()) <= 2e-6     # fp32 tables against float64 formulas
    # anything else is computed: one level fewer, or the other variance
    if T > 2:
        assert not torch.equal(Solver.ancestral(T - 1).tables(T, kind)[1][:, :3], coef[1:, :3])
        assert not torch.equal(Solver.ancestral(T, variance="posterior").tables(T, kind)[1][:, :3], coef[:, :3])


@pytest.mark.parametrize("T,K", [(16, 4), (16, 16), (1000, 50), (1000, 7)])
def test_tables_against_the_restatement_and_the_identities(T, K):
    ab = R.abar(T)
    for s, (kind, eta, variance) in ((Solver.ddim(K), ("ddim", 0.0, "beta")), (Solver.ddim(K, eta=0.5), ("ddim", 0.5, "beta")),
                                     (Solver.ancestral(K), ("ancestral", 0.0, "beta")),
                                     (Solver.ancestral(K, variance="posterior"), ("ancestral", 0.0, "posterior"))):
        got = s.coefficients64(T, "linear")
        want = torch.tensor(R.coefficients(R.levels(K, T - 1), ab, kind, eta, variance), dtype=torch.float64)
        assert got.shape == (K, 5) and float((got - want).abs().max()) <= 1e-12
        assert float(got[0, 2]) == 0.0                          # no noise at the last counter, whatever the kind
        assert abs(float(got[:, 1].prod()) - 1.0 / np.sqrt(ab[T - 1])) <= 1e-12 / np.sqrt(ab[T - 1]) * 10     # prod a = 1 / sqrt(abar_top)
        lv, tab = s.tables(T, "linear")
        if not s.full_length(lv.tolist(), T):
            assert torch.equal(tab[:, :5], got.float())         # rounded once
    one, post = Solver.ddim(K, eta=1.0).coefficients64(T, "linear"), Solver.ancestral(K, variance="posterior").coefficients64(T, "linear")
    assert float((one - post).abs().max()) <= 1e-12
    assert float(Solver.ddim(K).coefficients64(T, "linear")[:, 2].abs().max()) == 0.0
    assert bool((Solver.ddim(K, eta=0.3).coefficients64(T, "linear")[1:, 2] > 0).all())


def test_product_of_a_to_1e_12():
    for T, s in ((1000, Solver.ddim(50)), (1000, Solver.ancestral(13)), (16, Solver(timesteps=[12, 9, 2], kind="ddim"))):
        ab, a = R.abar(T), s.coefficients64(T, "linear")[:, 1]
        top = s.levels(T)[-1]
        assert abs(float(a.prod()) * np.sqrt(ab[top]) - 1.0) <= 1e-12


@pytest.mark.parametrize("T,lv", [(1000, R.levels(50, 999)), (16, R.levels(4, 15)), (1000, [0, 3, 4, 97, 500, 501, 998])])
def test_deterministic_loop_on_the_true_noise_returns_x0(T, lv):
    """float64, the package's own coefficients: z_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) e with one e throughout, the loop fed that e"""
    g = torch.Generator().manual_seed(5)
    x0, e = torch.randn(9, 3, generator=g, dtype=torch.float64), torch.randn(9, 3, generator=g, dtype=torch.float64)
    ab = torch.tensor(R.abar(T), dtype=torch.float64)
    s = Solver(timesteps=lv[::-1], kind="ddim")
    assert s.levels(T) == lv
    co = s.coefficients64(T, "linear")
    z = ab[lv[-1]].sqrt() * x0 + (1 - ab[lv[-1]]).sqrt() * e
    for k in range(len(lv) - 1, -1, -1):
        x0_hat = co[k, 4] * (z - co[k, 3] * e)
        assert float((x0_hat - x0).abs().max()) <= 1e-10        # the estimate of every step is x0 as well
        z = co[k, 1] * (z - co[k, 0] * e)
    assert float((z - x0).abs().max()) <= 1e-10
    assert float((R.ddim_true_noise_loop(x0, e, lv, R.abar(T)) - x0).abs().max()) <= 1e-10


# ---- draw accounting ------------------------------------------------------------------------------------------------------------------

class _Counting:
    """a noise source that records the shape of every draw"""

    def __init__(self):
        self.src, self.shapes = NoiseSource(1, 0), []

    def randn(self, *shape):
        self.shapes.append(tuple(shape))
        return self.src.randn(*shape)


def _drawn(spec, T, scaffold=None, N=6):
    src = _Counting()
    z0, s0, noise = diffusion_model.draw_loop_noise([src], N, diffusion_model.update_noise_rows(spec, T))
    if scaffold is not None:
        diffusion_model.draw_conditioning_noise([src], N, diffusion_model.conditioning_noise_rows(spec, T, scaffold.start))
    return src.shapes, z0, s0, noise


def test_draw_accounting():
    T, N = 16, 6
    head = [(N, 3), (N, 21)]
    shapes, z0, s0, noise = _drawn(None, T)
    assert shapes == head + [(N, 3)] * (T - 1) and noise.shape == (T - 1, 1, N, 3)        # what it consumed
    plain = NoiseSource(1, 0)
    assert torch.equal(z0[0], plain.randn(N, 3)) and torch.equal(s0[0], plain.randn(N, 21)) and torch.equal(noise[0, 0], plain.randn(N, 3))
    shapes, _, _, noise = _drawn(Solver.ddim(5), T)
    assert shapes == head and noise is None                     # z_T and seq_T only: no table
    shapes, z1, _, noise = _drawn(Solver.ancestral(5), T)
    assert shapes == head + [(N, 3)] * 4 and noise.shape == (4, 1, N, 3) and torch.equal(z1, z0)
    assert _drawn(Solver.ddim(5, eta=0.5), T)[0] == head + [(N, 3)] * 4
    assert _drawn(Solver.ancestral(1), T)[0] == head
    # a scaffold adds one draw per visited level, after everything else
    assert _drawn(Solver.ddim(5), T, Scaffold())[0] == head + [(N, 3)] * 5
    assert _drawn(Solver.ancestral(5), T, Scaffold())[0] == head + [(N, 3)] * (4 + 5)
    assert _drawn(Solver.ancestral(4), T, Scaffold(None, start=9))[0] == head + [(N, 3)] * (3 + 4)
    assert _drawn(None, T, Scaffold())[0] == head + [(N, 3)] * (T - 1 + T)
    assert _drawn(None, T, Scaffold(None, start=9))[0] == head + [(N, 3)] * (T - 1 + 10)


# ---- header, build, host refusals -----------------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    e = header_entries("solver")
    assert sorted(e) == ["prd_solver_boundary", "prd_solver_version"]
    assert all(x.inject is None and x.restype is _lib.ci for x in e.values())
    assert e["prd_solver_boundary"].argtypes == [_lib.vp] * 19 + [_lib.ci] * 8 + [_lib.vp, _lib.ci, _lib.vp, _lib.ci, _lib.vp]
    assert solver.ENTRIES == e and not set(e) & set(_lib.ENTRIES)
    assert solver.ABI_VERSION == solver._DEFINES["VERSION"] == 100 and solver._DEFINES["N_CLS"] == 21 and solver.MAX_TIME_DIM == 512
    assert solver.COEF_STRIDE == 8
    with open(os.path.join(ROOT, "protein_redesign_amd", "csrc", "prd_solver.hip")) as f:
        text = f.read()
    assert '#include "prd_launch.h"' in text and "hipLaunchKernelGGL" not in text and "<<<" not in text and "asm" not in text


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_one_kernel():
    mine = build.resource_usage(sources=build.SIDE_LIBS["solver"].sources)
    assert sorted(mine) == ["solver_boundary_kernel<21>"]
    u = mine["solver_boundary_kernel<21>"]
    assert u["scratch"] == 0 and u["agprs"] == 0 and 0 < u["lds"] <= 4096


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_library_refuses_on_the_host_before_any_device_call():
    """every refusal of prd_solver.h is host code that runs before the first HIP call: reachable without a GPU, with pointers that are
    never followed"""
    build.build_side("solver", verbose=False)
    L, D = solver.lib(), solver._DEFINES
    assert L.prd_solver_version() == 100
    p = ctypes.c_void_p(4096)
    names = ["z", "seq_t", "k", "t", "eps_raw", "seq_pred", "noise", "mask", "levels", "coef", "single_next", "static_single",
             "residue_mask", "w_rt", "ebeta_next", "freqs", "w_beta", "sync", "x0_out"]

    def call(b=2, N=5, n_cls=21, K=4, num_steps=16, S=128, P=64, time_dim=64, seq_h=p, ldh=128, w_seq=p, S_h=128, **ptrs):
        args = [ptrs.get(n, p) for n in names]
        return L.prd_solver_boundary(*args, b, N, n_cls, K, num_steps, S, P, time_dim, seq_h, ldh, w_seq, S_h, None)
    for n in names:
        if n not in ("noise", "x0_out"):                       # these two may be NULL
            assert call(**{n: None}) == D["ERR_ARG"], n
    for kw in (dict(b=0), dict(N=0), dict(K=0), dict(b=-1), dict(N=-3), dict(K=-1), dict(S=0), dict(P=0), dict(num_steps=0),
               dict(w_seq=None), dict(S_h=0)):
        assert call(**kw) == D["ERR_ARG"], kw
    for kw in (dict(n_cls=20), dict(n_cls=22), dict(time_dim=63), dict(time_dim=514), dict(time_dim=1024), dict(time_dim=0),
               dict(b=D["MAX_B"] + 1), dict(N=D["MAX_N"] + 1), dict(K=D["MAX_K"] + 1), dict(S=D["MAX_S"] + 1), dict(P=D["MAX_P"] + 1)):
        assert call(**kw) == D["ERR_UNSUPPORTED"], kw
    for kw in (dict(S_h=126), dict(ldh=130), dict(ldh=124)):
        assert call(**kw) == D["ERR_ALIGN"], kw
    # the launch geometry the bounds promise: the grid and the kernel's int row index stay below 2^31
    assert D["MAX_B"] * (D["MAX_N"] // 8 + D["MAX_P"] // 4 + 2) < 2 ** 31 and D["MAX_B"] * D["MAX_N"] <= 2 ** 30


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------

class _SolverStub(_Stub):
    def __init__(self):
        self.seen = []

    def sample(self, batch, sources, redesign=None, solver=None):
        self.seen.append(solver)
        return super().sample(batch, sources, redesign=redesign)


def test_generate_samples_hands_the_solver_through_and_changes_nothing_without_it(tmp_path):
    spec = Solver.ddim(4)
    model = _SolverStub()
    out = _generate(model, tmp_path / "with", solver=spec)
    assert len(out) == 4 and model.seen == [spec, spec] and all(s is spec for s in model.seen)
    want = torch.stack([torch.randn(NA + NR, 3, generator=NoiseSource(1, k).g) for k in range(3)]).numpy()
    for kw in ({}, dict(solver=None)):                          # _Stub has no ``solver`` parameter: the keyword must not reach it
        plain = _generate(_Stub(), tmp_path / "plain", **kw)
        assert len(plain) == 4 and np.array_equal(plain[0], want) and np.array_equal(plain[0], out[0]) and np.array_equal(plain[1], out[1])
    assert sorted(os.listdir(tmp_path / "with")) == sorted(os.listdir(tmp_path / "plain")) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
    with pytest.raises(TypeError, match="solver"):              # ... and with one it does reach it
        _generate(_Stub(), tmp_path / "c", solver=spec)
    with pytest.raises(TypeError, match="solver.Solver"):
        PL.generate_samples(_NoDevice(), {}, num_samples=2, solver="ddim")


def test_sample_sharded_passes_the_keyword_only_when_given():
    from protein_redesign_amd.distributed import sample_sharded
    from protein_redesign_amd.synthetic import synthetic_batch
    batch = synthetic_batch([(NA, NR)], esm_dim=16, seed=8)
    seen = []

    def sampler(bt, sources, **kw):
        seen.append(kw)
        n = bt["atom_mask"].shape[1]
        return torch.zeros(len(sources), n, 3), torch.zeros(len(sources), n, 21)
    spec = Solver.ancestral(3)
    sample_sharded(sampler, batch, 2)
    sample_sharded(sampler, batch, 2, solver=spec)
    sample_sharded(sampler, batch, 1, scaffold=Scaffold(), solver=spec)
    assert seen[:2] == [{}, {}] and seen[2:4] == [{"solver": spec}] * 2 and seen[2]["solver"] is spec
    assert sorted(seen[4]) == ["scaffold", "solver"]


# ---- the oracle's own fp32 run of the GPU test's loops --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.cases()))
def test_oracle_fp32_loop_stays_within_a_third_of_the_trajectory_bound(name):
    """What the GPU test compares the device loop with is the float64 loop; the bound it asserts (1e-4, the project's trajectory
    bound) only means something if fp32 arithmetic itself stays well inside it on this loop and seed."""
    args, params, batch = R.smoke_setup()
    lv, kind, eta, variance = R.cases()[name]
    assert R.package_solver(name).levels(16) == lv
    want = R.reference(name)
    got = R.oracle_loop(params, args, batch, NoiseSource(R.LOOP_SEED, 0), lv, kind, eta, variance, dtype=torch.float32)
    errs = [rel_l2(g, w) for g, w in zip(got, want)]
    print(f"\n{name}: oracle fp32 vs fp64: positions {errs[0]:.2e}, logits {errs[1]:.2e}, x0 {errs[2]:.2e}")
    assert all(e <= 1e-4 / 3 for e in errs), errs
    co = torch.tensor(R.coefficients(lv, R.abar(16), kind, eta, variance))
    if not bool((co[:, 2] != 0).any()):                         # deterministic: the last update IS the estimate
        assert rel_l2(got[0], 10.0 * got[2]) <= 1e-6
