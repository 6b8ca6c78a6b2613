"""CPU: multistep few-step sampling as far as it goes without a GPU -- the log-SNR levels, the new fields of ``Solver`` and their
refusals, the gain table against a quadrature restatement (tests/multistep_ref.py), polynomial exactness and the order of convergence
on a problem with a known solution, the header / build of libprd_multistep.so and its host refusals, and the oracle's own fp32 run of
every loop the GPU test uses against its float64 run."""
import ctypes
import math
import os

import pytest
import torch

import multistep_ref as M
import solver_ref as R
from conftest import ROOT, rel_l2
from protein_redesign_amd import _lib, build, diffusion_model, solver
from protein_redesign_amd.solver import Solver
from protein_redesign_amd.synthetic import NoiseSource
from sample_stubs import header_entries
from test_solver_cpu import _drawn

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
SOURCE = os.path.join(ROOT, "protein_redesign_amd", "csrc", "prd_multistep.hip")


# ---- levels ---------------------------------------------------------------------------------------------------------------------------

def test_the_level_lists_of_the_issue():
    assert Solver.multistep(6).levels(16, schedule="linear") == [0, 1, 2, 3, 7, 15] == M.levels(6, 15, 16)
    assert Solver.multistep(5).levels(16, schedule="linear") == [0, 1, 2, 6, 15] == M.levels(5, 15, 16)
    lv = Solver.multistep(21).levels(1000, schedule="linear")
    assert lv[:3] == [0, 1, 4] and lv[-3:] == [898, 950, 999] and lv == M.levels(21, 999, 1000)
    assert Solver.multistep(1).levels(16, schedule="linear") == [15]


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("T", [16, 64, 1000])
def test_logsnr_levels_are_strictly_increasing_between_their_end_points(T, schedule):
    lm = solver.log_snr64(T, schedule)
    assert bool((lm[1:] < lm[:-1]).all()) and float((lm - torch.tensor(M.lam(T, schedule), dtype=torch.float64)).abs().max()) <= 1e-12
    for top in sorted({T - 1, T // 2, 9}):                      # T - 1, and the start of a scaffold
        for K in sorted(K for K in {2, 3, 5, 6, 10, top // 2, top, top + 1} if K <= top + 1):
            lv = Solver.multistep(K).levels(T, top if top != T - 1 else None, schedule)
            assert len(lv) == K and lv[0] == 0 and lv[-1] == top and all(a < b for a, b in zip(lv, lv[1:])), (T, schedule, top, K)
            assert lv == M.levels(K, top, T, schedule), (T, schedule, top, K)
            assert lv == solver.logsnr_levels(K, top, T, schedule) == Solver(steps=K, kind="ddim", spacing="logsnr").levels(T, top, schedule)
        assert Solver.multistep(top + 1).levels(T, top, schedule) == list(range(top + 1))       # every level
        with pytest.raises(ValueError, match="do not fit"):
            Solver.multistep(top + 2).levels(T, top, schedule)


def test_uniform_spacing_is_what_it_was_and_logsnr_needs_the_schedule():
    assert Solver.ddim(4).levels(16) == solver.spaced_levels(4, 15) == [0, 5, 10, 15]
    assert Solver.ancestral(50).levels(1000) == solver.spaced_levels(50, 999) == Solver.ancestral(50).levels(1000, schedule="linear")
    assert Solver.multistep(4, spacing="uniform").levels(16) == [0, 5, 10, 15] == Solver.multistep(4, spacing="uniform").levels(16, schedule="linear")
    assert (Solver.ddim(4).spacing, Solver.ddim(4).spacing_rule, Solver.multistep(4).spacing_rule) == (None, "uniform", "logsnr")
    assert Solver.multistep(4, spacing=None).spacing_rule == "logsnr"
    assert Solver(steps=6, kind="ancestral", spacing="logsnr").levels(16, schedule="linear") == [0, 1, 2, 3, 7, 15]
    with pytest.raises(ValueError, match="schedule"):
        Solver.multistep(4).levels(16)
    with pytest.raises(ValueError, match="schedule"):
        Solver(steps=4, kind="ddim", spacing="logsnr").levels(16)
    assert Solver(timesteps=[15, 11, 6, 2, 0], kind="multistep", order=3).levels(16) == [0, 2, 6, 11, 15]


# ---- the spec -------------------------------------------------------------------------------------------------------------------------

def test_spec_is_validated_and_immutable():
    s = Solver.multistep(10)
    assert (s.kind, s.steps, s.order, s.form, s.spacing, s.eta, s.variance, s.K) == ("multistep", 10, 2, "exact", "logsnr", 0.0, "beta", 10)
    assert not s.stochastic and s.corrected and not Solver.multistep(10, order=1).corrected and not Solver.ddim(10).corrected
    d = Solver.dpmpp_2m(7)
    assert (d.kind, d.order, d.form, d.spacing, d.stochastic, d.corrected) == ("multistep", 2, "midpoint", "logsnr", False, True)
    e = Solver(timesteps=[15, 9, 2], kind="multistep", order=3)
    assert (e.order, e.form, e.spacing, e.K, e.stochastic) == (3, "exact", None, 3, False)
    assert [f.name for f in s.__dataclass_fields__.values()] == ["timesteps", "kind", "eta", "variance", "steps", "order", "form", "spacing"]
    assert (Solver.ddim(5).order, Solver.ddim(5).form, Solver.ancestral(5).spacing) == (1, "exact", None)
    for field in ("order", "form", "spacing", "kind"):
        with pytest.raises(Exception):                          # frozen
            setattr(s, field, getattr(d, field))
    ms, dd = dict(timesteps=[3, 1], kind="multistep"), dict(timesteps=[3, 1], kind="ddim")
    for kw, what in ((dict(ms, order=0), "order"), (dict(ms, order=4), "order"), (dict(ms, order=True), "order"), (dict(ms, order=2.5), "order"),
                     (dict(ms, form="trapezoid"), "form"), (dict(ms, order=3, form="midpoint"), "form='midpoint'"),
                     (dict(ms, order=1, form="midpoint"), "form='midpoint'"), (dict(dd, order=2), "order belongs"),
                     (dict(dd, form="midpoint"), "form belongs"), (dict(timesteps=[3, 1], form="midpoint"), "form belongs"),
                     (dict(timesteps=[3, 1], order=3), "order belongs"), (dict(dd, order=2, form="midpoint"), "order belongs"),
                     (dict(ms, eta=0.5), "eta"), (dict(ms, variance="posterior"), "variance"),
                     (dict(steps=4, kind="multistep", spacing="cosine"), "spacing"), (dict(steps=4, kind="ddim", spacing="log"), "spacing"),
                     (dict(ms, spacing="logsnr"), "spacing"), (dict(dd, spacing="uniform"), "spacing"), (dict(timesteps=[3, 1], kind="heun"), "kind")):
        with pytest.raises(ValueError, match=what):
            Solver(**kw)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="steps"):
            Solver.multistep(bad)
    assert "multistep" in repr(s) and "order=2" in repr(s) and "logsnr" in repr(s) and "midpoint" in repr(d) and "order=3" in repr(e)
    assert repr(Solver.ddim(50)) == "Solver(ddim, steps=50, eta=0.0)" and "posterior" in repr(Solver.ancestral(5, variance="posterior"))


def test_no_update_noise_is_drawn():
    T, N = 16, 6
    head = [(N, 3), (N, 21)]
    for spec in (Solver.multistep(5), Solver.multistep(5, order=3), Solver.dpmpp_2m(5), Solver.multistep(5, order=1)):
        shapes, _, _, noise = _drawn(spec, T)
        assert shapes == head and noise is None
        assert diffusion_model.update_noise_rows(spec, T) == 0 and diffusion_model.conditioning_noise_rows(spec, T, None) == 5
    from protein_redesign_amd.conditioning import Scaffold
    assert _drawn(Solver.multistep(5), T, Scaffold())[0] == head + [(N, 3)] * 5


def test_the_model_validates_the_levels_with_its_schedule():
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.conditioning import Scaffold
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    model = ProteinReDiffModel(make_args(single_dim=128, pair_dim=64, num_blocks=1, esm_dim=64, num_steps=8))
    s = Solver.multistep(4, order=3)
    assert model._solver_spec(s) is s and model._solver_spec(s, Scaffold(None, start=5)) is s
    with pytest.raises(ValueError, match="do not fit"):
        model.sample({}, sources=[], solver=Solver.multistep(9))
    with pytest.raises(ValueError, match="do not fit"):
        model._solver_spec(Solver.dpmpp_2m(5), Scaffold(None, start=3))


# ---- coefficients ---------------------------------------------------------------------------------------------------------------------

UNEVEN = {16: [15, 14, 9, 8, 3, 1, 0], 1000: [999, 998, 700, 650, 649, 300, 40, 39, 5, 0]}


def _specs(T):
    out = [(f"K{K}", K, None) for K in (3, 6, 21, 81) if K <= T]
    return out + [("uneven", len(UNEVEN[T]), UNEVEN[T])]


def _make(K, ts, order, form="exact"):
    if ts is not None:
        return Solver(timesteps=ts, kind="multistep", order=order, form=form)
    return Solver.dpmpp_2m(K) if form == "midpoint" else Solver.multistep(K, order=order)


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("T", [16, 1000])
def test_rows_are_those_of_ddim_on_the_same_levels_bit_for_bit(T, schedule):
    for _, K, ts in _specs(T):
        for order, form in ((1, "exact"), (2, "exact"), (2, "midpoint"), (3, "exact")):
            s = _make(K, ts, order, form)
            lv = s.levels(T, schedule=schedule)
            d = Solver(timesteps=lv[::-1], kind="ddim")
            assert torch.equal(s.coefficients64(T, schedule), d.coefficients64(T, schedule))
            (la, ta), (lb, tb) = s.tables(T, schedule), d.tables(T, schedule)
            assert torch.equal(la, lb) and torch.equal(ta, tb) and ta.dtype == torch.float32 and ta.shape == (K, 8)


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("T", [16, 1000])
def test_gains_against_the_quadrature_restatement_and_the_zero_pattern(T, schedule):
    worst = 0.0
    for name, K, ts in _specs(T):
        for order, form in ((1, "exact"), (2, "exact"), (2, "midpoint"), (3, "exact")):
            s = _make(K, ts, order, form)
            lv = s.levels(T, schedule=schedule)
            got = s.gains64(T, schedule)
            want = torch.tensor(M.gains(lv, T, schedule, order, form), dtype=torch.float64)
            assert got.shape == (K, 3) and got.dtype == torch.float64
            assert torch.equal(got == 0, want == 0), (T, schedule, name, order, form)
            nz = want != 0
            if bool(nz.any()):
                err = float(((got - want).abs()[nz] / want.abs()[nz]).max())
                worst = max(worst, err)
                assert err <= 1e-10, (T, schedule, name, order, form, err)
            # the zero pattern: row 0 (the last step is first order), and every entry whose history cannot exist
            assert float(got[0].abs().max()) == 0.0 and float(got[K - 1].abs().max()) == 0.0 and float(got[max(K - 2, 0):, 1:].abs().max()) == 0.0
            if order == 1:
                assert float(got.abs().max()) == 0.0
            else:
                assert bool((got[1:K - 1, 0] > 0).all())
            if order == 2 and K > 3:
                assert torch.equal(got[1:K - 2, 1], got[1:K - 2, 0]) and float(got[:, 2].abs().max()) == 0.0
            if order == 3 and K > 3:
                assert bool((got[1:K - 2, 1] > 0).all()) and bool((got[1:K - 2, 2] < 0).all())
            # the device table: rounded once, a zero column, 16-byte rows
            tab = s.gain_table(T, schedule)
            assert tab.shape == (K, 4) and tab.dtype == torch.float32 and torch.equal(tab[:, :3], got.float()) and float(tab[:, 3].abs().max()) == 0.0
    print(f"\nT={T} {schedule}: gains64 against 32-node Gauss-Legendre quadrature, worst relative deviation {worst:.2e}")


def test_the_series_takes_over_where_the_closed_forms_cancel():
    """every level of T = 1000 has steps of h ~ 0.01, where h^2 - 2 h - 2 expm1(-h) has lost six digits: the table still holds 1e-10"""
    assert solver.SERIES_BELOW == 0.05
    h = torch.tensor([1e-4, 1e-3, 1e-2, 0.049, 0.0501, 0.3, 2.0, 9.0], dtype=torch.float64)
    i1, i2 = solver._step_integrals(h)
    for j, hh in enumerate(h.tolist()):
        assert abs(float(i1[j]) - M.moment(hh, 1)) <= 1e-12 * M.moment(hh, 1) and abs(float(i2[j]) - M.moment(hh, 2)) <= 1e-12 * M.moment(hh, 2), hh
    s = Solver.multistep(1000, order=3)
    got, want = s.gains64(1000, "linear"), torch.tensor(M.gains(list(range(1000)), 1000, "linear", 3), dtype=torch.float64)
    nz = want != 0
    assert float(((got - want).abs()[nz] / want.abs()[nz]).max()) <= 1e-10


# ---- polynomial exactness ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order,poly,begin", [(3, (0.3, -0.2, 0.05), 2), (2, (0.3, -0.2, 0.0), 1)])
@pytest.mark.parametrize("T,K", [(1000, 21), (1000, 81), (16, 6)])
def test_the_update_integrates_the_polynomial_through_its_history_exactly(T, K, order, poly, begin):
    """float64 through the package's tables, fed the estimates x0(lam) = c0 + c1 lam + c2 lam^2: from step ``begin`` on (the history is
    then full) z_s = (sigma_s / sigma_t) z + sigma_s int e^lam x0(lam) dlam to 1e-10 at every step but the last, which is first order"""
    s = Solver.multistep(K, order=order)
    lv = s.levels(T, schedule="linear")
    co, gn, lm, ab = s.coefficients64(T, "linear"), s.gains64(T, "linear"), M.lam(T), R.abar(T)
    x0_of = lambda l: poly[0] + poly[1] * l + poly[2] * l * l          # noqa: E731
    z, hist, worst = 0.4, [], 0.0
    for step, k in enumerate(range(K - 1, 0, -1)):
        w, a, _, r, q = co[k].tolist()
        t, u = lv[k], lv[k - 1]
        x0 = x0_of(lm[t])
        eps = (z - x0 / q) / r                                   # the noise prediction whose estimate is x0
        want = math.sqrt((1 - ab[u]) / (1 - ab[t])) * z + M.flow_integral(poly, lm[t], lm[u], math.sqrt(1 - ab[u]))
        new = a * (z - w * eps)
        g = gn[k].tolist()
        if len(hist) == 1:
            new = new + g[0] * (x0 - hist[0])
        elif len(hist) == 2:
            new = new + g[1] * (x0 - hist[0]) + g[2] * (x0 - hist[1])
        if step >= begin:
            worst = max(worst, abs(new - want))
            assert abs(new - want) <= 1e-10, (T, K, order, step, new, want)
        elif order == 3 and step == 0:
            assert abs(new - want) > 1e-6                           # ... and not before: the first step is first order
        hist = [x0] + hist[:1]
        z = new
    print(f"\nT={T} K={K} order {order}: worst deviation from the exact integral {worst:.1e}")


# ---- order of convergence ---------------------------------------------------------------------------------------------------------------

def _toy_error(spec, T=1000):
    lv = spec.levels(T, schedule="linear")
    return M.toy_error(lv, R.abar(T), spec.coefficients64(T, "linear"), spec.gains64(T, "linear"))


def test_order_of_convergence_on_the_gaussian_toy_problem():
    """T = 1000, linear schedule, log-SNR spacing, data N(mu, s^2), the true noise, the exact probability flow: the error at level
    tau_0 falls by about 2, 4, 8 and 4 when K goes from 41 to 81 (orders 1, 2, 3 and DPM-Solver++ 2M); a margin is left below each"""
    assert (M.MU, M.S, M.START) == ((0.7, -0.3, 1.1), 0.5, (1.3, 0.2, -2.0))
    made = {"order 1": lambda K: Solver.multistep(K, order=1), "order 2": lambda K: Solver.multistep(K, order=2),
            "order 3": lambda K: Solver.multistep(K, order=3), "dpmpp_2m": Solver.dpmpp_2m}
    err = {name: {K: _toy_error(f(K)) for K in (21, 41, 81)} for name, f in made.items()}
    for name, e in err.items():
        print(f"\n{name}: error at tau_0 for K = 21, 41, 81: {e[21]:.3e} {e[41]:.3e} {e[81]:.3e}; ratio 41/81 {e[41] / e[81]:.2f}")
    for name, least in (("order 1", 1.8), ("order 2", 3.5), ("order 3", 7.0), ("dpmpp_2m", 3.5)):
        assert err[name][41] / err[name][81] >= least, (name, err[name])
    assert err["order 3"][81] < err["order 2"][81] < err["order 1"][81]
    # order 1 is ddim on the same levels, and under the uniform spacing a higher order does not help (why the spacing is part of this)
    assert _toy_error(Solver(steps=81, kind="ddim", spacing="logsnr")) == err["order 1"][81]
    uniform = [_toy_error(Solver.multistep(81, order=o, spacing="uniform")) for o in (1, 2, 3)]
    print(f"\nuniform spacing, K = 81, orders 1, 2, 3: " + " ".join(f"{e:.2e}" for e in uniform))
    assert min(uniform[1:]) > 0.5 * uniform[0]


# ---- header, build, host refusals -------------------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    e = header_entries("multistep")
    assert sorted(e) == ["prd_multistep_correct", "prd_multistep_version"]
    assert all(x.inject is None and x.restype is _lib.ci for x in e.values())
    assert e["prd_multistep_correct"].argtypes == [_lib.vp] * 6 + [_lib.ci] * 3 + [_lib.vp] and e["prd_multistep_version"].argtypes == []
    assert solver.MULTISTEP_ENTRIES == e and not set(e) & set(_lib.ENTRIES) and not set(e) & set(solver.ENTRIES)
    S = solver._DEFINES
    assert solver._MULTISTEP_DEFINES == {"VERSION": 100, "ERR_ARG": -1, "ERR_ALIGN": -2, "ERR_UNSUPPORTED": -3, "MAX_B": S["MAX_B"],
                                         "MAX_N": S["MAX_N"], "MAX_K": S["MAX_K"], "GAIN_STRIDE": 4}
    assert solver.MULTISTEP_ABI_VERSION == 100 and solver.GAIN_STRIDE == 4
    with open(SOURCE) as f:
        text = f.read()
    assert '#include "prd_launch.h"' in text and "hipLaunchKernelGGL" not in text and "<<<" not in text and "asm" not in text
    assert "atomic" not in text and "getenv" not in text and "hipMalloc" not in text and "Synchronize" not in text
    assert text.count("prd_launch<") == 1


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_one_kernel():
    mine = build.resource_usage(sources=build.SIDE_LIBS["multistep"].sources)
    assert sorted(mine) == ["multistep_correct_kernel"]
    u = mine["multistep_correct_kernel"]
    assert u["scratch"] == 0 and u["agprs"] == 0 and u["lds"] == 0 and u["vgprs"] <= 32


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_library_refuses_on_the_host_before_any_device_call():
    """every refusal of prd_multistep.h is host code that runs before the first HIP call: reachable without a GPU, with pointers that
    are never followed"""
    build.build_side("multistep", verbose=False)
    L, D = solver.multistep_lib(), solver._MULTISTEP_DEFINES
    assert L.prd_multistep_version() == 100
    p = ctypes.c_void_p(4096)
    names = ["z", "x0", "hist", "k", "first", "gain"]

    def call(b=2, N=5, K=4, **ptrs):
        return L.prd_multistep_correct(*[ptrs.get(n, p) for n in names], b, N, K, None)
    for n in names:
        assert call(**{n: None}) == D["ERR_ARG"], n
    for kw in (dict(b=0), dict(N=0), dict(K=0), dict(b=-1), dict(N=-3), dict(K=-1)):
        assert call(**kw) == D["ERR_ARG"], kw
    for kw in (dict(b=D["MAX_B"] + 1), dict(N=D["MAX_N"] + 1), dict(K=D["MAX_K"] + 1)):
        assert call(**kw) == D["ERR_UNSUPPORTED"], kw
    for off in (4, 8, 12):
        assert call(gain=ctypes.c_void_p(4096 + off)) == D["ERR_ALIGN"], off
    assert call(gain=ctypes.c_void_p(4096 + 4), b=0) == D["ERR_ARG"] and call(gain=ctypes.c_void_p(4096 + 4), N=D["MAX_N"] + 1) == D["ERR_UNSUPPORTED"]
    # the launch geometry the bounds promise: 3 N and the grid fit an int, the grid's second dimension stays below 65536
    assert 3 * D["MAX_N"] < 2 ** 31 and D["MAX_B"] < 65536 and 2 * D["MAX_B"] * 3 * D["MAX_N"] < 2 ** 63


def test_the_restatement_in_float32_keeps_the_order_of_the_launch():
    """restate_correct on the host: the three cases of n, the untouched samples, and nothing in place"""
    g = torch.Generator().manual_seed(2)
    K, b, N = 5, 6, 3
    z, x0, hist = torch.randn(b, N, 3, generator=g), torch.randn(b, N, 3, generator=g), torch.randn(2, b, N, 3, generator=g)
    gain = torch.randn(K, 4, generator=g)
    k, first = torch.tensor([3, 2, 1, -1, 4, 2]), torch.tensor([4, 4, 4, 4, 4, 2])       # cur = 4, 3, 2, 0, 5, 3 (> first)
    keep = [x.clone() for x in (z, x0, hist)]
    out = solver.restate_correct(z, x0, hist, k, first, gain, dtype=torch.float32)
    assert all(torch.equal(a, c) for a, c in zip(keep, (z, x0, hist))) and out["live"].tolist() == [True, True, True, False, False, False]
    assert torch.equal(out["z"][0], z[0]) and torch.equal(out["z"][1], z[1] + gain[3, 0] * (x0[1] - hist[0, 1]))
    assert torch.equal(out["z"][2], z[2] + (gain[2, 1] * (x0[2] - hist[0, 2]) + gain[2, 2] * (x0[2] - hist[1, 2])))
    for s in (0, 1, 2):
        assert torch.equal(out["hist"][0, s], x0[s]) and torch.equal(out["hist"][1, s], hist[0, s])
    for s in (3, 4, 5):
        assert torch.equal(out["z"][s], z[s]) and torch.equal(out["hist"][:, s], hist[:, s])
    assert solver.restate_correct(z, x0, hist, k, first, gain)["z"].dtype == torch.float64


# ---- the oracle's own fp32 run of the GPU test's loops ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(M.cases()))
def test_oracle_fp32_loop_stays_within_a_third_of_the_trajectory_bound(name):
    """What the GPU test compares the device loop with is the float64 loop; the bound it asserts (1e-4, the project's trajectory
    bound) only means something if fp32 arithmetic itself stays well inside it on this loop and seed."""
    args, params, batch = R.smoke_setup()
    lv, order, form = M.cases()[name]
    spec = M.package_solver(name)
    assert spec.levels(16, schedule="linear") == lv and (spec.order, spec.form) == (order, form)
    want = M.reference(name)
    got = M.oracle_loop(params, args, batch, NoiseSource(R.LOOP_SEED, 0), lv, order, form, dtype=torch.float32)
    errs = [rel_l2(g, w) for g, w in zip(got, want)]
    print(f"\n{name}: oracle fp32 vs fp64: positions {errs[0]:.2e}, logits {errs[1]:.2e}, x0 {errs[2]:.2e}")
    assert all(e <= 1e-4 / 3 for e in errs), errs
    assert rel_l2(got[0], 10.0 * got[2]) <= 1e-6                   # the last step is first order: the last update IS the estimate
