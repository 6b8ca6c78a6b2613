"""GPU: few-step sampling (solver.Solver, libprd_solver.so, ReverseDiffusion(solver=...)).

1. prd_solver_boundary against the float64 restatement (solver.restate_boundary), every tensor in a guarded, poisoned buffer of its own
   (tests/guarded_alloc.py): b in {1, 3} x N in {1, 7, 8, 9, 40, 257} -- the 8-node workgroup edge and the 256-thread reduction edge --,
   S in {96, 512}, P in {32, 64}, time_dim in {2, 64, 512}, the sequence head's hidden units given (contiguous and as a column block)
   and absent, the noise table and the estimate's buffer given and absent, counters at K - 1, in the middle, at 0, differing within a
   batch, and outside [0, K): such a sample is bit-untouched.  Relative L2 <= 1e-5, the project's operator bound; counters exact.
2. Equal tables, equal bits: against prd_step_boundary on the same inputs, and the whole loop under Solver.ancestral(T) against the
   loop without a solver, in both arithmetics.
3. Strided loops against the float64 loop over the oracle's network (tests/solver_ref.py), relative L2 <= 1e-4, the project's
   trajectory bound, both arithmetics; graph replay against eager stepping; with a scaffold; with sequence rules; no host
   synchronisation; pipeline.generate_samples end to end.

The model is the smoke configuration: single_dim 128, pair_dim 64, 2 blocks, num_steps 16, 8 atoms + 40 residues in 48 positions."""
import os
import warnings

import numpy as np
import pytest
import torch

import solver_ref as R
from conftest import rel_l2
from guarded_alloc import Guard
from no_host_sync import run_without_host_sync
from protein_redesign_amd import _lib, conditioning, ops
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd import sequence as SQ
from protein_redesign_amd.conditioning import Scaffold
from protein_redesign_amd.diffusion_model import ProteinReDiffModel, ReverseDiffusion
from protein_redesign_amd.masking import Redesign
from protein_redesign_amd.sequence import SequenceRules
from protein_redesign_amd.solver import Solver, restate_boundary, solver_boundary_
from protein_redesign_amd.synthetic import NoiseSource, batch_to, clone_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
OP_TOL, STEP_TOL, TRAJ_TOL = 1e-5, 4e-5, 1e-4
T, NA, NR, NP = 16, 8, 40, 48


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
# (S, P, time_dim, seq_h: None / "rows" / "block", noise given, x0_out given); every value of every axis occurs
CONFIGS = [(96, 32, 2, "rows", True, True), (512, 64, 512, None, True, False), (96, 64, 64, "block", False, True),
           (512, 32, 64, None, False, False), (96, 32, 512, "rows", True, True)]
SPEC = Solver.ddim(5, eta=0.5)          # K = 5 over T = 16: levels 0, 4, 8, 11, 15; every c but the first is non-zero
K = 5


def counter_sets(b):
    if b == 1:
        return [[K - 1], [2], [0], [-1], [K]]
    return [[K - 1, 2, 0], [0, K, 3], [-1, K - 1, K + 7], [1, 1, -4]]


def boundary_case(b, N, S, P, TD, g):
    r = lambda *shape: torch.randn(*shape, generator=g)       # noqa: E731
    mask = (torch.rand(b, N, generator=g) < 0.8).float()
    mask[:, 0] = 1.0                                            # at least one valid node per sample
    rm = mask * (torch.rand(b, N, generator=g) < 0.7).float()
    return dict(z=r(b, N, 3), eps_raw=r(b, N, 3), seq_pred=2.0 * r(b, N, 21), noise=r(K - 1, b, N, 3), mask=mask, static_single=r(b, N, S),
                residue_mask=rm, w_rt=r(S, 21) / 4, freqs=torch.logspace(-4.0, 0.0, TD // 2), w_beta=r(P, TD) / TD ** 0.5,
                seq_h=torch.relu(r(b, N, S)), w_seq=r(21, S) / S ** 0.5,
                seq_t0=r(b, N, 21), single0=r(b, N, S), ebeta0=r(b, P), x00=r(b, N, 3))


def launch(guard, c, ks, levels, coef, how_h, with_noise, with_x0):
    """one launch on guarded copies; returns the device tensors by name"""
    put = lambda x: guard.put(x, DEV)                           # noqa: E731
    d = {n: put(c[n]) for n in ("z", "eps_raw", "seq_pred", "mask", "static_single", "residue_mask", "w_rt", "freqs", "w_beta")}
    d["seq_t"], d["single_next"], d["ebeta_next"] = put(c["seq_t0"]), put(c["single0"]), put(c["ebeta0"])
    d["k"], d["t"] = put(torch.tensor(ks, dtype=torch.int64)), put(torch.full((len(ks),), 77, dtype=torch.int64))
    d["levels"], d["coef"], d["sync"] = put(levels), put(coef), put(torch.zeros(2, dtype=torch.int32))
    d["noise"] = put(c["noise"]) if with_noise else None
    d["x0"] = put(c["x00"]) if with_x0 else None
    h = w = None
    if how_h == "rows":
        h, w = put(c["seq_h"]), put(c["w_seq"])
    elif how_h == "block":                                      # the hidden units as a column block of a wider tensor
        S = c["seq_h"].shape[-1]
        big = put(torch.cat([c["seq_h"], torch.full_like(c["seq_h"][..., :8], float("nan"))], dim=-1))
        h, w = big[..., :S], put(c["w_seq"])
        assert h.stride(1) == S + 8
    solver_boundary_(d["z"], d["seq_t"], d["k"], d["t"], d["eps_raw"], d["seq_pred"], d["noise"], d["mask"], d["levels"], d["coef"], T,
                     d["single_next"], d["static_single"], d["residue_mask"], d["w_rt"], d["ebeta_next"], d["freqs"], d["w_beta"],
                     d["sync"], x0_out=d["x0"], seq_h=h, w_seq=w)
    return d


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("N", [1, 7, 8, 9, 40, 257])
def test_kernel_equals_the_float64_restatement(N, b):
    levels, coef = SPEC.tables(T, "linear")
    assert levels.tolist() == [0, 4, 8, 11, 15] and bool((coef[1:, 2] > 0).all())
    worst = {}
    for ci, (S, P, TD, how_h, with_noise, with_x0) in enumerate(CONFIGS):
        g = torch.Generator().manual_seed(10000 * b + 10 * N + ci)
        c = boundary_case(b, N, S, P, TD, g)
        for ks in counter_sets(b):
            guard = Guard("nan")
            d = launch(guard, c, ks, levels, coef, how_h, with_noise, with_x0)
            want = restate_boundary(c["z"], c["seq_pred"], torch.tensor(ks), c["eps_raw"], c["noise"] if with_noise else None, c["mask"],
                                    levels, coef, T, c["static_single"], c["residue_mask"], c["w_rt"], c["freqs"], c["w_beta"],
                                    seq_h=c["seq_h"] if how_h else None, w_seq=c["w_seq"] if how_h else None)
            where = (N, b, S, P, TD, how_h, with_noise, with_x0, ks)
            assert guard.intact(), (where, guard.report())
            got = {n: d[n].cpu() for n in ("z", "seq_t", "seq_pred", "single_next", "ebeta_next", "k", "t")}
            got["x0"] = d["x0"].cpu() if with_x0 else None
            before = dict(z=c["z"], seq_t=c["seq_t0"], seq_pred=c["seq_pred"], single_next=c["single0"], ebeta_next=c["ebeta0"], x0=c["x00"])
            assert d["sync"].cpu().tolist() == [0, 0], where        # the arrival counter is back at zero, nothing was non-finite
            for s, kk in enumerate(ks):
                if not 0 <= kk < K:             # bit-untouched: state, outputs, counters
                    for n, was in before.items():
                        assert got[n] is None or torch.equal(got[n][s], was[s]), where + (s, n)
                    assert int(got["k"][s]) == kk and int(got["t"][s]) == 77, where + (s,)
                    continue
                assert int(got["k"][s]) == kk - 1 and int(got["t"][s]) == (int(levels[kk - 1]) if kk > 0 else -1), where + (s,)
                names = ["z", "seq_t", "seq_pred", "single_next"] + (["ebeta_next"] if kk > 0 else []) + (["x0"] if with_x0 else [])
                for n in names:
                    err = rel_l2(got[n][s], want[n][s])
                    worst[n] = max(worst.get(n, 0.0), err)
                    assert err <= OP_TOL, where + (s, n, err)
                if kk == 0:
                    assert torch.equal(got["ebeta_next"][s], c["ebeta0"][s]), where + (s,)
                if not how_h:
                    assert torch.equal(got["seq_pred"][s], c["seq_pred"][s]), where + (s,)
            # what was only read came back as it went in
            for n in ("eps_raw", "mask", "static_single", "residue_mask", "w_rt", "freqs", "w_beta"):
                assert torch.equal(d[n].cpu(), c[n]), where + (n,)
            assert torch.equal(d["levels"].cpu(), levels) and torch.equal(d["coef"].cpu(), coef)
    print(f"\nN={N} b={b}: worst rel-L2 against float64 " + ", ".join(f"{n} {e:.1e}" for n, e in sorted(worst.items())))
    assert set(worst) == {"z", "seq_t", "seq_pred", "single_next", "ebeta_next", "x0"}


def test_two_launches_are_bit_identical():
    levels, coef = SPEC.tables(T, "linear")
    S, P, TD, b, N = 96, 32, 64, 3, 257
    c = boundary_case(b, N, S, P, TD, torch.Generator().manual_seed(11))
    outs = []
    for _ in range(2):
        guard = Guard("nan")
        d = launch(guard, c, [K - 1, 2, 0], levels, coef, "rows", True, True)
        outs.append([d[n].clone() for n in ("z", "seq_t", "seq_pred", "single_next", "ebeta_next", "x0", "k", "t")])
        assert guard.intact(), guard.report()
    assert all(torch.equal(a, b2) for a, b2 in zip(*outs))
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][3]).all())


def test_wrapper_refuses_tables_that_do_not_fit():
    levels, coef = SPEC.tables(T, "linear")
    c = boundary_case(1, 8, 96, 32, 64, torch.Generator().manual_seed(12))
    guard = Guard("nan")
    with pytest.raises(ValueError, match="coef must be"):
        launch(guard, c, [0], levels, coef[:, :4].contiguous(), None, True, True)
    with pytest.raises(ValueError, match="noise must be"):
        launch(guard, dict(c, noise=c["noise"][:2]), [0], levels, coef, None, True, True)
    with pytest.raises(ValueError, match="k and t"):
        launch(guard, c, [0, 1], levels, coef, None, True, True)


@pytest.mark.parametrize("how_h", [None, "rows"])
@pytest.mark.parametrize("N", [40, 257])
def test_equal_tables_give_the_bits_of_prd_step_boundary(N, how_h):
    """model._coef's rows, levels = range(T), k = t: the six outputs are those of prd_step_boundary on the same inputs, bit for bit --
    at t = 0 all but the time embedding, which prd_step_boundary computes for level -1 and this kernel leaves alone."""
    from protein_redesign_amd import schedule
    S, P, TD, b = 128, 64, 64, 3
    coef4 = schedule.reverse_coefficients(schedule.schedule_tables(T, "linear"))
    levels, coef8 = Solver.ancestral(T).tables(T, "linear", coef=coef4)
    assert torch.equal(coef8[:, :3], coef4[:, :3])
    g = torch.Generator().manual_seed(100 + N)
    c = boundary_case(b, N, S, P, TD, g)
    noise = torch.randn(T - 1, b, N, 3, generator=g)
    for ts in ([T - 1, 5, 1], [0, 9, 0], [0, 0, 0]):
        dev = lambda x: x.to(DEV).contiguous()                 # noqa: E731
        common = {n: dev(c[n]) for n in ("eps_raw", "mask", "static_single", "residue_mask", "w_rt", "freqs", "w_beta")}
        h, w = (dev(c["seq_h"]), dev(c["w_seq"])) if how_h else (None, None)
        outs = []
        for mine in (False, True):
            z, seq_t, seq_pred = dev(c["z"]), dev(c["seq_t0"]), dev(c["seq_pred"])
            single, eb = dev(c["single0"]), dev(c["ebeta0"])
            t = torch.tensor(ts, dtype=torch.int64, device=DEV)
            sync = torch.zeros(2, dtype=torch.int32, device=DEV)
            if mine:
                k = t.clone()
                solver_boundary_(z, seq_t, k, t, common["eps_raw"], seq_pred, dev(noise), common["mask"], dev(levels), dev(coef8), T, single,
                                 common["static_single"], common["residue_mask"], common["w_rt"], eb, common["freqs"], common["w_beta"], sync,
                                 seq_h=h, w_seq=w)
                assert torch.equal(k, t)
            else:
                ops.step_boundary_(z, seq_t, t, common["eps_raw"], seq_pred, dev(noise), common["mask"], dev(coef4), T, single,
                                   common["static_single"], common["residue_mask"], common["w_rt"], eb, common["freqs"], common["w_beta"], sync,
                                   seq_h=h, w_seq=w)
            outs.append(dict(z=z, seq_t=seq_t, seq_pred=seq_pred, single=single, eb=eb, t=t))
        old, new = outs
        for n in ("z", "seq_t", "seq_pred", "single", "t"):
            assert torch.equal(old[n], new[n]), (N, how_h, ts, n, float((old[n].double() - new[n].double()).abs().max()))
        later = torch.tensor(ts) > 0
        assert torch.equal(old["eb"][later], new["eb"][later]), (N, how_h, ts)
        assert torch.equal(new["eb"][~later].cpu(), c["ebeta0"][~later])


# ---------------------------------------------------------------------------------------------------
# 2. / 3. the loop
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup():
    args, params, batch = R.smoke_setup()
    model = ProteinReDiffModel(args)
    model.load_state_dict(params)
    model = model.to(DEV).eval()
    inv = torch.zeros(1, NP)
    inv[0, NA + 10: NA + 24] = 1                                 # an explicit design region: no permutation is drawn for it
    return dict(args=args, params=params, batch=batch, model=model, region=Redesign.positions(inv).to(DEV), inv=inv)


def loop_of(setup, solver=None, run=True, region=False, seed=R.LOOP_SEED, **kw):
    loop = ReverseDiffusion(setup["model"], batch_to(clone_batch(setup["batch"]), DEV), [NoiseSource(seed, 0)],
                            redesign=setup["region"] if region else None, **({"solver": solver} if solver is not None else {}), **kw)
    if run:
        loop.run()
    return loop


@pytest.mark.parametrize("arith", ["split16", "fp32"])
def test_full_length_ancestral_solver_is_the_loop_as_it_was(setup, arith):
    with _lib.arithmetic(arith):
        plain = loop_of(setup)
        mine = loop_of(setup, Solver.ancestral(T))
        assert mine.K == T and mine.steps_done == T and mine.k is not None and plain.k is None and plain.x0_hat is None
        assert mine.noise.shape == plain.noise.shape == (T - 1, 1, NP, 3) and torch.equal(mine.noise, plain.noise)
        assert torch.equal(mine.coef[:, :3], setup["model"]._coef[:, :3])
        for a, b in zip(plain.result() + (plain.z, plain.seq_t), mine.result() + (mine.z, mine.seq_t)):
            assert torch.equal(a, b), float((a.double() - b.double()).abs().max())
        assert int(mine.k[0]) == -1 and int(mine.t[0]) == -1 and int(plain.t[0]) == -1 and mine.finite()
        # through sample(): the same again, and without the keyword sample() is what it was
        model = setup["model"]
        keep, model.arithmetic = model.arithmetic, arith
        try:
            a = model.sample(batch_to(clone_batch(setup["batch"]), DEV), sources=[NoiseSource(R.LOOP_SEED, 0)])
            b = model.sample(batch_to(clone_batch(setup["batch"]), DEV), sources=[NoiseSource(R.LOOP_SEED, 0)], solver=Solver.ancestral(T))
        finally:
            model.arithmetic = keep
        assert all(torch.equal(x, y) for x, y in zip(a, plain.result())) and all(torch.equal(x, y) for x, y in zip(b, a))


@pytest.mark.parametrize("arith", ["split16", "fp32"])
@pytest.mark.parametrize("name", sorted(R.cases()))
def test_strided_loop_matches_the_float64_loop(setup, name, arith):
    """positions and logits against the float64 loop over the oracle's network (computed once per case, shared by both arithmetics;
    tests/test_solver_cpu.py holds the oracle's own fp32 run within a third of the bound).  The positions are ten times the last
    estimate -- for ddim with eta = 0 by construction, and for every other kind as well, since abar_s = 1 at the last counter makes
    a = q and w = r in the formulas and no noise is added there: up to one rounding of each coefficient the two agree to a few fp32
    ulps of the terms (8 ulps of the largest coordinate are asserted)."""
    want_pos, want_logits, want_x0 = R.reference(name)
    spec = R.package_solver(name)
    with _lib.arithmetic(arith):
        loop = loop_of(setup, spec)
        pos, logits = loop.result()
    assert loop.steps_done == spec.K == loop.K and loop.graph is not None and loop.finite()
    assert (loop.noise is None) == (not spec.stochastic) and (loop.noise is None or loop.noise.shape == (spec.K - 1, 1, NP, 3))
    e_pos, e_log, e_x0 = rel_l2(pos.cpu(), want_pos), rel_l2(logits.cpu(), want_logits), rel_l2(loop.x0_hat.cpu(), want_x0)
    print(f"\n{name} [{arith}] vs the float64 loop: positions {e_pos:.2e}, logits {e_log:.2e}, last estimate {e_x0:.2e}")
    assert e_pos <= TRAJ_TOL and e_log <= TRAJ_TOL and e_x0 <= TRAJ_TOL
    gap = float((pos - 10.0 * loop.x0_hat).abs().max())
    assert gap <= 8 * 2.0 ** -23 * float(pos.abs().max()), gap
    with pytest.raises(RuntimeError, match="already done"):
        loop.step()


@pytest.mark.parametrize("name", ["ddim4", "ancestral4_posterior"])
def test_graph_replay_equals_eager_stepping(setup, name):
    model, spec = setup["model"], R.package_solver(name)
    out = {}
    try:
        for graph in (False, True):
            model.use_hip_graph = graph
            loop = loop_of(setup, spec)
            assert (loop.graph is not None) == graph and loop.fused_boundary
            out[graph] = [x.clone() for x in (loop.z, loop.seq_t, loop.x0_hat, *loop.result())]
            if graph:                           # a second pass over the captured graph from the stored initial state
                loop.reset()
                assert int(loop.k[0]) == spec.K - 1 and int(loop.t[0]) == 15 and loop.steps_done == 0
                loop.run()
                assert all(torch.equal(a, b) for a, b in zip(out[True], (loop.z, loop.seq_t, loop.x0_hat, *loop.result())))
                # one replay too many is a no-op, not an out-of-range read: the counter is outside [0, K)
                loop.graph.replay()
                assert all(torch.equal(a, b) for a, b in zip(out[True], (loop.z, loop.seq_t, loop.x0_hat, *loop.result())))
                assert int(loop.k[0]) == -1
    finally:
        model.use_hip_graph = True
    assert all(torch.equal(a, b) for a, b in zip(out[False], out[True]))


def test_restart_continues_on_the_noise_the_loop_would_have_used(setup):
    """restart(0, ...) from the stored initial state is the run itself, bit for bit: both begin from _step_inputs, and the noise table is
    indexed by the counter.  restart(2, ...) from the state a run had after two steps rebuilds the coming step's inputs with
    prd_single_init / prd_time_embed where the uninterrupted run had them from the boundary kernel, so it is held to the trajectory
    bound, not to the bit -- a continuation on the wrong noise rows or levels would be off by the size of the noise itself."""
    spec = Solver.ancestral(4)
    whole = loop_of(setup, spec, run=False)
    init = (whole._init[0].clone(), whole._init[1].clone())
    whole.step()
    whole.step()
    z2, s2 = whole.z.clone(), whole.seq_t.clone()
    assert int(whole.k[0]) == 1 and int(whole.t[0]) == 5
    whole.run()
    again = loop_of(setup, spec, run=False)
    again.restart(2, z2, s2)
    assert int(again.k[0]) == 1 and int(again.t[0]) == 5 and again.steps_done == 2
    again.run()
    assert again.steps_done == 4 and int(again.k[0]) == -1
    e_z, e_log = rel_l2(again.z.cpu(), whole.z.cpu()), rel_l2(again.result()[1].cpu(), whole.result()[1].cpu())
    print(f"\nrestart(2) against the uninterrupted run: state {e_z:.2e}, logits {e_log:.2e}")
    assert e_z <= TRAJ_TOL and e_log <= TRAJ_TOL
    again.restart(0, *init)
    assert int(again.k[0]) == 3 and int(again.t[0]) == 15 and again.steps_done == 0
    again.run()
    assert torch.equal(again.z, whole.z) and torch.equal(again.result()[1], whole.result()[1])
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        again.restart(4, z2, s2)


def _conditioning_draws(setup, spec, loop, count):
    """the conditioning noise of the loop, drawn again from a copy of its source: after z_T, seq_T and the update tensors"""
    src = NoiseSource(R.LOOP_SEED, 0)
    for shape in [(NP, 3), (NP, 21)] + [(NP, 3)] * (spec.K - 1 if spec.stochastic else 0):
        src.randn(*shape)
    return [ops.remove_mean(src.randn(NP, 3)[None].to(DEV).contiguous(), loop.mask) for _ in range(count)]


def test_scaffold_rows_are_noised_to_the_level_that_comes_next(setup):
    """Scaffold('outside') under ddim(4), levels 15, 10, 5, 0: after every boundary the kept rows are A[tau] x0c + S[tau] eps_k for the
    level tau that comes NEXT, bit for bit against conditioning.restate_rows on the model's FULL tables and draws repeated here, and the
    input itself after the last one: back at the input's coordinates to 1e-5 Angstrom (coordinates below 32 Angstrom: one fp32 ulp is
    1.9e-6 Angstrom and four roundings lie between the input and the output)."""
    model, spec = setup["model"], Solver.ddim(4)
    model.use_hip_graph = False
    try:
        loop = loop_of(setup, spec, run=False, region=True, scaffold=Scaffold("outside"))
        lv = [0, 5, 10, 15]
        assert loop._levels == lv and loop.cond_noise.shape == (4, 1, NP, 3) and loop.level.shape == (4, 2) and loop.noise is None
        eps = dict(zip([15, 10, 5, 0], _conditioning_draws(setup, spec, loop, 4)))
        full = conditioning.level_table({k: getattr(model, k) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")})
        table = torch.zeros(T, 1, NP, 3, device=DEV)
        for tau, e in eps.items():
            table[tau] = e
        kept = loop.keep > 0.5
        assert 0 < int(kept.sum()) < NR and torch.equal(kept.cpu(), (setup["batch"]["residue_mask"] - setup["inv"]) > 0.5)

        def held(tau):
            z, _ = conditioning.restate_rows(torch.zeros_like(loop.z), None, torch.tensor([tau]), x0c=loop.x0c, keep_z=loop.keep, noise=table, level=full)
            return z[kept]
        assert torch.equal(loop.z[kept], held(15))              # the initial state: the top level
        for k in (3, 2, 1, 0):
            loop.step()
            nxt = lv[k - 1] if k > 0 else -1
            assert int(loop.k[0]) == k - 1 and int(loop.t[0]) == nxt
            assert torch.equal(loop.z[kept], held(nxt)), k
        assert loop.steps_done == 4 and torch.equal(loop.z[kept], loop.x0c[kept])
    finally:
        model.use_hip_graph = True
    b = setup["batch"]
    given = (b["atom_mask"].unsqueeze(-1) * b["atom_pos"] + b["residue_mask"].unsqueeze(-1) * b["residue_atom_pos"][:, :, 1]).to(DEV)
    assert float(given.abs().max()) < 32.0
    pos, _ = loop.result()
    err = float((pos[kept] - given[kept]).abs().max())
    print(f"\nkept rows against the input: {err:.2e} Angstrom")
    assert err <= 1e-5
    free = (loop.mask > 0.5) & ~kept
    assert bool((pos[free] - given[free]).abs().amax(dim=-1).gt(1e-2).all())


def test_partial_diffusion_spreads_the_levels_below_the_start(setup):
    """Scaffold(None, start=9) under ddim(4): levels 9, 6, 3, 0; every valid row starts at A[9] x0c + S[9] eps, eps the first of the four
    conditioning draws; nothing is held afterwards; the loop equals one restarted from that state."""
    model, spec = setup["model"], Solver.ddim(4)
    loop = loop_of(setup, spec, run=False, region=True, scaffold=Scaffold(None, start=9))
    assert loop._levels == [0, 3, 6, 9] and int(loop.t[0]) == 9 and int(loop.k[0]) == 3 and loop.cond is None and loop.steps_done == 0
    assert loop.cond_noise.shape == (4, 1, NP, 3)
    eps = _conditioning_draws(setup, spec, loop, 4)[0]
    full = conditioning.level_table({k: getattr(model, k) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")})
    table = torch.zeros(T, 1, NP, 3, device=DEV)
    table[9] = eps
    z9, _ = conditioning.restate_rows(torch.zeros_like(loop.z), None, torch.tensor([9]), x0c=loop.x0c, keep_z=loop.mask, noise=table, level=full)
    valid = loop.mask > 0.5
    assert torch.equal(loop._init[0][valid], z9[valid])
    steps = 0
    while loop.steps_done < loop.K:
        loop.step()
        steps += 1
    assert steps == 4 and int(loop.t[0]) == -1 and loop.finite()
    free = loop_of(setup, Solver(timesteps=[9, 6, 3, 0], kind="ddim"), run=False, region=True)
    free.restart(0, loop._init[0], loop._init[1])
    free.run()
    assert torch.equal(free.z, loop.z) and torch.equal(free.result()[1], loop.result()[1])
    with pytest.raises(ValueError, match="do not fit"):
        loop_of(setup, Solver.ddim(11), run=False, region=True, scaffold=Scaffold(None, start=9))


def test_sequence_rules_hold_under_a_solver(setup):
    """a banned class is exactly -1 in seq_t after every step and exactly BANNED (-32768) in the returned logits"""
    model, cls = setup["model"], 5
    rules = SequenceRules.for_residues(NA, NR, omit=SQ.ALPHABET[cls], unknown=True)
    assert SQ.BANNED == -32768.0
    model.use_hip_graph = False
    try:
        loop = loop_of(setup, Solver.ancestral(4), run=False, region=True, sequence_rules=rules.to(DEV))
        rows = loop.rules[1] > 0.5
        assert torch.equal(rows.cpu(), setup["inv"] > 0.5)
        steps = 0
        while loop.steps_done < loop.K:
            loop.step()
            steps += 1
            now = loop.seq_t[rows]
            assert bool((now[:, cls] == -1.0).all()) and bool((now.max(dim=-1).values > -1.0).all()), steps
        assert steps == 4
    finally:
        model.use_hip_graph = True
    _, logits = loop.result()
    assert bool((logits[rows][:, cls] == SQ.BANNED).all()) and bool(torch.isfinite(logits).all())
    # and through the captured graph the same bits
    again = loop_of(setup, Solver.ancestral(4), region=True, sequence_rules=rules.to(DEV))
    assert again.graph is not None and torch.equal(again.result()[1], logits) and torch.equal(again.seq_t, loop.seq_t)


def test_a_solver_loop_with_a_scaffold_is_set_up_and_run_without_host_synchronisation(setup):
    model = setup["model"]
    spec, scaffold = Solver.ancestral(4, variance="posterior"), Scaffold("outside", ligand=True, sequence=True).to(DEV)
    warm = loop_of(setup, spec, region=True, scaffold=scaffold)         # warm: library, allocators, the constant tables of the model
    d = batch_to(clone_batch(setup["batch"]), DEV)
    sources = [NoiseSource(R.LOOP_SEED, 0)]

    def work():
        loop = ReverseDiffusion(model, d, sources, redesign=setup["region"], scaffold=scaffold, solver=spec)
        loop.run()
        return loop
    loop = run_without_host_sync(work)
    assert loop.steps_done == 4 and loop.finite() and loop.graph is not None
    assert torch.equal(loop.z, warm.z) and torch.equal(loop.result()[1], warm.result()[1])


def test_generate_samples_end_to_end(setup, tmp_path):
    """the files it wrote without a solver, samples that differ from the full loop's, and the same samples on a second call"""
    from protein_redesign_amd.synthetic import synthetic_sample
    model = setup["model"]
    data = synthetic_sample(NA, NR, esm_dim=64, seed=0)

    def generate(out, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            return PL.generate_samples(model, data, num_samples=3, batch_size=2, seed=4, output_dir=out, **kw)
    few = generate(tmp_path / "few", solver=Solver.ddim(4))
    full = generate(tmp_path / "full")
    assert len(few) == len(full) == 4 and few[0].shape == full[0].shape == (3, NP, 3)
    assert sorted(os.listdir(tmp_path / "few")) == sorted(os.listdir(tmp_path / "full")) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
    assert np.isfinite(few[0]).all() and np.isfinite(few[1]).all() and not np.array_equal(few[0], full[0])
    assert np.abs(few[0][0] - few[0][1]).max() > 1e-2           # three samples, not one
    again = generate(tmp_path / "again", solver=Solver.ddim(4))
    assert np.array_equal(again[0], few[0]) and np.array_equal(again[1], few[1])
