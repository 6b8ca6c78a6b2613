"""GPU: structure-conditioned sampling (conditioning.Scaffold, libprd_condition.so, ReverseDiffusion(scaffold=...)).

1. prd_condition_rows against the torch restatement (conditioning.restate_rows, which tests/test_conditioning_cpu.py holds against
   float64), bit for bit: rows of 1 .. 257 positions (63 / 64 / 65: a wave, 257: more than one workgroup of z elements and of sequence
   elements), 1 and 3 samples whose counters mix -1, 0, levels - 1 and levels (the no-op), every keep pattern and NULL, tensors carved
   out of sentinel-filled buffers; bit-reproducibility; the refusals by code.
2. The loop: nothing kept changes nothing; kept rows come back at the input's coordinates; graph replay equals eager stepping with both
   boundaries and with the sequence clamp; partial diffusion equals a restarted unconditioned loop; the loop against one written here
   from the oracle's network; no host synchronisation.
3. pipeline.generate_samples end to end.

The model and fixture of section 2 are those of tests/test_redesign_region.py section 3 (5 atoms + 20 residues in 27 positions, T = 4)."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import prd_oracle as O
from conftest import rel_l2
from no_host_sync import run_without_host_sync
from protein_redesign_amd import conditioning, ops
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.conditioning import Scaffold, condition_rows_, restate_rows
from protein_redesign_amd.diffusion_model import ReverseDiffusion
from protein_redesign_amd.masking import Redesign
from protein_redesign_amd.synthetic import NoiseSource, batch_to, clone_batch
from test_hip_parity import TRAJ_TOL
from test_redesign_region import restated_spec_masks, sample_setup
from test_training_masks import oracle_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.0
BAND = 129                  # floats of sentinel on either side of every carved tensor
LEVELS, T_TABLE = 3, 5      # levels of the noise table; rows of the level table (more than the noise table holds)


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
def carve(values):
    """(view, buffer): ``values`` on the device in the middle of a sentinel-filled buffer"""
    buf = torch.full((values.numel() + 2 * BAND,), SENTINEL, dtype=values.dtype, device=DEV)
    view = buf[BAND: BAND + values.numel()].view(values.shape)
    view.copy_(values)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + BAND * values.element_size()
    return view, buf


def bands_intact(buf):
    return bool((buf[:BAND] == SENTINEL).all()) and bool((buf[-BAND:] == SENTINEL).all())


def patterns(b, N, g):
    alt = (torch.arange(b * N).view(b, N) % 2).float()
    return {"all": torch.ones(b, N), "none": torch.zeros(b, N), "alternating": alt, "odd-valued": alt * 0.75 + 0.25 * (torch.rand(b, N, generator=g) < 0.5),
            "null": None}


def counters(b):
    if b == 1:
        return [[-1], [0], [LEVELS - 1], [LEVELS]]
    return [[-1, 0, LEVELS], [LEVELS - 1, LEVELS + 4, -1], [0, LEVELS - 1, -3]]


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 257])
def test_kernel_equals_the_restatement(N, b):
    """'odd-valued' holds 0.25 / 0.75 / 1.0: the kernel's test is >= 0.5, the restatement's too.  Every output is compared whole, so an
    unkept row, a sample whose level the table does not hold, and the tensors that were only read must come back as they went in."""
    g = torch.Generator().manual_seed(1000 * b + N)
    r = lambda *shape: torch.randn(*shape, generator=g)       # noqa: E731
    level = torch.rand(T_TABLE, 2, generator=g)
    host = dict(z=r(b, N, 3), seq_t=r(b, N, 21), x0c=4.0 * r(b, N, 3), noise=r(LEVELS, b, N, 3), seq0=r(b, N, 21))
    pats = patterns(b, N, g)
    for ts in counters(b):
        t_host = torch.tensor(ts, dtype=torch.int64)
        for kz_name, kz in pats.items():
            for ks_name, ks in pats.items():
                if kz is None and ks is None and ts != counters(b)[0]:
                    continue
                dev = {k: carve(v) for k, v in host.items()}
                t, t_buf = carve(t_host)
                masks = {k: carve(v) if v is not None else (None, None) for k, v in (("keep_z", kz), ("keep_seq", ks))}
                lv, lv_buf = carve(level)
                kw = {}
                if kz is not None:
                    kw.update(x0c=dev["x0c"][0], keep_z=masks["keep_z"][0], noise=dev["noise"][0], level=lv)
                if ks is not None:
                    kw.update(seq0=dev["seq0"][0], keep_seq=masks["keep_seq"][0])
                condition_rows_(dev["z"][0], dev["seq_t"][0], t, **kw)
                want_z, want_s = restate_rows(host["z"], host["seq_t"], t_host, x0c=host["x0c"], keep_z=kz, noise=host["noise"], level=level,
                                              seq0=host["seq0"], keep_seq=ks)
                where = (N, b, ts, kz_name, ks_name)
                assert torch.equal(dev["z"][0].cpu(), want_z), where
                assert torch.equal(dev["seq_t"][0].cpu(), want_s), where
                for k in ("x0c", "noise", "seq0"):
                    assert torch.equal(dev[k][0].cpu(), host[k]), where + (k,)
                assert torch.equal(t.cpu(), t_host) and torch.equal(lv.cpu(), level), where
                for name, (_, buf) in list(dev.items()) + list(masks.items()) + [("t", (None, t_buf)), ("level", (None, lv_buf))]:
                    assert buf is None or bands_intact(buf), where + (name,)
    # the restatement did something on this shape: a kept row moved, at a level the table holds
    want_z, want_s = restate_rows(host["z"], host["seq_t"], torch.zeros(b, dtype=torch.int64), x0c=host["x0c"], keep_z=pats["all"],
                                  noise=host["noise"], level=level, seq0=host["seq0"], keep_seq=pats["all"])
    assert not torch.equal(want_z, host["z"]) and torch.equal(want_s, host["seq0"])


def test_two_launches_are_bit_identical():
    b, N = 3, 257
    g = torch.Generator().manual_seed(7)
    r = lambda *shape: torch.randn(*shape, generator=g).to(DEV)       # noqa: E731
    x0c, noise, seq0, level = r(b, N, 3), r(LEVELS, b, N, 3), r(b, N, 21), torch.rand(T_TABLE, 2, generator=g).to(DEV)
    keep = (torch.rand(b, N, generator=g) < 0.5).float().to(DEV)
    t = torch.tensor([1, -1, 2], device=DEV)
    outs = []
    for _ in range(2):
        z, seq = torch.full((b, N, 3), float("nan"), device=DEV), torch.full((b, N, 21), float("nan"), device=DEV)
        condition_rows_(z, seq, t, x0c=x0c, keep_z=keep, noise=noise, level=level, seq0=seq0, keep_seq=keep)
        outs.append((z, seq))
    rows = keep >= 0.5
    assert torch.isfinite(outs[0][0][rows]).all() and torch.isnan(outs[0][0][~rows]).all() and torch.isnan(outs[0][1][~rows]).all()
    assert torch.equal(outs[0][0][rows], outs[1][0][rows]) and torch.equal(outs[0][1][rows], outs[1][1][rows])


def test_entry_refuses_by_code_before_any_launch():
    b, N = 2, 5
    z, seq = torch.full((b, N, 3), 7.0, device=DEV), torch.full((b, N, 21), 7.0, device=DEV)
    x0c, noise, seq0 = torch.zeros(b, N, 3, device=DEV), torch.zeros(LEVELS, b, N, 3, device=DEV), torch.zeros(b, N, 21, device=DEV)
    keep, level, t = torch.ones(b, N, device=DEV), torch.ones(LEVELS, 2, device=DEV), torch.zeros(b, dtype=torch.int64, device=DEV)
    f, D = conditioning.lib().prd_condition_rows, conditioning._DEFINES
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None      # noqa: E731

    def call(b=b, N=N, n_cls=21, levels=LEVELS, keep_z=keep, keep_seq=keep, t=t, x0c=x0c):
        return f(ptr(z), ptr(seq), ptr(t), ptr(x0c), ptr(keep_z), ptr(noise), ptr(level), ptr(seq0), ptr(keep_seq), b, N, n_cls, levels, None)
    for kw in (dict(b=0), dict(N=0), dict(b=-2), dict(levels=0), dict(t=None), dict(x0c=None)):
        assert call(**kw) == D["ERR_ARG"], kw
    for kw in (dict(n_cls=20), dict(n_cls=22), dict(b=D["MAX_B"] + 1)):
        assert call(**kw) == D["ERR_UNSUPPORTED"], kw
    assert call(keep_z=None, keep_seq=None, n_cls=20) == 0          # nothing to hold: no launch, n_cls is not looked at
    torch.cuda.synchronize()
    assert float(z.min()) == float(z.max()) == 7.0 and float(seq.min()) == float(seq.max()) == 7.0
    assert call(n_cls=20, keep_seq=None) == 0                       # n_cls counts only with keep_seq
    assert float(z.abs().max()) == 0.0 and float(seq.min()) == 7.0
    with pytest.raises(ValueError, match="21 classes"):
        condition_rows_(z, torch.zeros(b, N, 20, device=DEV), t, seq0=torch.zeros(b, N, 20, device=DEV), keep_seq=keep)
    with pytest.raises(ValueError, match="level must be"):
        condition_rows_(z, seq, t, x0c=x0c, keep_z=keep, noise=noise, level=level[:2])
    with pytest.raises(ValueError, match="contiguous"):
        condition_rows_(z, seq, t, x0c=x0c, keep_z=keep.t().contiguous().t(), noise=noise, level=level)


# ---------------------------------------------------------------------------------------------------
# 2. the loop
# ---------------------------------------------------------------------------------------------------
SEED = 9


@pytest.fixture(scope="module")
def setup():
    """model, CPU batch, the design region (the pocket within 12 Angstrom as explicit positions: the sources are then not consulted for a
    permutation) and, computed once, the unconditioned run every test compares with: its initial state, final state and result."""
    args, params, batch, model = sample_setup()
    extra, inv = restated_spec_masks(batch, "within", 12.0)
    assert 0 < int(inv.sum()) < int(batch["residue_mask"].sum())
    region = Redesign.positions(inv).to(DEV)
    loop = ReverseDiffusion(model, batch_to(clone_batch(batch), DEV), [NoiseSource(SEED, 0)], redesign=region)
    init = (loop._init[0].clone(), loop._init[1].clone())
    loop.run()
    pos, logits = loop.result()
    plain = dict(init=init, z=loop.z.clone(), pos=pos.clone(), logits=logits.clone())
    return dict(args=args, params=params, batch=batch, model=model, extra=extra, inv=inv, region=region, plain=plain)


def conditioned(setup, scaffold, run=True):
    loop = ReverseDiffusion(setup["model"], batch_to(clone_batch(setup["batch"]), DEV), [NoiseSource(SEED, 0)], redesign=setup["region"],
                            scaffold=scaffold.to(DEV))
    if run:
        loop.run()
    return loop


def frame(loop):
    """(x0c, centre over the valid rows) as the loop documents them: remove_mean of batch['x'] and the masked mean"""
    x0, valid = loop.batch["x"], loop.mask.unsqueeze(-1)
    centre = (valid * x0).sum(dim=1, keepdim=True) / valid.sum(dim=1, keepdim=True)
    return ops.remove_mean(x0.contiguous(), loop.mask), centre


def half_kept(setup):
    """every other residue, over the collated row"""
    rm = setup["batch"]["residue_mask"][0]
    keep = torch.zeros_like(rm)
    keep[torch.nonzero(rm > 0.5).flatten()[::2]] = 1
    return keep


def test_nothing_kept_changes_nothing(setup):
    """An all-zero keep mask: the launch runs after every boundary and holds no row.  State and logits are bit-identical to the
    unconditioned loop on the same sources -- so the draws of an unconditioned loop are what they were, the conditioning noise comes
    after them -- and the positions are that state in the input's frame, 10 (z + centre), as with every scaffold."""
    plain, model = setup["plain"], setup["model"]
    loop = conditioned(setup, Scaffold(torch.zeros(27)), run=False)
    assert loop.cond is not None and float(loop.keep.sum()) == 0 and loop.cond_noise.shape == (4, 1, 27, 3)
    assert torch.equal(loop._init[0], plain["init"][0]) and torch.equal(loop._init[1], plain["init"][1])
    loop.run()
    pos, logits = loop.result()
    assert torch.equal(loop.z, plain["z"]) and torch.equal(logits, plain["logits"])
    _, centre = frame(loop)
    assert torch.equal(pos, 10.0 * (plain["z"] + loop.mask.unsqueeze(-1) * centre))
    # through sample(): the same, and without the keyword sample() is what it was
    d = batch_to(clone_batch(setup["batch"]), DEV)
    pos2, logits2 = model.sample(d, sources=[NoiseSource(SEED, 0)], redesign=setup["region"], scaffold=Scaffold(torch.zeros(27)))
    assert torch.equal(pos2, pos) and torch.equal(logits2, logits) and float(d[conditioning.BATCH_KEY].sum()) == 0
    pos3, logits3 = model.sample(batch_to(clone_batch(setup["batch"]), DEV), sources=[NoiseSource(SEED, 0)], redesign=setup["region"])
    assert torch.equal(pos3, plain["pos"]) and torch.equal(logits3, plain["logits"])


def test_kept_rows_come_back_at_the_input(setup):
    """Everything kept: the positions equal 10 (x0c + centre) bit for bit, which is the input to within four fp32 roundings at <= 20 nm
    (2^-23 * 20 nm = 2.4e-5 Angstrom each), two orders below the 1e-3 Angstrom asserted.  Half kept: the kept rows likewise, and the
    free rows are not where the unconditioned run put them."""
    batch, plain = setup["batch"], setup["plain"]
    given = (batch["atom_mask"].unsqueeze(-1) * batch["atom_pos"] + batch["residue_mask"].unsqueeze(-1) * batch["residue_atom_pos"][:, :, 1]).to(DEV)
    assert float(given.abs().max()) <= 100.0
    loop = conditioned(setup, Scaffold(torch.ones(27), ligand=True))
    valid = loop.mask > 0.5
    assert torch.equal(loop.keep, loop.mask) and int(valid.sum()) == 25
    x0c, centre = frame(loop)
    pos, _ = loop.result()
    want = 10.0 * (x0c + centre)
    assert torch.equal(loop.z[valid], x0c[valid]) and torch.equal(pos[valid], want[valid])
    err = float((pos[valid] - given[valid]).abs().max())
    print(f"\nkept rows against the input: {err:.2e} Angstrom")
    assert err <= 1e-3
    keep = half_kept(setup)
    loop = conditioned(setup, Scaffold(keep, ligand=True))
    pos, logits = loop.result()
    kept = loop.keep > 0.5
    assert int(kept.sum()) == 5 + 10 and torch.equal(kept.cpu()[0], (keep + batch["atom_mask"][0]) > 0.5)
    assert torch.equal(pos[kept], want[kept]) and float((pos[kept] - given[kept]).abs().max()) <= 1e-3
    free = valid & ~kept
    assert int(free.sum()) == 10 and bool(torch.isfinite(pos).all()) and bool(torch.isfinite(logits).all())
    moved = (loop.z[free] - plain["z"][free]).abs().amax(dim=-1)
    assert bool((moved > 0).all()), moved


@pytest.mark.parametrize("sequence", [False, True])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_graph_replay_equals_eager_stepping(setup, monkeypatch, fused, sequence):
    monkeypatch.setenv("PRD_FUSED_BOUNDARY", fused)
    model = setup["model"]
    spec = Scaffold(half_kept(setup), ligand=True, sequence=sequence)
    out = {}
    try:
        for graph in (False, True):
            model.use_hip_graph = graph
            loop = conditioned(setup, spec)
            assert loop.fused_boundary == (fused == "1") and (loop.graph is not None) == graph
            out[graph] = (loop.z.clone(), loop.seq_t.clone(), *[x.clone() for x in loop.result()])
            if graph:                           # a second pass over the captured graph from the stored initial state
                loop.reset()
                loop.run()
                assert all(torch.equal(a, b) for a, b in zip(out[True], (loop.z, loop.seq_t, *loop.result())))
    finally:
        model.use_hip_graph = True
    assert all(torch.equal(a, b) for a, b in zip(out[False], out[True]))
    known = loop.batch["residue_extra_mask"] > 0.5
    clamped = torch.equal(out[True][1][known], loop.batch["residue_one_hot"][known])
    assert int(known.sum()) > 0 and clamped == sequence     # without the option every row is 2 softmax - 1 after the first step
    if sequence:
        assert not torch.equal(out[True][3], conditioned(setup, Scaffold(half_kept(setup), ligand=True)).result()[1])


@pytest.mark.parametrize("L", [0, 1, 3])
def test_partial_diffusion_equals_a_restarted_loop(setup, L):
    """Scaffold(None, start=L) against an unconditioned loop restarted at step T - 1 - L from z_L = A[L] x0c + S[L] eps_L on the valid
    rows, eps_L being the FIRST conditioning draw of a copy of the source: after z_T, seq_T and the T - 1 reverse-update tensors."""
    model, plain, T = setup["model"], setup["plain"], 4
    part = conditioned(setup, Scaffold(None, start=L), run=False)
    assert part.cond is None and part.cond_noise.shape == (L + 1, 1, 27, 3) and int(part.t[0]) == L and part.steps_done == T - 1 - L
    steps = 0
    while part.steps_done < T:
        part.step()
        steps += 1
    assert steps == L + 1 and int(part.t[0]) == -1
    with pytest.raises(RuntimeError, match="already done"):
        part.step()
    src = NoiseSource(SEED, 0)
    for shape in [(27, 3), (27, 21)] + [(27, 3)] * (T - 1):
        src.randn(*shape)
    free = ReverseDiffusion(model, batch_to(clone_batch(setup["batch"]), DEV), [NoiseSource(SEED, 0)], redesign=setup["region"])
    eps = ops.remove_mean(src.randn(27, 3)[None].to(DEV).contiguous(), free.mask)
    x0c, _ = frame(free)
    z_L = torch.where(free.mask.unsqueeze(-1) > 0.5, model.sqrt_alphas_cumprod[L] * x0c + model.sqrt_one_minus_alphas_cumprod[L] * eps, plain["init"][0])
    assert torch.equal(part._init[0], z_L) and torch.equal(part._init[1], plain["init"][1])
    free.restart(T - 1 - L, z_L, plain["init"][1])
    free.run()
    assert torch.equal(part.z, free.z) and torch.equal(part.result()[1], free.result()[1])
    _, centre = frame(part)
    assert torch.equal(part.result()[0], 10.0 * (free.z + free.mask.unsqueeze(-1) * centre))
    part.reset()                                # back to level L, not to T - 1
    assert int(part.t[0]) == L and part.steps_done == T - 1 - L
    part.run()
    assert torch.equal(part.z, free.z)
    with pytest.raises(ValueError, match="start"):
        conditioned(setup, Scaffold(None, start=T), run=False)


def oracle_conditioned_loop(setup, keep, clamp):
    """The conditioned loop on the CPU, written from the oracle's network, schedule and remove_mean: positions (input frame) and logits"""
    params, args, batch, T = setup["params"], setup["args"], setup["batch"], 4
    pb = oracle_batch(batch, setup["extra"], setup["inv"])
    sch = O.schedule_tables(T, "linear")
    A, S = sch["sqrt_alphas_cumprod"], sch["sqrt_one_minus_alphas_cumprod"]
    mask, rm, seq0, known = pb["residue_and_atom_mask"], pb["residue_mask"], pb["residue_one_hot"], pb["residue_extra_mask"] > 0.5
    src = NoiseSource(SEED, 0)
    z = O.remove_mean(src.randn(27, 3)[None], mask)
    seq_t = O.remove_mean(src.randn(27, 21)[None], rm)
    seq_t = pb["residue_extra_mask"].unsqueeze(-1) * seq0 + pb["residue_inv_extra_mask"].unsqueeze(-1) * seq_t
    step_noise = [O.remove_mean(src.randn(27, 3)[None], mask) for _ in range(T - 1)]
    eps = {T - 1 - j: O.remove_mean(src.randn(27, 3)[None], mask) for j in range(T)}         # drawn for the levels T-1 .. 0, in that order
    x0c = O.remove_mean(pb["x"], mask)
    centre = (mask.unsqueeze(-1) * pb["x"]).sum(1, keepdim=True) / mask.sum(1, keepdim=True).unsqueeze(-1)
    K = keep > 0.5

    def hold(z, seq_t, l):
        z = z.clone()
        z[K] = x0c[K] if l < 0 else (A[l] * x0c + S[l] * eps[l])[K]
        if clamp:
            seq_t = seq_t.clone()
            seq_t[known] = seq0[known]
        return z, seq_t
    z, seq_t = hold(z, seq_t, T - 1)
    for i in range(T):
        tt = T - 1 - i
        t = torch.full((1,), tt, dtype=torch.long)
        noise_pred, seq_pred = O.network_step(params, args, pb, z, seq_t, mask, t)
        w_noise = (1.0 - sch["alphas"][t]) / S[t]
        z = (1.0 / sch["sqrt_alphas"][t])[:, None, None] * (z - w_noise[:, None, None] * noise_pred)
        seq_t = torch.softmax(seq_pred, dim=-1) * 2 - 1
        if tt > 0:
            z = z + sch["sqrt_betas"][t][:, None, None] * step_noise[i]
        z, seq_t = hold(z, seq_t, tt - 1)
    return 10.0 * (z + mask.unsqueeze(-1) * centre), rm.unsqueeze(-1) * seq_pred, z


@pytest.mark.parametrize("clamp", [False, True])
def test_conditioned_loop_matches_the_oracle(setup, clamp):
    """Half of the residues and the ligand kept.  The kept rows are part of the comparison; the centred state is compared as well as the
    positions, whose norm the centre of the complex inflates."""
    keep = half_kept(setup)
    with torch.inference_mode():
        want_pos, want_logits, want_z = oracle_conditioned_loop(setup, (keep + setup["batch"]["atom_mask"][0])[None], clamp)
    loop = conditioned(setup, Scaffold(keep, ligand=True, sequence=clamp))
    pos, logits = loop.result()
    e_pos, e_log, e_z = rel_l2(pos.cpu(), want_pos), rel_l2(logits.cpu(), want_logits), rel_l2(loop.z.cpu(), want_z)
    print(f"\nconditioned loop (sequence clamp {clamp}) vs oracle: positions {e_pos:.2e}, centred state {e_z:.2e}, logits {e_log:.2e}")
    assert e_pos < TRAJ_TOL and e_log < TRAJ_TOL and e_z < TRAJ_TOL


@pytest.mark.parametrize("kind", ["outside", "beyond", "mask"])
def test_a_conditioned_loop_is_set_up_and_run_without_host_synchronisation(setup, kind):
    """prepare_batch, the conditioning set-up (x0c, centre, K, the tables: uploaded from pinned memory, where a pageable copy would wait
    for the device), the first step, the capture of the step graph and its replays."""
    model = setup["model"]
    spec = {"outside": Scaffold("outside", ligand=True, sequence=True), "beyond": Scaffold.beyond(12.0, sequence=True, start=2),
            "mask": Scaffold(half_kept(setup), ligand=True)}[kind].to(DEV)
    conditioned(setup, spec)                    # warm: library, allocators, the constant tables of the model
    d = batch_to(clone_batch(setup["batch"]), DEV)
    sources = [NoiseSource(SEED, 0)]

    def work():
        loop = ReverseDiffusion(model, d, sources, redesign=setup["region"], scaffold=spec)
        loop.run()
        return loop
    loop = run_without_host_sync(work)
    assert loop.steps_done == 4 and loop.finite() and loop.graph is not None        # (start=2: three steps, the second one captured)
    if kind == "beyond":                        # farther than 12 Angstrom from every ligand atom: the complement of the design region
        assert torch.equal(loop.keep.cpu(), setup["extra"])
    if kind == "outside":
        assert torch.equal(loop.keep.cpu(), setup["extra"] + setup["batch"]["atom_mask"])


# ---------------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------------
def test_generate_samples_end_to_end(tmp_path):
    """Redesign the pocket within 8 Angstrom, keep everything outside it and the ligand where the input has them, score against the
    input.  The fixture (8 atoms + 40 residues, seed 0) has 14 pocket residues, the nearest C-alpha 0.24 Angstrom from the 8 Angstrom
    shell, and 10 kept residues all of whose neighbours within the lDDT radius are kept too."""
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    from protein_redesign_amd.quality import LDDT_RADIUS
    from protein_redesign_amd.synthetic import deterministic_state_dict, synthetic_sample
    from protein_redesign_amd.weights import spec_tensors
    NA, NR = 8, 40
    args = make_args(single_dim=128, pair_dim=64, num_blocks=2, esm_dim=64, num_steps=4, mask_prob=0.3)
    model = ProteinReDiffModel(args)
    model.load_state_dict(deterministic_state_dict(spec_tensors(args), seed=1))
    model = model.to(DEV).eval()
    data = synthetic_sample(NA, NR, esm_dim=64, seed=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        out = PL.generate_samples(model, data, num_samples=3, batch_size=2, seed=4, output_dir=tmp_path, redesign=Redesign.within(8.0),
                                  scaffold=Scaffold("outside", ligand=True), assess="input")
    assert len(out) == 7
    pos, used_mask, quality, kept = out[0], out[4], out[5], out[6]
    assert sorted(kept) == ["keep", "ligand", "sequence", "start"] and (kept["ligand"], kept["sequence"], kept["start"]) == (True, False, None)
    keep = kept["keep"] > 0.5
    assert int(used_mask.sum()) == 14 and np.array_equal(keep[NA:], used_mask[NA:] < 0.5) and keep[:NA].all() and int(keep.sum()) == NA + NR - 14
    given = np.concatenate([data["atom_pos"].numpy(), data["residue_atom_pos"][:, 1].numpy()]).astype(np.float32)
    assert float(np.abs(given).max()) <= 100.0
    err = float(np.abs(pos[:, keep] - given[keep]).max())
    print(f"\nkept rows of {pos.shape[0]} samples against the input: {err:.2e} Angstrom")
    assert err <= 1e-3
    free = ~keep
    assert all(np.abs(pos[s, free] - given[free]).max() > 1e-2 for s in range(3)) and np.abs(pos[0, free] - pos[1, free]).max() > 1e-2
    # lDDT-C-alpha of a kept residue whose neighbours within the radius are all kept: every distance it counts is the input's own
    ca = given[NA:].astype(np.float64)
    near = (np.linalg.norm(ca[:, None] - ca[None], axis=-1) < LDDT_RADIUS - 1e-3) & ~np.eye(NR, dtype=bool)
    margin = (np.linalg.norm(ca[:, None] - ca[None], axis=-1) < LDDT_RADIUS + 1e-3) & ~np.eye(NR, dtype=bool)
    sure = keep[NA:] & ~(margin & ~keep[NA:][None]).any(1) & near.any(1)
    assert int(sure.sum()) == 10
    assert (quality["lddt_ca_per_residue"][:, sure] == 1.0).all() and quality["lddt_ca_per_residue"].shape == (3, NR)
    assert (quality["lddt_ca"] < 1.0).all()                     # the pocket was rebuilt
    assert sorted(os.listdir(tmp_path)) == ["sample_ligand_pos.npy", "sample_protein.pdb", "sample_quality.npz", "sample_quality.txt",
                                            "sample_redesign_mask.npy", "sample_scaffold.npz"]
    with np.load(tmp_path / "sample_scaffold.npz") as z:
        assert np.array_equal(z["keep"], kept["keep"]) and bool(z["ligand"]) and not bool(z["sequence"]) and int(z["start"]) == -1
    assert np.array_equal(np.load(tmp_path / "sample_ligand_pos.npy"), pos[:, :NA])
