"""GPU: sequence rules at inference (sequence.SequenceRules / Decode, libprd_sequence.so, ReverseDiffusion(sequence_rules=...)).

1. The kernels against the torch restatements of protein_redesign_amd/sequence.py (fp32 ``logits + bias``, float64 after it; held against
   straight float64 formulas by tests/test_sequence_rules_cpu.py): prd_sequence_constrain on rows of 1 .. 257 positions (63 / 64 / 65: a
   wave of two-row halves, 257: more than one workgroup and a ragged tail of one row in eight), 1 and 3 samples, shared and per-sample
   tables, every row pattern and NULL, tensors carved out of sentinel-filled buffers; the hard rows; bit-reproducibility;
   prd_sequence_decode (argmax and Gumbel-max at temperatures 0.5 and 2, ties, bans); prd_sequence_census against numpy; the refusals.
2. The loop: a spec that rules no row changes nothing; graph replay equals eager stepping; the loop against one written here from the
   oracle's network; an omitted residue never reaches the network nor the output; allow / bias at one position; no host synchronisation.
3. pipeline.generate_samples end to end with rules and device decoding.

Measured on an MI355X (printed by the tests): see the docstrings of the tests that assert a tolerance.

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
from protein_redesign_amd import _lib
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd import sequence as SQ
from protein_redesign_amd.conditioning import Scaffold
from protein_redesign_amd.diffusion_model import ReverseDiffusion
from protein_redesign_amd.masking import Redesign
from protein_redesign_amd.sequence import BANNED, Decode, SequenceRules
from protein_redesign_amd.synthetic import NoiseSource, batch_to, clone_batch
from test_hip_parity import TRAJ_TOL
from test_redesign_region import restated_spec_masks, sample_setup
from test_training_masks import oracle_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.0
BAND = 129                  # floats of sentinel on either side of every carved tensor
TOL = 1e-5                  # absolute, on p-derived values: an fp32 softmax over 21 entries, an order of magnitude for a different exp


# ---------------------------------------------------------------------------------------------------
# 1. the kernels
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
    return {"all": torch.ones(b, N), "none": torch.zeros(b, N), "alternating": alt, "odd-valued": alt * 0.5 + 0.25, "null": None}


def random_table(bias_b, N, g, ban=0.3):
    """finite biases with about ``ban`` of the entries banned (a row may lose every class: the library has to be safe there)"""
    t = torch.randn(bias_b, N, 21, generator=g)
    t[torch.rand(bias_b, N, 21, generator=g) < ban] = BANNED
    return t


def check_constrain(seq_t, logits, bias, rows, where):
    """one launch on carved tensors against the restatement; returns the largest error on the allowed entries of the marked rows"""
    host = dict(seq_t=seq_t, logits=logits, bias=bias)
    dev = {k: carve(v) for k, v in host.items()}
    r_dev = carve(rows) if rows is not None else (None, None)
    SQ.constrain_rows_(dev["seq_t"][0], dev["logits"][0], dev["bias"][0], r_dev[0])
    got = dev["seq_t"][0].cpu()
    want = SQ.restate_constrain(seq_t, logits, bias, rows)
    for k in ("logits", "bias"):
        assert torch.equal(dev[k][0].cpu(), host[k]), where + (k,)
    for name, (_, buf) in list(dev.items()) + [("rows", r_dev)]:
        assert buf is None or bands_intact(buf), where + (name,)
    if rows is None:
        assert torch.equal(got, seq_t), where
        return 0.0
    assert torch.equal(r_dev[0].cpu(), rows), where
    marked = rows >= 0.5
    assert torch.equal(got[~marked], seq_t[~marked]), where             # bit-equal to what went in
    banned = (bias <= BANNED).expand_as(logits)
    assert bool((got[marked][banned[marked]] == -1.0).all()), where      # exactly -1, whatever the logit
    assert bool(torch.isfinite(got[marked]).all()), where
    return float((got[marked].double() - want[marked].double()).abs().max()) if bool(marked.any()) else 0.0


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 257])
def test_constrain_equals_the_restatement(N, b):
    """Allowed entries within 1e-5 absolute of the float64 restatement; banned entries exactly -1; unmarked rows, the read-only tensors
    and the bands bit-equal to what went in.  'odd-valued' holds 0.25 / 0.75: the kernel's test is >= 0.5, the restatement's too.
    Measured on an MI355X: at most 3.6e-07 over all shapes and patterns."""
    g = torch.Generator().manual_seed(1000 * b + N)
    seq_t, logits = torch.randn(b, N, 21, generator=g), 3.0 * torch.randn(b, N, 21, generator=g)
    worst = 0.0
    for bias_b in sorted({1, b}):
        bias = random_table(bias_b, N, g)
        for name, rows in patterns(b, N, g).items():
            worst = max(worst, check_constrain(seq_t, logits, bias, rows, (N, b, bias_b, name)))
    print(f"\nconstrain vs restatement, N {N} b {b}: {worst:.2e}")
    assert worst <= TOL
    want = SQ.restate_constrain(seq_t, logits, bias, torch.ones(b, N))      # the restatement did something on this shape
    assert not torch.equal(want, seq_t) and bool((want[(bias <= BANNED).expand_as(want)] == -1).all())


def test_constrain_on_the_hard_rows():
    """Every row finite and within 1e-5 of the restatement: logits scaled by 400 and by 1e4; the only allowed class holding the lowest
    logit (p = 1 there, exactly); a banned class 5e4 above every allowed one (still exactly -1: the ban is a test, not a fill); every
    class banned (all -1, no NaN); finite biases of +-20.  Measured on an MI355X: 6.0e-08."""
    g = torch.Generator().manual_seed(5)
    base = torch.randn(1, 8, 21, generator=g)
    logits, bias = base.clone(), torch.zeros(1, 8, 21)
    logits[0, 0] *= 400.0
    logits[0, 1] *= 1e4
    low = int(logits[0, 2].argmin())
    bias[0, 2] = BANNED
    bias[0, 2, low] = 0.0
    logits[0, 3, 7] = float(logits[0, 3].max()) + 5e4
    bias[0, 3, 7] = BANNED
    bias[0, 4] = BANNED
    bias[0, 5] = 20.0 * (2.0 * (torch.rand(21, generator=g) < 0.5).float() - 1.0)
    logits[0, 6] = 1e4 * base[0, 6]
    bias[0, 6, ::2] = BANNED
    seq_t = torch.randn(1, 8, 21, generator=g)
    err = check_constrain(seq_t, logits, bias, torch.ones(1, 8), ("hard",))
    out = seq_t.to(DEV).contiguous()
    SQ.constrain_rows_(out, logits.to(DEV), bias.to(DEV), torch.ones(1, 8, device=DEV))
    out = out.cpu()
    print(f"\nconstrain on the hard rows vs restatement: {err:.2e}")
    assert err <= TOL and bool(torch.isfinite(out).all())
    assert float(out[0, 2, low]) == 1.0 and int((out[0, 2] == -1.0).sum()) == 20
    assert float(out[0, 3, 7]) == -1.0 and float(out[0, 3].max()) > -1.0
    assert bool((out[0, 4] == -1.0).all())


def test_two_launches_are_bit_identical():
    b, N = 3, 257
    g = torch.Generator().manual_seed(7)
    logits, bias = (3.0 * torch.randn(b, N, 21, generator=g)).to(DEV), random_table(b, N, g).to(DEV)
    rows = (torch.rand(b, N, generator=g) < 0.5).float().to(DEV)
    outs = []
    for _ in range(2):
        seq = torch.full((b, N, 21), float("nan"), device=DEV)
        SQ.constrain_rows_(seq, logits, bias, rows)
        outs.append(seq)
    marked = rows >= 0.5
    assert torch.isfinite(outs[0][marked]).all() and torch.isnan(outs[0][~marked]).all()
    assert torch.equal(outs[0][marked], outs[1][marked])


def decode_case(S, N, temperature, g, bias_b):
    """inputs on the CPU whose two largest keys are at least 1e-3 apart in float64 on every row: where a draw leaves them closer, the
    logit of the winner is raised by 0.01 * temperature-or-1 until they are not (a condition on the inputs; no row is left out)"""
    logits, bias = 3.0 * torch.randn(S, N, 21, generator=g), random_table(bias_b, N, g)
    bias[:, :, 20] = torch.randn(bias_b, N, generator=g)        # one class is always allowed
    gumbel = -torch.log(-torch.log(torch.rand(S, N, 21, generator=g).clamp_(min=1e-30))) if temperature > 0 else None
    allowed = (bias > BANNED).expand_as(logits)

    def top_two(logits):
        x = (logits + torch.where(bias > BANNED, bias, torch.zeros_like(bias))).double()
        key = x if gumbel is None else x / temperature + gumbel.double()
        top2 = torch.where(allowed, key, torch.full_like(key, -float("inf"))).topk(2, dim=-1)
        return (top2.values[..., 0] - top2.values[..., 1]) < 1e-3, top2.indices[..., :1]
    for _ in range(4):
        close, winner = top_two(logits)
        bump = torch.zeros_like(logits)
        bump.scatter_(-1, winner, 0.01 * (temperature if temperature > 0 else 1.0))
        logits = logits + bump * close.unsqueeze(-1)
    assert not bool(top_two(logits)[0].any())
    return logits, bias, gumbel


@pytest.mark.parametrize("temperature", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("S,N", [(1, 1), (3, 65), (2, 257)])
def test_decode_equals_the_restatement(S, N, temperature):
    """Tokens exactly; logp and entropy within 1e-5 absolute (logits of scale 3, so |logp| is of order 10 and its fp32 ulp 1e-6);
    unmarked rows -1 / 0 / 0; no banned token.  Measured on an MI355X: logp at most 8.5e-07, entropy at most 2.7e-07."""
    g = torch.Generator().manual_seed(100 * S + N + int(10 * temperature))
    worst = [0.0, 0.0]
    for bias_b in sorted({1, S}):
        logits, bias, gumbel = decode_case(S, N, temperature, g, bias_b)
        for name, rows in patterns(S, N, g).items():
            if rows is None:
                continue
            dev = {k: carve(v) for k, v in dict(logits=logits, bias=bias, rows=rows, **({"gumbel": gumbel} if gumbel is not None else {})).items()}
            tokens, logp, entropy = SQ.decode(dev["logits"][0], dev["rows"][0], bias=dev["bias"][0],
                                              gumbel=dev["gumbel"][0] if gumbel is not None else None, temperature=temperature)
            want_t, want_lp, want_h = SQ.restate_decode(logits, rows, bias, gumbel, temperature)
            where = (S, N, temperature, bias_b, name)
            assert all(bands_intact(buf) for _, buf in dev.values()) and all(torch.equal(v.cpu(), h) for (v, _), h in
                                                                            zip(dev.values(), [logits, bias, rows] + [gumbel] * (gumbel is not None))), where
            tokens, logp, entropy = tokens.cpu(), logp.cpu(), entropy.cpu()
            assert tokens.dtype == torch.int32 and torch.equal(tokens, want_t), where
            marked = rows >= 0.5
            assert bool((tokens[~marked] == -1).all()) and bool((logp[~marked] == 0).all()) and bool((entropy[~marked] == 0).all()), where
            picked = torch.gather((bias <= BANNED).expand_as(logits), -1, tokens.clamp(min=0).long().unsqueeze(-1)).squeeze(-1)
            assert not bool(picked[marked].any()) and bool((tokens[marked] >= 0).all()), where
            worst[0] = max(worst[0], float((logp.double() - want_lp).abs().max()))
            worst[1] = max(worst[1], float((entropy.double() - want_h).abs().max()))
    print(f"\ndecode vs restatement, S {S} N {N} T {temperature}: logp {worst[0]:.2e}, entropy {worst[1]:.2e}")
    assert worst[0] <= TOL and worst[1] <= TOL


def test_decode_resolves_ties_to_the_lowest_index_and_works_without_a_bias():
    logits = torch.zeros(1, 5, 21)
    bias = torch.zeros(1, 5, 21)
    logits[0, 1, [5, 9]] = 2.0                  # a tie of two
    logits[0, 2, [5, 9]] = 2.0                  # ... the lower one banned
    bias[0, 2, 5] = BANNED
    bias[0, 3, :4] = BANNED                     # all equal, the first four banned
    bias[0, 4] = BANNED                         # nothing allowed: -1 / 0 / 0
    rows = torch.ones(1, 5)
    tokens, logp, entropy = SQ.decode(logits.to(DEV), rows.to(DEV), bias=bias.to(DEV))
    assert tokens.cpu().tolist() == [[0, 5, 9, 4, -1]] and float(logp[0, 4]) == 0.0 and float(entropy[0, 4]) == 0.0
    assert abs(float(entropy[0, 0]) - np.log(21)) <= TOL and abs(float(logp[0, 3]) + np.log(17)) <= TOL
    tokens, logp, entropy = SQ.decode(logits.to(DEV), rows.to(DEV))
    want = SQ.restate_decode(logits, rows)
    assert torch.equal(tokens.cpu(), want[0]) and tokens.cpu().tolist() == [[0, 5, 5, 0, 0]]
    assert float((logp.cpu().double() - want[1]).abs().max()) <= TOL and float((entropy.cpu().double() - want[2]).abs().max()) <= TOL


def numpy_census(tokens, mask, ref):
    S, N = tokens.shape
    on = mask >= 0.5
    identity = np.zeros((S, S), np.int32)
    for s in range(S):
        for r in range(S):
            identity[s, r] = int((on & (tokens[s] >= 0) & (tokens[s] == tokens[r])).sum())
    recovery = None if ref is None else np.array([int((on & (tokens[s] >= 0) & (tokens[s] == ref)).sum()) for s in range(S)], np.int32)
    profile = np.zeros((N, 21), np.int32)
    for i in range(N):
        if on[i]:
            for s in range(S):
                if tokens[s, i] >= 0:
                    profile[i, tokens[s, i]] += 1
    return identity, recovery, profile


@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("N", [1, 64, 257])
@pytest.mark.parametrize("S", [1, 2, 65])
def test_census_equals_numpy(S, N, with_ref):
    """exactly; tokens hold -1, the mask is partial, the outputs are pre-filled with garbage (the call writes every element itself)"""
    g = torch.Generator().manual_seed(S * 1000 + N)
    tokens = torch.randint(-1, 4, (S, N), generator=g, dtype=torch.int32)       # few classes: samples agree often
    tokens[:, ::7] = torch.randint(0, 21, (S, len(range(0, N, 7))), generator=g, dtype=torch.int32)
    mask = (torch.rand(N, generator=g) < 0.7).float()
    mask[0] = 1.0
    ref = torch.randint(-1, 4, (N,), generator=g, dtype=torch.int32) if with_ref else None
    t, t_buf = carve(tokens)
    m, m_buf = carve(mask)
    r, r_buf = carve(ref) if with_ref else (None, None)
    out = [carve(torch.full(shape, -77, dtype=torch.int32)) for shape in ((S, S), (S,), (N, 21))]
    identity, recovery, profile = SQ.census(t, m, r, out=(out[0][0], out[1][0] if with_ref else None, out[2][0]))
    want = numpy_census(tokens.numpy(), mask.numpy(), ref.numpy() if with_ref else None)
    assert np.array_equal(identity.cpu().numpy(), want[0]) and np.array_equal(profile.cpu().numpy(), want[2])
    if with_ref:
        assert np.array_equal(recovery.cpu().numpy(), want[1])
    else:
        assert recovery is None and bool((out[1][0] == -77).all())
    assert all(bands_intact(buf) for buf in (t_buf, m_buf, out[0][1], out[1][1], out[2][1])) and (r_buf is None or bands_intact(r_buf))
    assert torch.equal(t.cpu(), tokens) and torch.equal(m.cpu(), mask)
    torch_want = SQ.restate_census(tokens, mask, ref)
    assert np.array_equal(torch_want[0].numpy(), want[0]) and np.array_equal(torch_want[2].numpy(), want[2])
    fresh = SQ.census(t, m, r)                                                   # tensors of the call's own
    assert torch.equal(fresh[0], identity) and torch.equal(fresh[2], profile)


def test_entries_refuse_by_code_before_any_launch():
    b, N = 2, 5
    seq, logits = torch.full((b, N, 21), 7.0, device=DEV), torch.zeros(b, N, 21, device=DEV)
    bias, rows = torch.zeros(b, N, 21, device=DEV), torch.ones(b, N, device=DEV)
    tokens, logp = torch.full((b, N), 7, dtype=torch.int32, device=DEV), torch.full((b, N), 7.0, device=DEV)
    ident, prof, mask = torch.full((b, b), 7, dtype=torch.int32, device=DEV), torch.full((N, 21), 7, dtype=torch.int32, device=DEV), torch.ones(N, device=DEV)
    L, D = SQ.lib(), SQ._DEFINES
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None      # noqa: E731

    def constrain(b=b, N=N, n_cls=21, bias_b=b, seq=seq, logits=logits, rows=rows):
        return L.prd_sequence_constrain(ptr(seq), ptr(logits), ptr(bias), ptr(rows), b, N, n_cls, bias_b, None)

    def decode(S=b, N=N, n_cls=21, bias_b=b, tokens=tokens, rows=rows):
        return L.prd_sequence_decode(ptr(tokens), ptr(logp), ptr(logp), ptr(logits), ptr(bias), ptr(rows), None, 1.0, S, N, n_cls, bias_b, None)

    def census(S=b, N=N, n_cls=21, recovery=None, ref=None, mask=mask):
        return L.prd_sequence_census(ptr(ident), ptr(recovery), ptr(prof), ptr(tokens), ptr(ref), ptr(mask), S, N, n_cls, None)
    for call, name in ((constrain, "b"), (decode, "S"), (census, "S")):
        for kw in ({name: 0}, {name: -2}, dict(N=0)):
            assert call(**kw) == D["ERR_ARG"], (call.__name__, kw)
        for kw in (dict(n_cls=20), dict(n_cls=22), dict(N=D["MAX_N"] + 1), {name: D["MAX_B" if name == "b" else "MAX_S"] + 1}):
            assert call(**kw) == D["ERR_UNSUPPORTED"], (call.__name__, kw)
    for kw in (dict(bias_b=3), dict(seq=None), dict(logits=None)):
        assert constrain(**kw) == D["ERR_ARG"], kw
    for kw in (dict(bias_b=3), dict(tokens=None), dict(rows=None)):
        assert decode(**kw) == D["ERR_ARG"], kw
    for kw in (dict(recovery=tokens), dict(ref=tokens), dict(mask=None)):
        assert census(**kw) == D["ERR_ARG"], kw
    assert constrain(rows=None) == 0            # a successful no-op
    torch.cuda.synchronize()
    assert float(seq.min()) == float(seq.max()) == 7.0 and int(tokens.min()) == int(tokens.max()) == 7 and float(logp.min()) == 7.0
    assert int(ident.min()) == int(prof.min()) == 7
    with pytest.raises(ValueError, match="21 classes"):
        SQ.constrain_rows_(torch.zeros(b, N, 20, device=DEV), torch.zeros(b, N, 20, device=DEV), None, rows)
    with pytest.raises(ValueError, match="contiguous"):
        SQ.constrain_rows_(seq, logits, bias, rows.t().contiguous().t())
    with pytest.raises(ValueError, match="bias must be"):
        SQ.decode(logits, rows, bias=torch.zeros(3, N, 21, device=DEV))


# ---------------------------------------------------------------------------------------------------
# 2. the loop
# ---------------------------------------------------------------------------------------------------
SEED = 9
NA, NR, NP = 5, 20, 27


@pytest.fixture(scope="module")
def setup():
    """model, CPU batch, the design region (the pocket within 12 Angstrom as explicit positions) and, computed once, the run without
    rules that the tests compare with"""
    args, params, batch, model = sample_setup()
    extra, inv = restated_spec_masks(batch, "within", 12.0)
    assert 0 < int(inv.sum()) < int(batch["residue_mask"].sum())
    region = Redesign.positions(inv).to(DEV)
    loop = ReverseDiffusion(model, batch_to(clone_batch(batch), DEV), [NoiseSource(SEED, 0)], redesign=region)
    loop.run()
    pos, logits = loop.result()
    plain = dict(z=loop.z.clone(), seq_t=loop.seq_t.clone(), pos=pos.clone(), logits=logits.clone())
    return dict(args=args, params=params, batch=batch, model=model, extra=extra, inv=inv, region=region, plain=plain)


def ruled(setup, rules, run=True, region=None, seed=SEED, **kw):
    loop = ReverseDiffusion(setup["model"], batch_to(clone_batch(setup["batch"]), DEV), [NoiseSource(seed, 0)],
                            redesign=setup["region"] if region is None else region, sequence_rules=rules.to(DEV), **kw)
    if run:
        loop.run()
    return loop


def some_rules(scope="design"):
    return SequenceRules.for_residues(NA, NR + 2, omit="CM", allow={3: "AVLI", 11: "DE"}, bias={"G": 1.5, (7, "W"): -2.0}, scope=scope)


def test_a_spec_that_rules_no_row_changes_nothing(setup):
    """A table without any ban or bias rules no row by construction: nothing is launched, and state, positions and logits are bit-equal
    to the loop without the keyword.  Rules over a design region that turns out empty at run time do launch -- the kernel finds no
    marked row and seq_t stays what the boundary wrote -- but prd_single_init then rebuilds the coming step's single input, whose
    layer norm sums in another order than the fused boundary's: equal to rounding, not to the bit (as with Scaffold(sequence=True)).
    Measured on an MI355X against the loop without the keyword: positions 1.8e-07, logits 5.5e-07 relative L2; held to TRAJ_TOL, the
    project's bound for two fp32 evaluations of one trajectory."""
    plain, model = setup["plain"], setup["model"]
    for spec in (SequenceRules(torch.zeros(NP, 21)), SequenceRules.for_residues(NA, NR + 2, unknown=True, scope="all")):
        assert spec.inert and spec.to(DEV).inert
        got = ruled(setup, spec)
        assert got.rules is None and float(got.batch[SQ.BATCH_KEY].sum()) == 0
        assert all(torch.equal(a, b) for a, b in zip((plain["z"], plain["seq_t"], plain["pos"], plain["logits"]), (got.z, got.seq_t, *got.result())))
    # through sample(); and without the keyword sample() is what it was
    pos, logits = model.sample(batch_to(clone_batch(setup["batch"]), DEV), sources=[NoiseSource(SEED, 0)], redesign=setup["region"], sequence_rules=spec)
    assert torch.equal(pos, plain["pos"]) and torch.equal(logits, plain["logits"])
    pos, logits = model.sample(batch_to(clone_batch(setup["batch"]), DEV), sources=[NoiseSource(SEED, 0)], redesign=setup["region"])
    assert torch.equal(pos, plain["pos"]) and torch.equal(logits, plain["logits"])
    # a design region that is empty at run time
    nothing = Redesign.positions(torch.zeros(NP)).to(DEV)
    loop = ReverseDiffusion(model, batch_to(clone_batch(setup["batch"]), DEV), [NoiseSource(SEED, 0)], redesign=nothing)
    loop.run()
    got = ruled(setup, some_rules(), region=nothing)
    assert not some_rules().inert and got.rules is not None and float(got.rules[1].sum()) == 0 and float(got.batch[SQ.BATCH_KEY].sum()) == 0
    e_pos, e_log = rel_l2(got.result()[0].cpu(), loop.result()[0].cpu()), rel_l2(got.result()[1].cpu(), loop.result()[1].cpu())
    print(f"\nrules over an empty design region vs no rules: positions {e_pos:.2e}, logits {e_log:.2e}")
    assert e_pos < TRAJ_TOL and e_log < TRAJ_TOL and int((got.result()[1] == BANNED).sum()) == 0


@pytest.mark.parametrize("arith", ["split16", "fp32"])
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_graph_replay_equals_eager_stepping(setup, monkeypatch, fused, clamp, arith):
    monkeypatch.setenv("PRD_FUSED_BOUNDARY", fused)
    model = setup["model"]
    kw = dict(scaffold=Scaffold("outside", sequence=True)) if clamp else {}
    out = {}
    try:
        with _lib.arithmetic(arith):
            for graph in (False, True):
                model.use_hip_graph = graph
                loop = ruled(setup, some_rules("all"), **kw)
                assert loop.fused_boundary == (fused == "1") and (loop.graph is not None) == graph
                out[graph] = (loop.z.clone(), loop.seq_t.clone(), *[x.clone() for x in loop.result()])
                if graph:                       # a second pass over the captured graph from the stored initial state
                    loop.reset()
                    loop.run()
                    assert all(torch.equal(a, b) for a, b in zip(out[True], (loop.z, loop.seq_t, *loop.result())))
    finally:
        model.use_hip_graph = True
    assert all(torch.equal(a, b) for a, b in zip(out[False], out[True]))
    assert bool(torch.isfinite(out[True][0]).all()) and not torch.equal(out[True][1], setup["plain"]["seq_t"])
    known = loop.batch["residue_extra_mask"] > 0.5
    held = torch.equal(out[True][1][known], loop.batch["residue_one_hot"][known])
    assert int(known.sum()) > 0 and held == clamp       # a held row wins over the rules of scope 'all'


def oracle_ruled_loop(setup, rules):
    """The loop with rules on the CPU, written from the oracle's network, schedule and remove_mean; restate_constrain after each update"""
    params, args, batch, T = setup["params"], setup["args"], setup["batch"], 4
    pb = oracle_batch(batch, setup["extra"], setup["inv"])
    sch = O.schedule_tables(T, "linear")
    S = sch["sqrt_one_minus_alphas_cumprod"]
    mask, rm, seq0 = pb["residue_and_atom_mask"], pb["residue_mask"], pb["residue_one_hot"]
    table, rows = rules.table(pb), rules.rows(pb)
    src = NoiseSource(SEED, 0)
    z = O.remove_mean(src.randn(NP, 3)[None], mask)
    seq_t = O.remove_mean(src.randn(NP, 21)[None], rm)
    seq_t = pb["residue_extra_mask"].unsqueeze(-1) * seq0 + pb["residue_inv_extra_mask"].unsqueeze(-1) * seq_t
    step_noise = [O.remove_mean(src.randn(NP, 3)[None], mask) for _ in range(T - 1)]
    for i in range(T):
        tt = T - 1 - i
        t = torch.full((1,), tt, dtype=torch.long)
        noise_pred, seq_pred = O.network_step(params, args, pb, z, seq_t, mask, t)
        w_noise = (1.0 - sch["alphas"][t]) / S[t]
        z = (1.0 / sch["sqrt_alphas"][t])[:, None, None] * (z - w_noise[:, None, None] * noise_pred)
        seq_t = torch.softmax(seq_pred, dim=-1) * 2 - 1
        if tt > 0:
            z = z + sch["sqrt_betas"][t][:, None, None] * step_noise[i]
        seq_t = SQ.restate_constrain(seq_t, seq_pred.contiguous(), table, rows)
    return 10.0 * z, rules.apply(rm.unsqueeze(-1) * seq_pred, table, rows), seq_t


@pytest.mark.parametrize("scope", ["design", "all"])
def test_ruled_loop_matches_the_oracle(setup, scope):
    """T = 4 steps within TRAJ_TOL.  Banned logits are BANNED on both sides and dominate a norm, so the logits are compared where they
    are allowed, and the banned places must coincide."""
    rules = some_rules(scope)
    with torch.inference_mode():
        want_pos, want_logits, want_seq = oracle_ruled_loop(setup, rules)
    loop = ruled(setup, rules)
    pos, logits = loop.result()
    pos, logits, seq_t = pos.cpu(), logits.cpu(), loop.seq_t.cpu()
    off = want_logits == BANNED
    assert int(off.sum()) > 0 and torch.equal(logits == BANNED, off) and torch.equal(seq_t == -1.0, want_seq == -1.0)
    e_pos, e_log, e_seq = rel_l2(pos, want_pos), rel_l2(logits[~off], want_logits[~off]), rel_l2(seq_t, want_seq)
    print(f"\nruled loop (scope {scope}) vs oracle: positions {e_pos:.2e}, allowed logits {e_log:.2e}, seq_t {e_seq:.2e}")
    assert e_pos < TRAJ_TOL and e_log < TRAJ_TOL and e_seq < TRAJ_TOL


def decoded_design(logits, inv):
    """the decoded classes of the design region of sample 0"""
    return logits[0].argmax(dim=-1).cpu()[inv[0] > 0.5]


def test_an_omitted_residue_never_reaches_the_network_nor_the_output(setup):
    """The run without rules decodes some residue type most often in its design region.  With that type omitted, seq_t is exactly -1 at
    its class on the ruled rows after EVERY step (eager stepping), the final logits hold BANNED there, and the decoded design region
    contains none of it.  Fails without the feature: the keyword does not exist."""
    inv, plain = setup["inv"], setup["plain"]
    before = decoded_design(plain["logits"], inv)
    cls = int(torch.bincount(before[before > 0], minlength=21).argmax())
    assert cls > 0 and int((before == cls).sum()) > 0          # the unconstrained run did contain it
    rules = SequenceRules.for_residues(NA, NR + 2, omit=SQ.ALPHABET[cls], unknown=True)
    model = setup["model"]
    model.use_hip_graph = False
    try:
        loop = ruled(setup, rules, run=False)
        rows = loop.rules[1] > 0.5
        assert torch.equal(rows.cpu(), inv > 0.5) and int(rows.sum()) > 0
        steps = 0
        while loop.steps_done < loop.T:
            loop.step()
            steps += 1
            now = loop.seq_t[rows]
            assert bool((now[:, cls] == -1.0).all()) and bool((now.max(dim=-1).values > -1.0).all()), steps
        assert steps == 4
    finally:
        model.use_hip_graph = True
    _, logits = loop.result()
    assert bool((logits[rows][:, cls] == BANNED).all()) and int((logits == BANNED).sum()) == int(rows.sum())
    after = decoded_design(logits, inv)
    assert int((after == cls).sum()) == 0 and bool(torch.isfinite(logits).all())
    other = ~rows & (loop.rm > 0.5)
    assert torch.equal(logits[other], (loop.rm.unsqueeze(-1) * loop.seq_pred)[other])      # other rows are returned as before


def test_allow_and_bias_at_one_position_are_honoured_in_every_sample(setup):
    inv = setup["inv"]
    first, second = [int(i) - NA for i in torch.nonzero(inv[0] > 0.5).flatten()[:2]]       # two residues of the design region
    rules = SequenceRules.for_residues(NA, NR + 2, allow={first: "AVLI"}, bias={(second, "W"): 20.0})
    allowed = {SQ.ALPHABET.index(ch) for ch in "AVLI"}
    for seed in (SEED, SEED + 1, SEED + 2):
        _, logits = ruled(setup, rules, seed=seed).result()
        tokens = logits[0].argmax(dim=-1).cpu()
        assert int(tokens[NA + first]) in allowed and int(tokens[NA + second]) == SQ.ALPHABET.index("W"), seed


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("scope", ["design", "all"])
def test_a_ruled_loop_is_set_up_and_run_without_host_synchronisation(setup, scope, on_device):
    """prepare_batch, the table (on the device already, or still on the host: one upload from pinned memory), the ruled rows, the first
    step, the capture of the step graph and its replays"""
    model = setup["model"]
    rules = some_rules(scope)
    ruled(setup, rules)                         # warm: library, allocators, the constant tables of the model
    if on_device:
        rules = rules.to(DEV)
    d = batch_to(clone_batch(setup["batch"]), DEV)
    sources = [NoiseSource(SEED, 0)]

    def work():
        loop = ReverseDiffusion(model, d, sources, redesign=setup["region"], sequence_rules=rules)
        loop.run()
        return loop
    loop = run_without_host_sync(work)
    assert loop.steps_done == 4 and loop.finite() and loop.graph is not None
    assert torch.equal(loop.rules[1].cpu(), setup["inv"] if scope == "design" else setup["batch"]["residue_mask"])


# ---------------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------------
def test_generate_samples_end_to_end(tmp_path):
    """Redesign the pocket within 8 Angstrom (14 residues of the 8 atoms + 40 residues fixture) with cysteine and methionine omitted
    and one position held to A / V / L / I; decode on the device at temperature 0.7 and count against the input."""
    from protein_redesign_amd.constants import RESIDUE_TYPES, make_args
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    from protein_redesign_amd.synthetic import deterministic_state_dict, synthetic_sample
    from protein_redesign_amd.weights import spec_tensors
    A, R = 8, 40
    args = make_args(single_dim=128, pair_dim=64, num_blocks=2, esm_dim=64, num_steps=4, mask_prob=0.3)
    model = ProteinReDiffModel(args)
    model.load_state_dict(deterministic_state_dict(spec_tensors(args), seed=1))
    model = model.to(DEV).eval()
    data = synthetic_sample(A, R, esm_dim=64, seed=0)

    def generate(out, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            return PL.generate_samples(model, data, num_samples=3, batch_size=2, seed=4, output_dir=out, redesign=Redesign.within(8.0), **kw)
    plain = generate(tmp_path / "plain")
    used = plain[4]
    pocket = np.nonzero(used[A:] > 0.5)[0]
    assert len(plain) == 5 and len(pocket) == 14
    rules = SequenceRules.for_residues(A, R, omit="CM", allow={int(pocket[0]): "AVLI"})
    out = generate(tmp_path / "a", sequence_rules=rules, decode=Decode(temperature=0.7, against="input"), assess="self")
    assert len(out) == 7 and isinstance(out[5], dict) and "ca_clashes" in out[5]            # the trailing dict comes last
    logits, proteins, seqs = out[1], out[2], out[6]
    assert sorted(seqs) == ["diversity", "entropy", "identity", "logp", "profile", "recovery", "recovery_design", "sequences", "tokens"]
    tokens = seqs["tokens"]
    assert tokens.shape == (3, R) and tokens.dtype == np.int32 and seqs["logp"].shape == seqs["entropy"].shape == (3, R)
    assert seqs["identity"].shape == (3, 3) and seqs["identity"].dtype == np.float64 and np.allclose(np.diag(seqs["identity"]), (tokens >= 0).mean(1))
    assert seqs["profile"].shape == (R, 21) and (seqs["profile"].sum(1) == 3).all() and 0.0 <= seqs["diversity"] <= 1.0
    assert seqs["recovery"].shape == seqs["recovery_design"].shape == (3,) and (seqs["logp"] <= 0).all() and (seqs["entropy"] >= -1e-6).all()
    off = [SQ.ALPHABET.index(ch) for ch in "XCM"]
    assert (logits[:, A:][:, pocket][:, :, off] == BANNED).all() and not np.isin(tokens[:, pocket], off).any()
    assert all(SQ.ALPHABET[c] in "AVLI" for c in tokens[:, pocket[0]])
    truth = np.asarray(data["residue_type"]) + 1
    assert np.allclose(seqs["recovery"], (tokens == truth[None]).mean(1))
    assert np.allclose(seqs["recovery_design"], (tokens[:, pocket] == truth[pocket][None]).mean(1))
    for k in range(3):                          # the proteins carry the tokens (class 0 is aatype -1)
        assert np.array_equal(proteins[k].aatype, tokens[k].astype(np.int64) - 1)
        assert seqs["sequences"][k] == "".join(("X" + "".join(RESIDUE_TYPES))[c] for c in tokens[k])
    assert sorted(os.listdir(tmp_path / "a")) == ["sample_ligand_pos.npy", "sample_protein.pdb", "sample_quality.npz", "sample_quality.txt",
                                                  "sample_redesign_mask.npy", "sample_sequences.fasta", "sample_sequences.npz"]
    fasta = (tmp_path / "a" / "sample_sequences.fasta").read_text().splitlines()
    assert len(fasta) == 6 and fasta[0].startswith(">sample_0 mean_logp=") and " recovery=" in fasta[0] and fasta[1::2] == seqs["sequences"]
    with np.load(tmp_path / "a" / "sample_sequences.npz") as z:
        assert np.array_equal(z["tokens"], tokens) and list(z["sequences"]) == seqs["sequences"]
    again = generate(tmp_path / "b", sequence_rules=rules, decode=Decode(temperature=0.7, against="input"), assess="self")
    assert again[6]["sequences"] == seqs["sequences"] and np.array_equal(again[1], logits) and np.array_equal(again[0], out[0])
    cold = generate(tmp_path / "c", sequence_rules=rules, decode=Decode())
    assert len(cold) == 6 and np.array_equal(cold[1], logits) and sorted(cold[5]) == sorted(set(seqs) - {"recovery", "recovery_design"})
    assert np.array_equal(cold[5]["tokens"], logits[:, A: A + R].argmax(-1))                # temperature 0: the host argmax
    bare = generate(tmp_path / "d", decode=Decode())                                        # no rules: the logits are the plain run's
    assert np.array_equal(bare[1], plain[1]) and np.array_equal(bare[5]["tokens"], plain[1][:, A: A + R].argmax(-1))
    assert all(np.array_equal(bare[2][k].aatype, plain[2][k].aatype) for k in range(3))
