"""GPU: libprd_align.so over the whole range include/prd_align.h promises -- up to PRD_ALIGN_MAX_N = 4096 positions, on masks that
make the compaction work, in rows much longer than the chain, on pairs where one seed decides, for many pairs, with junk where the
mask is 0, with strided x, and inside guarded buffers.  The properties and tolerances are those of tests/test_align.py (check_entry:
1e-4 on tm, 1e-4 Angstrom + 1e-5 relative on rmsd, 1e-5 on |R^T R - 1|, the determinant matches ``mirrored``); they hold because
every coordinate stays within 100 Angstrom of the origin (AR.chain, AR.planted, AR.core3_case).  The device result is compared with
the float64 yardstick tests/align_ref.py, with the float64 Kabsch fit (seed 0, round 0 of the search IS that fit) and with the planted
transform -- and, where the header's rules make the result independent of something (the row length N, the junk in masked-out rows,
the strides), with itself under that change, bit for bit.  Each test's docstring names the kernel defect it is there to catch."""
import functools
import time

import numpy as np
import pytest
import torch

import align_ref as AR
from protein_redesign_amd import align
from test_align import DEV, check_entry, embed, family, layout, run, strided_ref

pytestmark = pytest.mark.gpu
FIELDS = ("tm", "rmsd", "rotation", "translation", "mirrored")
MAX_N = 4096
ERR_WORKSPACE = -4


def f32(a):
    """float32-rounded, as float64"""
    return np.asarray(a).astype(np.float32).astype(np.float64)


def scattered(N, L, seed):
    """(mask [N], rows): L masked positions scattered at random over a row of N"""
    rows = np.sort(np.random.default_rng(seed).choice(N, size=L, replace=False))
    mask = np.zeros(N, np.float32)
    mask[rows] = 1.0
    return mask, rows


def all_ones(L):
    return L, np.ones(L, np.float32), np.arange(L)


def same_bits(a, b, what):
    for k in FIELDS:
        assert torch.equal(torch.from_numpy(a[k]), torch.from_numpy(b[k])), (what, k)


# ---- a. the upper range ------------------------------------------------------------------------------------------------------------
# N = 2048 is the last row length whose six LDS planes fit 48 KiB, N = 2049 the first that takes the attribute branch of the host
# code; L = 4033 is the first compacted length that uses bit 63 of the subset word; 4096 is the limit itself, with an all-ones mask.
UPPER = [2034, 2035, 3000, 4033, 4082, 4096]


def upper_layout(L):
    return all_ones(L) if L == MAX_N else layout(L)


@functools.lru_cache(maxsize=None)
def upper_case(L, frac):
    rng = np.random.default_rng(8000 + 10 * L + int(10 * frac))
    x, y, R0, t0, _ = AR.planted(rng, L, frac)
    return dict(x=f32(x), y=f32(y), R0=R0, t0=t0)


@functools.lru_cache(maxsize=None)
def upper_yardstick(L):
    """the unmirrored float64 search of the 0.35 case, once: a lower bound for the mirrored search of an unmirrored plant too"""
    c = upper_case(L, 0.35)
    t0 = time.perf_counter()
    ref = AR.superimpose(c["x"], c["y"], mirror=False)
    print(f"    yardstick at L={L}: {time.perf_counter() - t0:.1f} s of CPU")
    return ref


@pytest.mark.parametrize("frac", [1.0, 0.35])
@pytest.mark.parametrize("L", UPPER)
def test_upper_range(L, frac):
    """Catches: the branch that raises the dynamic-LDS limit not taken or not effective (N >= 2049: the launch fails or the planes
    beyond 48 KiB are not there), positions >= 4032 lost from the subsets (bit 63 of the 64-bit word, e.g. a 32-bit shift), LDS planes
    that overlap at large N, 8-wave workgroups that drop the seeds of waves 4 to 7 or of blockIdx.y > 0 (the 0.35 core is found only by
    short fragments, which sit at high seed indices), a finalize pass that reads the wrong one of up to 256 records."""
    N, mask, rows = upper_layout(L)
    assert N == (L if L == MAX_N else L + 14) and int(mask.sum()) == L
    c = upper_case(L, frac)
    rng = np.random.default_rng(11)
    xe, ye = embed(rng, c["x"][None], N, rows), embed(rng, c["y"][None], N, rows)
    got = run(xe, ye, mask, mirror=True)
    tm, _, mir = check_entry(got, (0, 0), c["x"], c["y"], f"L={L} N={N} core={frac}")
    Rk, tk = AR.kabsch(c["x"], c["y"])
    tm_k, tm_p = AR.tm_of(c["x"], c["y"], Rk, tk), AR.tm_of(c["x"], c["y"], c["R0"], c["t0"])
    print(f"    kabsch {tm_k:.6f}  planted {tm_p:.6f}")
    assert tm >= tm_k - 1e-4, (L, frac)
    assert tm >= tm_p - 1e-4, (L, frac)
    if frac == 1.0:
        assert mir == 0, (L, frac)
    else:
        ref = upper_yardstick(L)
        print(f"    yardstick {ref['tm']:.6f}")
        assert tm >= ref["tm"] - 1e-4, (L, frac)
    got = run(xe, ye, mask, mirror=False, mode="rmsd", single=True)
    _, rmsd, mir = check_entry(got, (0,), c["x"], c["y"], f"L={L} N={N} core={frac} rmsd mode")
    rmsd_k = AR.rmsd_of(c["x"], c["y"], Rk, tk)
    print(f"    kabsch rmsd {rmsd_k:.6f}")
    assert rmsd <= rmsd_k + 1e-4 and mir == 0, (L, frac)


# ---- b. masks that exercise the compaction -----------------------------------------------------------------------------------------
def hard_mask(kind, N):
    m = np.zeros(N, np.float32)
    rng = np.random.default_rng(8100 + N)
    if kind == "random":                        # (i) every thread of the compaction has a mixed count, 255 others follow it
        m[rng.random(N) < 0.5] = 1.0
    elif kind == "one_in_16":                   # (ii) every thread owns exactly one position, at an offset of its own
        m[16 * np.arange(N // 16) + rng.integers(0, 16, size=N // 16)] = 1.0
    elif kind == "last3":                       # (iii) thread 255 alone, at the very end of its range
        m[N - 3:] = 1.0
    elif kind == "second_half":                 # (iv) 128 empty threads, then 128 full ones
        m[N // 2:] = 1.0
    elif kind == "three_far":                   # (v) the first thread, one in the middle, the last one: one position each
        m[[0, N // 2 - 1, N - 1]] = 1.0
    return m


MASKS = [("random", 257), ("random", 1039), ("random", MAX_N), ("one_in_16", MAX_N), ("last3", MAX_N), ("second_half", MAX_N),
         ("three_far", MAX_N)]


@pytest.mark.parametrize("kind,N", MASKS)
def test_masks_that_make_the_compaction_work(kind, N):
    """Catches: a scan offset of the compaction off by one or taken from the wrong thread (a compacted row then holds another position's
    coordinates or workspace junk, and the tm the device reports is no longer the tm of the true masked rows under the returned
    transform), a thread range cut at N wrongly (N = 257: thread 16 owns one position; N = 1039: thread 64 owns 15), L counted
    wrongly (d0 and every seed depend on it), rows of x and of ref compacted differently."""
    mask = hard_mask(kind, N)
    rows = np.nonzero(mask)[0]
    L = len(rows)
    assert {"one_in_16": L == 256, "last3": L == 3 and rows[0] == N - 3, "second_half": L == 2048 and rows[0] == 2048,
            "three_far": list(rows) == [0, 2047, 4095], "random": 0.4 * N < L < 0.6 * N}[kind]
    rng = np.random.default_rng(8200 + N + L)
    x, y, R0, t0, _ = AR.planted(rng, L, 0.35 if L >= 5 else 1.0)
    x, y = f32(x), f32(y)
    xe, ye = embed(rng, x[None], N, rows), embed(rng, y[None], N, rows)
    got = run(xe, ye, mask, mirror=True)
    tm, _, _ = check_entry(got, (0, 0), x, y, f"{kind} N={N} L={L}")
    Rk, tk = AR.kabsch(x, y)
    assert tm >= AR.tm_of(x, y, Rk, tk) - 1e-4
    assert tm >= AR.tm_of(x, y, R0, t0) - 1e-4
    if L <= 300:
        ref = AR.superimpose(x, y, mirror=True)
        print(f"    yardstick {ref['tm']:.6f}")
        assert tm >= ref["tm"] - 1e-4
    got = run(xe, ye, mask, mirror=False, mode="rmsd", single=True)
    _, rmsd, mir = check_entry(got, (0,), x, y, f"{kind} N={N} L={L} rmsd mode")
    assert rmsd <= AR.rmsd_of(x, y, Rk, tk) + 1e-4 and mir == 0


def test_two_positions_in_a_full_length_row():
    """(vi) Catches: L counted over more than the mask (junk rows taken in), or the L < 3 exit of the search / finalize pass missed at
    the large grid of N = 4096 (records that were never written would be read)."""
    N = MAX_N
    x = torch.from_numpy(np.random.default_rng(8300).uniform(-50, 50, size=(2, N, 3)).astype(np.float32)).to(DEV)
    m = torch.zeros(N, device=DEV)
    m[[100, 4000]] = 1.0
    for out in (align.superimpose(x, x[:1] + 1.0, m), align.pairwise(x, m), align.superimpose(x, x[0], m, mode="rmsd")):
        torch.cuda.synchronize()
        assert not out.tm.any() and not out.rmsd.any() and not out.mirrored.any() and not out.translation.any()
        assert torch.equal(out.rotation, torch.eye(3, device=DEV).expand_as(out.rotation))


# ---- c. the result does not depend on the embedding ---------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [130, 20, 3])
def test_result_does_not_depend_on_the_row_it_is_embedded_in(L):
    """Each seed's arithmetic is local to a wave and fixed by L and the compacted values; the choice among seeds is the
    order-independent rule of the header's step 4.  So the row length N, the number of waves (4 up to N = 1024, else 8) and the number
    of workgroups per problem (from the largest seed count up to N) must not change a bit.  Catches: a compaction that depends on where
    the masked positions sit, seeds lost when they are spread over many nearly empty workgroups, an empty workgroup's -inf record taken
    by the finalize pass, a tie between seeds, waves or workgroups broken by position in the grid and not by seed index."""
    rng = np.random.default_rng(8400 + L)
    x, y, *_ = AR.planted(rng, L, 0.35 if L >= 5 else 1.0)
    x, y = f32(x), f32(y)
    places = [("layout", layout(L)), ("all ones", all_ones(L))]
    for N in (1100, 2049, MAX_N):
        mask, rows = scattered(N, L, 8500 + N + L)
        places.append((f"scattered in N={N}", (N, mask, rows)))
    assert places[0][1][0] == L + 14
    for kw in (dict(mirror=True), dict(mirror=False, mode="rmsd")):
        first = None
        for k, (name, (N, mask, rows)) in enumerate(places):
            junk = np.random.default_rng(8600 + k)
            got = run(embed(junk, x[None], N, rows), embed(junk, y[None], N, rows), mask, **kw)
            if first is None:
                first = got
                check_entry(got, (0, 0), x, y, f"L={L} {kw}")
            same_bits(got, first, (L, name, kw))


# ---- d. decisive seeds -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decisive():
    return AR.decisive_cases()


def test_decisive_seeds_are_not_skipped():
    """In every case kept here the float64 search loses at least 1e-3 of tm when its winning seed -- a fragment of 3 on a planted core of
    3 -- is left out, ten times the tolerance.  The same pair runs in three rows with 4, 8 and 8 waves per workgroup and different
    numbers of workgroups, so the same seed index lands in another workgroup and another wave each time.  Catches: seeds of
    blockIdx.y > 0 skipped, seeds of waves 4 to 7 skipped, a seed stride that leaves some out, the last level (fragments of 3, L <= 21)
    missing from the device's seed list, a workgroup's best record lost among its waves or among the records of the finalize pass."""
    cases = decisive()
    seeds = sorted({c["seed"] for c in cases})
    print(f"\n{len(cases)} decisive cases, winning seeds {seeds}")
    assert len(cases) >= 8 and len(seeds) >= 5            # checked on the CPU before any device call (also in test_align_cpu.py)
    for c in cases:
        L, x, y = c["L"], c["x"], c["y"]
        places = [layout(L)] + [(N,) + scattered(N, L, 8700 + N + 100 * L + c["p"]) for N in (1100, MAX_N)]
        for N, mask, rows in places:
            for mirror in (False, True):
                junk = np.random.default_rng(8800 + N)
                got = run(embed(junk, x[None], N, rows), embed(junk, y[None], N, rows), mask, mirror=mirror)
                tm, _, _ = check_entry(got, (0, 0), x, y, f"L={L} p={c['p']} seed {c['seed']} N={N} mirror={mirror}")
                print(f"    yardstick {c['tm']:.6f}, without seed {c['seed']}: {c['tm_without']:.6f}")
                assert tm >= c["tm"] - 1e-4, (L, c["p"], c["seed"], N, mirror)


# ---- e. many pairs -----------------------------------------------------------------------------------------------------------------
def both_searches(x, y):
    """the yardstick's two candidates: (tm unmirrored, tm mirrored)"""
    return AR.tm_search(x, y)[0], AR.tm_search(x @ AR.MIRROR, y)[0]


def check_pair(got, idx, x, y, what):
    tm, _, mir = check_entry(got, idx, x, y, what)
    tm0, tm1 = both_searches(x, y)
    Rk, tk = AR.kabsch(x, y)
    assert tm >= max(tm0, tm1) - 1e-4, what
    assert tm >= AR.tm_of(x, y, Rk, tk) - 1e-4, what
    return mir, tm0, tm1


def test_many_pairs_self_mode():
    """S = 33: 528 searched pairs, 1056 problems.  Catches: the pair decode of the self mode wrong beyond the first rows (a result
    written to another (s, r), which is then not honest for the structures of that entry, or two pairs sharing records), the transposed
    entry not the inverse, diagonal blocks of the finalize pass off by the pair count."""
    L, S = 22, 33
    N, mask, rows = layout(L)
    assert N == 36
    xs = family(L, S, 71)
    x = torch.from_numpy(embed(np.random.default_rng(12), xs, N, rows)).to(DEV)
    full = align.pairwise(x, torch.from_numpy(mask).to(DEV))
    torch.cuda.synchronize()
    got = {k: getattr(full, k).cpu().numpy() for k in FIELDS}
    assert got["tm"].shape == (S, S) and got["rotation"].shape == (S, S, 3, 3)
    assert np.array_equal(got["tm"], got["tm"].T) and np.array_equal(got["rmsd"], got["rmsd"].T) and np.array_equal(got["mirrored"], got["mirrored"].T)
    assert np.array_equal(np.diag(got["tm"]), np.ones(S, np.float32)) and not np.diag(got["rmsd"]).any() and not np.diag(got["mirrored"]).any()
    for s in range(S):
        assert np.array_equal(got["rotation"][s, s], np.eye(3)) and not got["translation"][s, s].any()
        for r in range(S):
            if s == r:
                continue
            if s < r:
                check_pair(got, (s, r), xs[s], xs[r], f"pair ({s},{r}) of {S}")
            else:
                check_entry(got, (s, r), xs[s], xs[r], f"pair ({s},{r}) of {S}")
            Rsr, tsr = got["rotation"][s, r].astype(np.float64), got["translation"][s, r].astype(np.float64)
            Rrs, trs = got["rotation"][r, s].astype(np.float64), got["translation"][r, s].astype(np.float64)
            assert np.abs(Rrs - Rsr.T).max() <= 1e-5 and np.abs(trs + tsr @ Rsr.T).max() <= 1e-5, (s, r)


def test_many_pairs_cross_mode():
    """17 x 9.  Catches: the row-major pair decode wrong for R that is no power of two, problems p = pair * 2 + mirror mixed up (the
    mirrored flag of a pair taken from its neighbour: the families are mirrored or not by a wide margin)."""
    L, S, R = 22, 17, 9
    N, mask, rows = layout(L)
    xs, ys = family(L, S, 72), family(L, R, 73)
    rng = np.random.default_rng(13)
    got = run(embed(rng, xs, N, rows), embed(rng, ys, N, rows), mask, mirror=True)
    assert got["tm"].shape == (S, R) and got["rotation"].shape == (S, R, 3, 3) and got["mirrored"].dtype == np.int32
    clear = 0
    for s in range(S):
        for r in range(R):
            mir, tm0, tm1 = check_pair(got, (s, r), xs[s], ys[r], f"pair ({s},{r}) of {S} x {R}")
            if abs(tm0 - tm1) > 0.05:
                clear += 1
                assert mir == int(tm1 > tm0), (s, r, tm0, tm1)
    print(f"{clear} of {S * R} pairs with a clear mirror decision")
    assert clear > 0                                    # (d0 is 0.57 at L = 22: few pairs of noisy variants are that far apart)


# ---- f. junk and strides -----------------------------------------------------------------------------------------------------------
def test_junk_in_masked_out_rows_and_strided_x():
    """Catches: a masked-out row read into a sum (NaN, inf or 1e30 then reach the result: 0 * NaN is NaN), the compaction addressing
    x with the wrong stride (row stride 15, structure stride 15 N: another atom's coordinates would be fitted), _structures copying a
    view it could have passed on."""
    N, L, S, R = 300, 130, 3, 2
    mask, rows = scattered(N, L, 8900)
    xs, ys = family(L, S, 74), family(L, R, 75)
    rng = np.random.default_rng(14)
    xe, ye = embed(rng, xs, N, rows), embed(rng, ys, N, rows)
    out = ~(mask > 0.5)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30], np.float32)
    xj, yj = xe.copy(), ye.copy()
    xj[:, out] = np.resize(bad, (S, int(out.sum()), 3))
    yj[:, out] = np.resize(bad[::-1], (R, int(out.sum()), 3))
    assert not np.isfinite(xj[:, out]).all() and np.array_equal(xj[:, rows], xe[:, rows]) and np.array_equal(yj[:, rows], ye[:, rows])
    m = torch.from_numpy(mask).to(DEV)
    for kw in (dict(mirror=True), dict(mirror=False, mode="rmsd")):
        plain = run(xe, ye, mask, **kw)
        for s in range(S):
            for r in range(R):
                check_entry(plain, (s, r), xs[s], ys[r], f"pair ({s},{r}) {kw}")
        same_bits(run(xj, yj, mask, **kw), plain, ("junk", kw))
        wide = torch.full((S, N, 5, 3), float("nan"))
        wide[:, :, 1] = torch.from_numpy(xe)
        view = wide.to(DEV)[:, :, 1]
        assert view.stride() == (N * 15, 15, 1)
        passed, ss, rs = align._structures(view, "x")
        assert passed.data_ptr() == view.data_ptr() and (ss, rs) == (N * 15, 15)        # no copy was made
        res = align.superimpose(view, strided_ref(ye), m, **kw)
        torch.cuda.synchronize()
        same_bits({k: getattr(res, k).cpu().numpy() for k in FIELDS}, plain, ("strided x", kw))


# ---- g. workspace and output bounds ------------------------------------------------------------------------------------------------
GUARD = 4096


def guarded_call(x, y, mask, S, R, N, pairs, mode, mirror, short=0, shift=0):
    """prd_align_superimpose with every output and the workspace in the middle of one 0xA5-filled buffer, 16-byte aligned, GUARD bytes
    apart; the workspace is handed over with exactly prd_align_workspace_bytes - ``short`` bytes, ``shift`` bytes off its alignment.
    Returns (return code, outputs as tensors, True if every byte outside the handed ranges is still 0xA5)."""
    L = align.lib()
    nbytes = L.prd_align_workspace_bytes(S, R, N, pairs, mode, mirror)
    assert nbytes > 0
    sizes = [("tm", S * R * 4), ("rmsd", S * R * 4), ("rotation", S * R * 36), ("translation", S * R * 12), ("mirrored", S * R * 4), ("ws", nbytes)]
    off, at = GUARD, {}
    for name, n in sizes:
        at[name] = off
        off = (off + n + GUARD + 15) // 16 * 16
    buf = torch.full((off,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    base = buf.data_ptr()
    torch.cuda.synchronize()
    code = L.prd_align_superimpose(base + at["tm"], base + at["rmsd"], base + at["rotation"], base + at["translation"], base + at["mirrored"],
                                   x.data_ptr(), x.stride(0), x.stride(1), None if y is None else y.data_ptr(),
                                   0 if y is None else y.stride(0), 0 if y is None else y.stride(1), mask.data_ptr(), S, R, N, pairs, mode,
                                   mirror, base + at["ws"] + shift, nbytes - short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    outside = np.ones(off, bool)
    if code == 0:
        for name, n in sizes:
            outside[at[name]: at[name] + n] = False
    untouched = bool((host[outside] == 0xA5).all())
    shapes = dict(tm=(S, R), rmsd=(S, R), rotation=(S, R, 3, 3), translation=(S, R, 3), mirrored=(S, R))
    outs = {k: host[at[k]: at[k] + dict(sizes)[k]].view(np.int32 if k == "mirrored" else np.float32).reshape(shapes[k]) for k in shapes}
    return code, outs, untouched


@pytest.mark.parametrize("S,R,N,pairs,mode,mirror", [(2, 2, MAX_N, "cross", "tm", 1), (3, 3, 5, "self", "tm", 1), (1, 1, 2049, "cross", "rmsd", 0)])
def test_nothing_is_written_outside_the_outputs_and_the_workspace(S, R, N, pairs, mode, mirror):
    """Catches: a record, a compacted plane or the header written past the workspace that prd_align_workspace_bytes asked for (the
    largest grid: 2 pairs x 2 mirrors x 128 workgroups at N = 4096; the self mode's S diagonal blocks; the smallest workspace of the RMSD
    mode), an output written past its [S][R] extent or before its start, a refused call that writes all the same."""
    rng = np.random.default_rng(9000 + N)
    L = N - 2 if N > 5 else N
    mask_np = np.ones(N, np.float32)
    mask_np[[1, N // 2][: N - L]] = 0.0
    rows = np.nonzero(mask_np)[0]
    xs, ys = family(L, S, 76), family(L, R, 77)
    x = torch.from_numpy(embed(rng, xs, N, rows)).to(DEV)
    y = None if pairs == "self" else torch.from_numpy(embed(rng, ys, N, rows)).to(DEV)
    m = torch.from_numpy(mask_np).to(DEV)
    P, M = dict(cross=align.PAIRS_CROSS, self=align.PAIRS_SELF)[pairs], align.MODES[mode]
    want = align.pairwise(x, m, mirror=bool(mirror), mode=mode) if y is None else align.superimpose(x, y, m, mirror=bool(mirror), mode=mode)
    torch.cuda.synchronize()
    code, outs, untouched = guarded_call(x, y, m, S, R, N, P, M, mirror)
    assert code == 0 and untouched
    for k in FIELDS:
        assert np.array_equal(outs[k], getattr(want, k).cpu().numpy()), k
    check_entry(outs, (0, R - 1), xs[0], (xs if y is None else ys)[R - 1], f"{S} x {R} x {N} {pairs} {mode}")
    for kw in (dict(short=1), dict(shift=4)):
        code, _, untouched = guarded_call(x, y, m, S, R, N, P, M, mirror, **kw)
        assert code == ERR_WORKSPACE and untouched, kw


# ---- h. capture at the large size --------------------------------------------------------------------------------------------------
def test_capture_and_replay_at_the_largest_size():
    """Catches: host work at N = 4096 that a capture does not take (raising the dynamic-LDS limit is such a candidate) or that
    synchronises, a replay that depends on state the eager call left behind.  One stream, no parallel branches."""
    N = MAX_N
    xs = family(N, 2, 78)
    assert np.abs(xs).max() < 100.0
    x = torch.from_numpy(xs.astype(np.float32)).to(DEV)
    m = torch.ones(N, device=DEV)
    ref = x[1]

    def work():
        return align.superimpose(x[:1], ref, m), align.pairwise_tm(x, m)
    eager = work()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = work()
    for _ in range(2):
        for t in (got[0].tm, got[0].rmsd, got[0].rotation, got[0].translation, got[1]):
            t.fill_(7.0)
        got[0].mirrored.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for k in FIELDS:
            assert torch.equal(getattr(got[0], k), getattr(eager[0], k)), k
        assert torch.equal(got[1], eager[1])
    out = {k: getattr(eager[0], k).cpu().numpy() for k in FIELDS}
    check_entry(out, (0,), xs[0], xs[1], "captured pair at N = 4096")
    assert float(eager[1][0, 1]) == float(eager[1][1, 0]) and float(eager[1][0, 0]) == 1.0
