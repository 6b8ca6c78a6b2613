"""CPU: pipeline.generate_samples over the COMBINATIONS of its post-processing options -- six alignment requests x four ``assess``
requests, ``redesign`` on every other call, every call with ``output_dir`` -- held exactly to a record of what it returned, wrote,
warned and asked of the side libraries, plus the type and full text of every host-side refusal these options can reach.

The model is sample_stubs._Stub (device = cpu) and the side libraries are replaced, as module attributes, by thin wrappers over the
float64 yardsticks of the GPU tests (align_ref, tmalign_ref, quality_ref).  The wrappers round what the yardsticks return to a decimal
grid (1e-6 on scores and transforms, 1e-3 Angstrom on moved coordinates) before the cast to float32: the record is compared on other
machines, whose LAPACK may differ from the recording one's in the last bits of an SVD, and this test is about what generate_samples
does with the numbers, not about the numbers.

The record is tests/golden/generate_samples_combinations.npz.  It is made by ``python tests/test_generate_samples_combinations_cpu.py
PATH`` on the commit whose behaviour is to be kept, never on the tree under test."""
import contextlib
import dataclasses
import hashlib
import itertools
import json
import os
import sys
import tempfile
import warnings
from unittest import mock

import numpy as np
import torch

import align_ref as AR
import quality_ref as QR
import tmalign_ref as TR
from conftest import ROOT
from protein_redesign_amd import align, quality, tmalign
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.masking import Redesign
from protein_redesign_amd.synthetic import synthetic_sample
from sample_stubs import _NoDevice, _Stub

GOLDEN = os.path.join(ROOT, "tests", "golden", "generate_samples_combinations.npz")
NA, NR = 5, 9


def _grid(a, decimals=6, dtype=np.float32):
    return torch.from_numpy(np.asarray(np.round(np.asarray(a, np.float64), decimals), dtype=dtype))


def _rows(mask):
    return np.nonzero(mask.numpy() > 0.5)[0]


def _shapes(*tensors):
    return [None if t is None else list(t.shape) for t in tensors]


def fakes(log):
    """{(module, attribute): stand-in}; every call is appended to ``log`` as [name, argument shapes, the options that matter]"""
    def superimpose(x, ref, mask, mirror=True, mode="tm"):
        log.append(["align.superimpose", _shapes(x, ref, mask), {"mirror": mirror, "mode": mode}])
        rows = _rows(mask)
        fits = [AR.superimpose(s.numpy()[rows], ref.numpy()[rows], mirror=mirror, mode=mode) for s in x]
        return align.Superposition(_grid([f["tm"] for f in fits]), _grid([f["rmsd"] for f in fits]), _grid([f["rotation"] for f in fits]),
                                   _grid([f["translation"] for f in fits]), torch.tensor([f["mirrored"] for f in fits], dtype=torch.int32))

    def diversity(x, mask, mirror=True):
        log.append(["align.diversity", _shapes(x, mask), {"mirror": mirror}])
        rows = _rows(mask)
        tms = [AR.superimpose(x[s].numpy()[rows], x[r].numpy()[rows], mirror=mirror)["tm"] for s in range(len(x)) for r in range(len(x)) if s != r]
        return _grid(np.mean(tms))

    def apply(pos, rotation, translation):
        log.append(["align.apply", _shapes(pos, rotation, translation), {}])
        p, rot, tr = (t.numpy().astype(np.float64) for t in (pos, rotation, translation))
        return _grid(tr[:, None] + np.einsum("snk,skj->snj", p, rot), 3)

    def tm_align(x, ref, mask, ref_mask, mirror=True):
        log.append(["tmalign.align", _shapes(x, ref, mask, ref_mask), {"mirror": mirror}])
        rx, ry = _rows(mask), _rows(ref_mask)
        fits = [TR.align(s.numpy()[rx], ref.numpy()[ry], mirror=mirror) for s in x]
        mapping = np.full((len(x), x.shape[1]), -1, np.int32)
        for k, f in enumerate(fits):
            on = f["mapping"] >= 0
            mapping[k, rx[on]] = ry[f["mapping"][on]]
        ints = lambda key: torch.tensor([f[key] for f in fits], dtype=torch.int32)
        return tmalign.StructuralAlignment(_grid([f["tm"] for f in fits]), _grid([f["rmsd"] for f in fits]), ints("n_aligned"),
                                           _grid([f["rotation"] for f in fits]), _grid([f["translation"] for f in fits]), ints("mirrored"),
                                           torch.from_numpy(mapping))

    def assess(pos, batch, ref=None, *, index=0, num_atoms=None, num_residues=None, ref_has_ligand=True):
        log.append(["quality.assess", _shapes(pos, ref), {"num_atoms": num_atoms, "num_residues": num_residues, "ref_has_ligand": bool(ref_has_ligand)}])
        N = pos.shape[1]
        out = QR.assess(pos.numpy(), num_atoms, num_residues, batch["residue_atom_mask"][index, :N, 1].numpy() > 0.5,
                        batch["bond_distance"][index, :N, :N].numpy(), batch["residue_index"][index, :N].numpy(),
                        batch["residue_chain_index"][index, :N].numpy(), None if ref is None else ref.numpy(), ref_has_ligand)
        return {k: torch.from_numpy(v.astype(np.int32) if v.dtype.kind == "i" else v.astype(np.float64)) for k, v in out.items()}

    return {(align, "superimpose"): superimpose, (align, "diversity"): diversity, (align, "apply"): apply, (tmalign, "align"): tm_align,
            (quality, "assess"): assess}


# ---- the description of a value: plain JSON, arrays by reference into one store -----------------------------------------------------

def describe(obj, store):
    if isinstance(obj, PL.Protein):
        return {"Protein": [[f.name, describe(getattr(obj, f.name), store)] for f in dataclasses.fields(obj)]}
    if torch.is_tensor(obj):
        return {"tensor": describe(obj.detach().cpu().numpy(), store)}
    if isinstance(obj, (np.ndarray, np.generic)):
        a = np.asarray(obj)
        key = "a" + hashlib.sha1(repr((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()[:16]
        store[key] = a
        return {"array": key, "type": type(obj).__name__, "dtype": a.dtype.str, "shape": list(a.shape)}
    if isinstance(obj, dict):
        return {"dict": [[k, describe(v, store)] for k, v in obj.items()]}
    if isinstance(obj, (list, tuple)):
        return {type(obj).__name__: [describe(v, store) for v in obj]}
    if isinstance(obj, float):
        return {"float": obj.hex()}
    assert obj is None or isinstance(obj, (int, str, bool)), type(obj)
    return obj


def describe_files(path, store):
    out = []
    for name in sorted(os.listdir(path)):
        full = os.path.join(path, name)
        if name.endswith(".npy"):
            out.append([name, describe(np.load(full), store)])
        elif name.endswith(".npz"):
            with np.load(full) as z:
                out.append([name, {"npz": [[member, describe(z[member], store)] for member in z.files]}])
        else:
            with open(full) as f:
                out.append([name, f.read()])
    return out


# ---- the calls -------------------------------------------------------------------------------------------------------------------------

def reference(n, seed, marked=None):
    """a Protein of n residues with seeded C-alpha coordinates, the first ``marked`` (default: all) of them marked"""
    p = PL.protein_from_sequence(("ACDEFGHIKLMNPQRSTVWY" * (n // 20 + 1))[:n])
    p.atom_pos[:, 1] = (np.random.default_rng(seed).normal(size=(n, 3)) * 10.0).astype(np.float32)
    p.atom_mask[:, 1] = 0.0
    p.atom_mask[: n if marked is None else marked, 1] = 1.0
    return p


def complex_data():
    return synthetic_sample(NA, NR, esm_dim=16, seed=8)


def alignment_requests():
    return [("none", {}), ("input", dict(align_to="input")), ("first", dict(align_to="first")),
            ("protein", dict(align_to=reference(NR, 31))),
            ("protein-of-another-length", dict(align_to=reference(12, 32, marked=10), correspondence="structure")),
            ("array-of-another-length", dict(align_to=reference(11, 33).atom_pos[:, 1].copy(), correspondence="structure"))]


def assess_requests():
    return [("none", {}), ("self", dict(assess="self")), ("input", dict(assess="input")), ("protein", dict(assess=reference(NR, 34)))]


def redesign_spec():
    mask = torch.zeros(NA + NR)
    mask[[1, NA, NA + 3, NA + NR - 1]] = 1          # a ligand atom (ignored) and three residues
    return Redesign.positions(mask)


def refusal_requests():
    """[(label, data, keywords)]: every host-side refusal these options reach, and pairs of them whose order is part of the behaviour"""
    full = complex_data()
    lig = {k: v for k, v in full.items() if k.startswith(("atom_", "bond_")) or k == "num_atoms"}
    bare = PL.protein_to_data(PL.protein_from_sequence("ACDEFGHIK"), **lig)         # a protein built from its sequence alone
    unmarked = dict(full, residue_atom_mask=torch.zeros(NR, 37))
    structure = dict(correspondence="structure")
    return [
        ("align_to unknown", full, dict(align_to="reference")),
        ("assess unknown", full, dict(assess="reference")),
        ("assess an array", full, dict(assess=np.zeros((NR, 3)))),
        ("correspondence unknown", full, dict(align_to=np.zeros((NR, 3)), correspondence="sequence")),
        ("align_to input, no coordinates", bare, dict(align_to="input")),
        ("align_to input, no C-alpha marked", unmarked, dict(align_to="input")),
        ("assess input, no coordinates", bare, dict(assess="input")),
        ("assess input, no C-alpha marked", unmarked, dict(assess="input")),
        ("align_to array of a wrong length", full, dict(align_to=np.zeros((8, 3)))),
        ("align_to Protein of a wrong length", full, dict(align_to=PL.protein_from_sequence("ACD"))),
        ("assess Protein of a wrong length", full, dict(assess=PL.protein_from_sequence("ACD"))),
        ("structure with input", full, dict(align_to="input", **structure)),
        ("structure with first", full, dict(align_to="first", **structure)),
        ("structure without a reference", full, dict(**structure)),
        ("structure, 4 C-alphas marked", full, dict(align_to=reference(12, 35, marked=4), **structure)),
        ("structure, 4 rows", full, dict(align_to=np.ones((4, 3)), **structure)),
        ("structure, [12,4] array", full, dict(align_to=np.ones((12, 4)), **structure)),
        ("structure, all-zero Protein", full, dict(align_to=PL.protein_from_sequence("ACDEFGHIK"), **structure)),
        ("structure, all-zero array", full, dict(align_to=np.zeros((12, 3)), **structure)),
        ("structure, 2049 reference rows", full, dict(align_to=np.ones((2049, 3)), **structure)),
        ("structure, 2049 sample rows", dict(full, num_residues=2044), dict(align_to=reference(12, 36), **structure)),
        ("pocket within, no coordinates", bare, dict(redesign=Redesign.within(8.0))),
        ("pocket nearest, no coordinates", bare, dict(redesign=Redesign.nearest(0.3))),
        ("pocket, no C-alpha marked", unmarked, dict(redesign=Redesign.within(8.0))),
        ("pocket, no ligand atom", dict(full, num_atoms=0), dict(redesign=Redesign.within(8.0))),
        # two refusals at once: which one speaks
        ("correspondence before assess", full, dict(align_to="first", correspondence="sequence", assess="reference")),
        ("structure reference before assess", full, dict(align_to=np.zeros((12, 3)), assess="reference", **structure)),
        ("align_to before assess", full, dict(align_to="reference", assess="reference")),
        ("assess before the pocket", bare, dict(assess="input", redesign=Redesign.within(8.0))),
        ("align_to before the pocket", bare, dict(align_to="input", redesign=Redesign.within(8.0))),
    ]


def record():
    """(description, {key: array}) of every call on the pipeline that is importable now"""
    store, calls, refusals = {}, [], []
    combos = itertools.product(enumerate(alignment_requests()), enumerate(assess_requests()))
    for (ia, (a_name, a_kw)), (iq, (q_name, q_kw)) in combos:
        kw = dict(a_kw, **q_kw, mirror=bool((4 * ia + iq) % 3))
        if (ia + iq) % 2:
            kw["redesign"] = redesign_spec()
        log = []
        with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings(record=True) as caught, contextlib.ExitStack() as stack:
            warnings.simplefilter("always")
            for (module, name), fn in fakes(log).items():
                stack.enter_context(mock.patch.object(module, name, fn))
            for module in (align, tmalign, quality):         # nothing but the stand-ins may be reached
                stack.enter_context(mock.patch.object(module, "lib", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a library was loaded"))))
            out = PL.generate_samples(_Stub(), complex_data(), num_samples=3, batch_size=2, seed=1, output_dir=tmp, **kw)
            calls.append({"label": f"align_to {a_name}, assess {q_name}, redesign {'redesign' in kw}, mirror {kw['mirror']}",
                          "length": len(out), "returned": describe(out, store), "files": describe_files(tmp, store),
                          "warnings": [[w.category.__name__, str(w.message)] for w in caught], "library calls": log})
    for label, data, kw in refusal_requests():
        try:
            PL.generate_samples(_NoDevice(), data, num_samples=2, **kw)
            refusals.append([label, None, None])
        except Exception as e:          # noqa: BLE001 -- the type is part of the record (an AssertionError: the model was touched)
            refusals.append([label, type(e).__name__, str(e)])
    return {"calls": calls, "refusals": refusals}, store


def test_generate_samples_is_what_the_record_says():
    got, store = record()
    with np.load(GOLDEN, allow_pickle=False) as z:
        want = json.loads(str(z["record"]))
        arrays = {k: z[k] for k in z.files if k != "record"}
    assert len(got["calls"]) == len(want["calls"]) == 24 and len(got["refusals"]) == len(want["refusals"]) == 30
    assert all(kind == "ValueError" for _, kind, _ in want["refusals"])
    for g, w in zip(got["refusals"], want["refusals"]):
        assert g == w, w[0]
    for g, w in zip(got["calls"], want["calls"]):
        for part in ("label", "length", "library calls", "warnings", "returned", "files"):
            assert g[part] == w[part], (w["label"], part)
    assert got == json.loads(json.dumps(got)) == want
    assert sorted(store) == sorted(arrays)
    for k, a in store.items():          # a key is a digest of dtype, shape and bytes: equal keys were equal arrays already
        assert a.dtype == arrays[k].dtype and a.shape == arrays[k].shape and a.tobytes() == arrays[k].tobytes(), k


if __name__ == "__main__":
    desc, arrays = record()
    np.savez_compressed(sys.argv[1], record=np.array(json.dumps(desc)), **arrays)
    print(f"{len(desc['calls'])} calls, {len(desc['refusals'])} refusals, {len(arrays)} arrays, {os.path.getsize(sys.argv[1])} bytes")
