"""Callers and data formats on either side of the hot path (SURVEY.md §8f "next" #2 and #3), host-side Python.

* batch assembly: ``collate_fn`` / ``RepeatDataset`` / ``PDBDataset`` with the contract of the reference's
  ProteinReDiff/data.py:80-185 (atoms first, residues after, ``residue_type + 1``, padded to the longest complex);
* output handling of ``generate.py``: sequence decoding (generate.py:75-91), CA placement (:65-74), multi-model PDB
  text (protein.py:124-174);
* ``generate_samples``: the ``Trainer.predict`` loop of generate.py:138-159 without Lightning.

rdkit / Biopython / TM-align are not needed: ligands are handled as coordinate arrays, proteins as plain arrays.
Nothing here is on the arithmetic path; the model call goes to the HIP path through ``ProteinReDiffModel``.
"""
from __future__ import annotations

import dataclasses
import os
import warnings
from pathlib import Path
from typing import Any, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from .constants import NUM_RESIDUE_ATOMS, RESIDUE_TYPES

UNKNOWN_RESIDUE_NAME = "UNK"          # PDB name written for aatype -1 ('X': undetermined / undecoded residue)
RESIDUE_NAMES = ["ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE",
                 "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP", "TYR", "VAL"]
RESIDUE_ATOMS = ["N", "CA", "C", "CB", "O", "CG", "CG1", "CG2", "OG", "OG1", "SG", "CD", "CD1", "CD2", "ND1", "ND2",
                 "OD1", "OD2", "SD", "CE", "CE1", "CE2", "CE3", "NE", "NE1", "NE2", "OE1", "OE2", "CH2", "NH1", "NH2",
                 "OH", "CZ", "CZ2", "CZ3", "NZ", "OXT"]
PDB_CHAIN_IDS = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"
assert len(RESIDUE_ATOMS) == NUM_RESIDUE_ATOMS


# ---------------------------------------------------------------------------------------------------
# batch assembly (data.py:80-185)
# ---------------------------------------------------------------------------------------------------

def collate_fn(data_list: Sequence[Mapping[str, Any]]) -> Dict[str, Any]:
    """Pad and stack per-complex dicts.  Key families decide the placement, as in data.py:80-142:
    ``atom_*`` -> rows [0, na); ``bond_*`` -> the [0, na)^2 corner; ``residue_*`` -> rows [na, na+nr)
    (and ``residue_type`` shifted by +1 so that 0 means pad / atom slot); ``*_mol`` -> python lists."""
    n_max = max(d["num_atoms"] + d["num_residues"] for d in data_list)
    out: Dict[str, Any] = {}
    for key, first in data_list[0].items():
        if key.startswith("atom_"):
            tail = (0, 0) * (first.dim() - 1)
            out[key] = torch.stack([F.pad(d[key], tail + (0, n_max - d["num_atoms"])) for d in data_list])
        elif key.startswith("bond_"):
            tail = (0, 0) * (first.dim() - 2)
            out[key] = torch.stack([F.pad(d[key], tail + (0, n_max - d["num_atoms"]) * 2) for d in data_list])
        elif key.startswith("residue_"):
            tail = (0, 0) * (first.dim() - 1)
            shift = 1 if key.endswith("_type") else 0
            out[key] = torch.stack([
                F.pad(d[key] + shift, tail + (d["num_atoms"], n_max - d["num_atoms"] - d["num_residues"]))
                for d in data_list])
        elif key.endswith("_mol"):
            out[key] = [d[key] for d in data_list]
        elif torch.is_tensor(first):
            out[key] = torch.stack([d[key] for d in data_list])
        elif isinstance(first, (int, float)):
            out[key] = torch.tensor([d[key] for d in data_list])
        else:
            out[key] = [d[key] for d in data_list]
    return out


class RepeatDataset(torch.utils.data.Dataset):
    """data.py:145-155: the same complex ``repeat`` times (one entry per requested sample)."""

    def __init__(self, data: Mapping[str, Any], repeat: int):
        self.data, self.repeat = data, repeat

    def __len__(self):
        return self.repeat

    def __getitem__(self, index: int):
        return self.data


class InferenceDataset(torch.utils.data.Dataset):
    """data.py:157-168: a LIST of featurised complexes, one entry per index (the ``predict_batch_*`` scripts' dataset);
    ``repeat`` is the length the caller declares, as in the reference."""

    def __init__(self, data: Sequence[Mapping[str, Any]], repeat: int):
        self.data, self.repeat = data, repeat

    def __len__(self):
        return self.repeat

    def __getitem__(self, index: int):
        return self.data[index]


class PDBDataset(torch.utils.data.Dataset):
    """data.py:170-185: ``root/<pdb_id>/{ligand,protein}_data.pt`` as written by preprocess_pdbbind.py:79-83."""

    def __init__(self, root_dir: Union[str, Path], pdb_ids: Sequence[str]):
        self.root_dir, self.pdb_ids = Path(root_dir), list(pdb_ids)

    def __len__(self):
        return len(self.pdb_ids)

    def __getitem__(self, index: int):
        pdb_id = self.pdb_ids[index]
        ligand = torch.load(self.root_dir / pdb_id / "ligand_data.pt", weights_only=False)
        protein = torch.load(self.root_dir / pdb_id / "protein_data.pt", weights_only=False)
        return {"pdb_id": pdb_id, **ligand, **protein}


class BucketBatchSampler(torch.utils.data.Sampler):
    """Batches of complexes of SIMILAR size for data-parallel training.

    The reference shuffles complexes freely (data.py:238-246: ``DataLoader(shuffle=True)``), so a batch is padded to its
    longest complex and, under DDP, every optimisation step lasts as long as the rank that drew the largest one (N ranges over
    100 .. 384 in PDBbind: the pair track costs O(N^3)).  This sampler keeps the reference's statistics -- every complex once per
    epoch, order reshuffled every epoch -- but draws each batch from one size bucket and hands the ranks of a step batches of
    the SAME bucket:

    * ``sizes[i]`` = num_atoms + num_residues of complex i; complexes are sorted into buckets ``bucket_width`` nodes wide;
    * per epoch (``set_epoch``) the members of every bucket are shuffled, cut into batches of ``batch_size``, the batches of a
      bucket grouped into steps of ``world_size`` batches (an incomplete last group is completed by wrapping around inside the
      bucket, as DistributedSampler pads), and the steps shuffled; rank r takes batch r of every step;
    * deterministic in ``(seed, epoch)``, identical on every rank, no communication.

    Use as ``DataLoader(dataset, batch_sampler=BucketBatchSampler(...), collate_fn=collate_fn)``."""

    def __init__(self, sizes: Sequence[int], batch_size: int, world_size: int = 1, rank: int = 0, bucket_width: int = 32,
                 seed: int = 0, shuffle: bool = True):
        if not 0 <= rank < world_size:
            raise ValueError(f"rank {rank} outside world of {world_size}")
        if batch_size < 1 or bucket_width < 1:
            raise ValueError("batch_size and bucket_width must be positive")
        self.sizes = [int(v) for v in sizes]
        self.batch_size, self.world_size, self.rank = batch_size, world_size, rank
        self.bucket_width, self.seed, self.shuffle, self.epoch = bucket_width, seed, shuffle, 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _steps(self) -> List[List[List[int]]]:
        g = torch.Generator().manual_seed((self.seed * 1_000_003 + self.epoch) & 0x7FFFFFFF)
        buckets: Dict[int, List[int]] = {}
        for i, n in enumerate(self.sizes):
            buckets.setdefault(n // self.bucket_width, []).append(i)
        steps: List[List[List[int]]] = []
        for key in sorted(buckets):
            members = buckets[key]
            if self.shuffle:
                members = [members[j] for j in torch.randperm(len(members), generator=g).tolist()]
            batches = [members[k:k + self.batch_size] for k in range(0, len(members), self.batch_size)]
            n0, k = len(batches), 0
            while len(batches) % self.world_size:                 # complete the last step by wrapping around inside the bucket:
                batches.append(batches[k % n0])                   # distinct batches as long as the bucket has them
                k += 1
            steps.extend(batches[k:k + self.world_size] for k in range(0, len(batches), self.world_size))
        if self.shuffle:
            steps = [steps[j] for j in torch.randperm(len(steps), generator=g).tolist()]
        return steps

    def __iter__(self):
        for step in self._steps():
            yield step[self.rank]

    def __len__(self) -> int:
        return len(self._steps())

    def padding_waste(self) -> Tuple[float, float]:
        """(this sampler, free shuffling with the same seed): fraction of the O(N^2) pair positions of an epoch that are
        padding or idle time of a rank waiting for the largest batch of its step."""
        def waste(steps):
            used = total = 0
            for step in steps:
                nmax = max(self.sizes[i] for bt in step for i in bt)
                for bt in step:
                    total += len(bt) * nmax * nmax
                    used += sum(self.sizes[i] ** 2 for i in bt)
            return 1.0 - used / max(total, 1)
        g = torch.Generator().manual_seed((self.seed * 1_000_003 + self.epoch) & 0x7FFFFFFF)
        order = torch.randperm(len(self.sizes), generator=g).tolist()
        free = [order[k:k + self.batch_size] for k in range(0, len(order), self.batch_size)]
        free_steps = [free[k:k + self.world_size] for k in range(0, len(free), self.world_size)]
        return waste(self._steps()), waste(free_steps)


class PDBDataModule:
    """data.py:206-259 without Lightning: the three id lists under ``data_dir`` and loaders over the preprocessed cache.
    ``bucket_width`` > 0 makes the TRAINING loader draw size-bucketed batches (BucketBatchSampler; sizes are read once from
    the cache); 0 reproduces the reference's free shuffling."""

    def __init__(self, data_dir: Union[str, Path] = "data", batch_size: int = 1, num_workers: int = 1, bucket_width: int = 32,
                 world_size: int = 1, rank: int = 0, seed: int = 0, group=None):
        self.data_dir = Path(data_dir)
        self.group = group                  # process group of the data-parallel ranks (None: the default group) -- _train_sizes
        self.cache_dir = self.data_dir / "PDB_processed_cache"
        self.batch_size, self.num_workers, self.bucket_width = batch_size, num_workers, bucket_width
        self.world_size, self.rank, self.seed = world_size, rank, seed
        self.train_sampler: Optional[BucketBatchSampler] = None

    def setup(self, stage: Optional[str] = None) -> None:
        def ids(name):
            with open(self.data_dir / name, "r") as f:
                return [line.strip() for line in f if line.strip()]
        self.train_pdb_ids, self.val_pdb_ids, self.test_pdb_ids = ids("PRD_train_pdb_ids"), ids("PRD_val_pdb_ids"), ids("PRD_test_pdb_ids")

    def train_dataloader(self):
        ds = PDBDataset(self.cache_dir, self.train_pdb_ids)
        if self.bucket_width <= 0:
            if self.world_size > 1:         # what Lightning injects under DDP (train.py:38): a disjoint shard per rank, reshuffled per epoch
                self.train_sampler = torch.utils.data.distributed.DistributedSampler(
                    ds, num_replicas=self.world_size, rank=self.rank, shuffle=True, seed=self.seed)
                return torch.utils.data.DataLoader(ds, batch_size=self.batch_size, sampler=self.train_sampler,
                                                   num_workers=self.num_workers, collate_fn=collate_fn)
            return torch.utils.data.DataLoader(ds, batch_size=self.batch_size, shuffle=True, num_workers=self.num_workers, collate_fn=collate_fn)
        self.train_sampler = BucketBatchSampler(self._train_sizes(ds), self.batch_size, self.world_size, self.rank, self.bucket_width, self.seed)
        return torch.utils.data.DataLoader(ds, batch_sampler=self.train_sampler, num_workers=self.num_workers, collate_fn=collate_fn)

    def set_epoch(self, epoch: int) -> None:
        """Reshuffle for a new epoch (both samplers are deterministic in (seed, epoch), identical on every rank)."""
        if self.train_sampler is not None:
            self.train_sampler.set_epoch(epoch)

    def _train_sizes(self, ds) -> List[int]:
        """num_atoms + num_residues of every training complex.  Read from ``<cache>/sizes_index.json`` where an entry's
        FINGERPRINT -- (mtime_ns, size) of the complex's two cache files -- still matches: a cache that was re-preprocessed
        (other cropping / featurisation) is re-scanned instead of driving the buckets with stale sizes.  Under an initialised
        process group rank 0 alone scans and writes the index and broadcasts its verdict, the other ranks then read the file (ranks that
        start together on a shared cache neither scan it N times nor overwrite each other's file; a scan that raises on rank 0 raises
        on every rank instead of leaving the others in a barrier).  Best effort on a read-only cache:
        it is scanned every time."""
        import json
        index_path = self.cache_dir / "sizes_index.json"

        def fingerprint(pid):
            fp = []
            for name in ("ligand_data.pt", "protein_data.pt"):
                try:
                    st = os.stat(self.cache_dir / pid / name)
                    fp += [int(st.st_mtime_ns), int(st.st_size)]
                except OSError:
                    fp += [0, 0]
            return fp

        def load():
            if not index_path.exists():
                return {}
            try:
                with open(index_path, "r") as f:
                    raw = json.load(f)
                if not isinstance(raw, dict) or raw.get("version") != 2:
                    return {}           # round-4 files had no fingerprints: rebuilt once
                return {str(k): (int(v[0]), [int(x) for x in v[1]]) for k, v in raw["entries"].items()}
            except (OSError, ValueError, KeyError, TypeError, IndexError):
                return {}

        def scan_and_store(index):
            stale = [i for i, pid in enumerate(ds.pdb_ids) if pid not in index or index[pid][1] != fingerprint(pid)]
            for i in stale:
                d = ds[i]
                index[ds.pdb_ids[i]] = (int(d["num_atoms"]) + int(d["num_residues"]), fingerprint(ds.pdb_ids[i]))
            if stale:
                try:
                    tmp = index_path.with_suffix(".json.tmp%d" % os.getpid())
                    with open(tmp, "w") as f:
                        json.dump({"version": 2, "entries": {k: [v[0], v[1]] for k, v in index.items()}}, f)
                    os.replace(tmp, index_path)
                except OSError:
                    pass
            return index

        distributed = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        if not distributed:
            index = scan_and_store(load())
        else:
            # Rank 0 scans; its verdict travels as an object broadcast (which is also the rendezvous: a bare barrier would leave the
            # other ranks waiting for ever when rank 0's scan raises -- a corrupt cache item -- and, with NCCL, needs a device already
            # set).  ``self.group`` (None: the default group) is the group the loaders of this module are sharded over.
            group = getattr(self, "group", None)
            rank = torch.distributed.get_rank(group)
            verdict = [None]
            index = None
            if rank == 0:
                try:
                    index = scan_and_store(load())
                    verdict = [("ok", None)]
                except Exception as exc:                # noqa: BLE001 -- re-raised on every rank below
                    verdict = [("error", f"{type(exc).__name__}: {exc}")]
            src = torch.distributed.get_global_rank(group, 0) if group is not None else 0
            torch.distributed.broadcast_object_list(verdict, src=src, group=group)
            if verdict[0][0] != "ok":
                raise RuntimeError(f"PDBDataModule: rank 0 failed while scanning the cache for complex sizes ({verdict[0][1]})")
            if rank != 0:
                index = load()
                if any(pid not in index or index[pid][1] != fingerprint(pid) for pid in ds.pdb_ids):
                    index = scan_and_store(index)       # rank 0 could not write (read-only cache): scan here too
        return [index[pid][0] for pid in ds.pdb_ids]

    def val_dataloader(self):
        return torch.utils.data.DataLoader(PDBDataset(self.cache_dir, self.val_pdb_ids), batch_size=self.batch_size,
                                           num_workers=self.num_workers, collate_fn=collate_fn)

    def test_dataloader(self):
        return torch.utils.data.DataLoader(PDBDataset(self.cache_dir, self.test_pdb_ids), batch_size=self.batch_size,
                                           num_workers=self.num_workers, collate_fn=collate_fn)


# ---------------------------------------------------------------------------------------------------
# proteins and output handling (protein.py:50-202, generate.py:65-91)
# ---------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Protein:
    chain_index: np.ndarray
    residue_index: np.ndarray
    aatype: np.ndarray
    atom_pos: np.ndarray
    atom_mask: np.ndarray


def protein_from_sequence(sequence: str) -> Protein:
    """protein.py:177-191: CA-only placeholder protein for a sequence ('X' -> -1)."""
    idx = {name: i for i, name in enumerate(RESIDUE_TYPES)}
    idx["X"] = -1
    aatype = np.array([idx[s] for s in sequence], dtype=np.int64)
    n = len(aatype)
    mask = np.zeros((n, NUM_RESIDUE_ATOMS), dtype=np.float32)
    mask[:, 1] = 1.0
    return Protein(np.zeros((n,), np.int64), np.arange(n, dtype=np.int64), aatype,
                   np.zeros((n, NUM_RESIDUE_ATOMS, 3), np.float32), mask)


def protein_to_data(prot: Protein, **extra) -> Dict[str, Any]:
    """data.py:59-77 without the rdkit CA molecule."""
    return {"num_residues": len(prot.aatype), "residue_type": torch.from_numpy(prot.aatype),
            "residue_mask": torch.ones(len(prot.aatype)), "residue_chain_index": torch.from_numpy(prot.chain_index),
            "residue_index": torch.from_numpy(prot.residue_index), "residue_atom_pos": torch.from_numpy(prot.atom_pos),
            "residue_atom_mask": torch.from_numpy(prot.atom_mask), **extra}


def protein_to_pdb_string(prot: Protein) -> str:
    """Fixed-column ATOM records, one per present atom (protein.py:124-156)."""
    lines, serial = [], 1
    for i in range(prot.chain_index.shape[0]):
        aa = int(prot.aatype[i])
        chain, resi = PDB_CHAIN_IDS[prot.chain_index[i]], prot.residue_index[i]
        resn = RESIDUE_NAMES[aa] if aa >= 0 else UNKNOWN_RESIDUE_NAME       # -1 must not wrap around to VAL
        for xyz, present, name in zip(prot.atom_pos[i], prot.atom_mask[i], RESIDUE_ATOMS):
            if present < 0.5:
                continue
            field = name if len(name) >= 4 else " " + name.ljust(3)
            lines.append(f"{'ATOM':<6}{serial:>5} {field}{'':>1}{resn:>3} {chain:>1}{resi:>4}{'':>1}   "
                         f"{xyz[0]:>8.3f}{xyz[1]:>8.3f}{xyz[2]:>8.3f}{1.0:>6.2f}{0.0:>6.2f}          {name[0]:>2}{'':>2}".ljust(80))
            serial += 1
    return "\n".join(lines) + "\n"


def proteins_to_pdb_file(proteins: Iterable[Protein], pdb_path: Union[str, Path]) -> None:
    """Multi-model PDB (protein.py:165-174)."""
    text = ""
    for model_id, prot in enumerate(proteins, 1):
        text += f"MODEL      {model_id:>3}".ljust(80) + "\n" + protein_to_pdb_string(prot) + "ENDMDL".ljust(80) + "\n"
    Path(pdb_path).write_text(text)


def predict_seq(logits) -> List[str]:
    """generate.py:75-80: argmax over the 21 classes with alphabet ["X"] + RESIDUE_TYPES."""
    tokens = torch.argmax(torch.softmax(torch.as_tensor(logits), dim=-1), dim=-1)
    alphabet = ["X"] + RESIDUE_TYPES
    return [alphabet[int(i)] for i in tokens]


def update_seq(protein: Protein, logits) -> Protein:
    """generate.py:82-91: decoded sequence with leading / trailing X stripped becomes the new aatype."""
    sequence = "".join(predict_seq(logits)).lstrip("X").rstrip("X")
    return dataclasses.replace(protein, aatype=np.array([RESIDUE_TYPES.index(s) for s in sequence], dtype=np.int64))


def update_pos(protein: Protein, num_ligand_atoms: int, pos: np.ndarray) -> Tuple[Protein, np.ndarray]:
    """generate.py:65-74: rows [na:] are the CA trace, rows [:na] the ligand atoms (returned as an array)."""
    atom_pos = np.zeros_like(protein.atom_pos)
    atom_pos[:, 1] = pos[num_ligand_atoms: num_ligand_atoms + atom_pos.shape[0]]
    atom_mask = np.zeros_like(protein.atom_mask)
    atom_mask[:, 1] = 1.0
    return dataclasses.replace(protein, atom_pos=atom_pos, atom_mask=atom_mask), np.asarray(pos[:num_ligand_atoms])


# ---------------------------------------------------------------------------------------------------
# generate.py:138-195 without Lightning / rdkit / TM-align
# ---------------------------------------------------------------------------------------------------

def _ca_trace_problem(data: Mapping[str, Any]) -> Optional[str]:
    """What keeps the featurised complex from serving as a C-alpha trace with coordinates, as the clause of a message; None if nothing."""
    ram, rap = torch.as_tensor(data["residue_atom_mask"]), torch.as_tensor(data["residue_atom_pos"])
    if ram.numel() == 0 or not bool((ram[:, 1] > 0.5).any()):
        return "no residue has its C-alpha marked in residue_atom_mask"
    if not bool((rap[:, 1] != 0).any()):
        return "the C-alpha coordinates are all zero (a protein built from its sequence alone?)"
    return None


def check_complex_structure(data: Mapping[str, Any]) -> None:
    """ValueError unless the featurised complex carries the coordinates a pocket is measured in: the C-alpha column of
    ``residue_atom_mask`` set, C-alpha coordinates that are not all zero, and at least one ligand atom with a position.  Host data
    only; ``protein_from_sequence`` inputs have none (their coordinates are zero)."""
    what = _ca_trace_problem(data)
    if what is None and (int(data.get("num_atoms", 0)) < 1 or "atom_pos" not in data or torch.as_tensor(data["atom_pos"]).shape[0] < 1):
        what = "there is no ligand atom with a position"
    if what is not None:
        raise ValueError("Redesign.within / Redesign.nearest measure a pocket and need the complex's coordinates: " + what
                         + "; use Redesign.positions for an input without a structure")


def _alignment_reference(data: Mapping[str, Any], align_to) -> Optional[np.ndarray]:
    """The [nr,3] C-alpha coordinates that ``generate_samples(align_to=...)`` superimposes on (None: the first sample), from host
    data alone; ValueError for a request that cannot be served."""
    nr = int(data["num_residues"])
    if isinstance(align_to, str):
        if align_to == "first":
            return None
        if align_to != "input":
            raise ValueError(f"align_to must be 'input', 'first', a Protein or an [{nr},3] array, got {align_to!r}")
        what = _ca_trace_problem(data)
        if what is not None:
            raise ValueError("align_to='input' superimposes the samples on the complex's own C-alpha coordinates: " + what
                             + "; use align_to='first' or pass a reference structure")
        return np.asarray(torch.as_tensor(data["residue_atom_pos"])[:, 1], dtype=np.float32)
    ref = align_to.atom_pos[:, 1] if isinstance(align_to, Protein) else align_to
    ref = np.asarray(ref, dtype=np.float32)
    if ref.shape != (nr, 3):
        raise ValueError(f"align_to: the reference has shape {ref.shape}, the complex has {nr} residues ([{nr},3] expected; chains of "
                         "another length need a sequence alignment, which is out of scope)")
    return ref


def _quality_reference(data: Mapping[str, Any], assess):
    """What ``generate_samples(assess=...)`` scores against, from host data alone: None for ``"self"``, else (the [na + nr, 3] reference
    over the rows of a sample, whether its ligand rows hold coordinates); ValueError for a request that cannot be served."""
    na, nr = int(data["num_atoms"]), int(data["num_residues"])
    if isinstance(assess, str):
        if assess == "self":
            return None
        if assess != "input":
            raise ValueError(f"assess must be None, 'self', 'input' or a Protein, got {assess!r}")
        what = _ca_trace_problem(data)
        if what is not None:
            raise ValueError("assess='input' scores the samples against the complex's own coordinates: " + what
                             + "; use assess='self' or pass a reference structure")
        ref = np.zeros((na + nr, 3), dtype=np.float32)
        ref[na:] = np.asarray(torch.as_tensor(data["residue_atom_pos"])[:, 1], dtype=np.float32)
        ligand = na >= 1 and "atom_pos" in data and tuple(torch.as_tensor(data["atom_pos"]).shape) == (na, 3)
        if ligand:
            ref[:na] = np.asarray(data["atom_pos"], dtype=np.float32)
        return ref, ligand
    if not isinstance(assess, Protein):
        raise ValueError(f"assess must be None, 'self', 'input' or a Protein, got {type(assess).__name__}")
    ca = np.asarray(assess.atom_pos, dtype=np.float32)[:, 1]
    if ca.shape != (nr, 3):
        raise ValueError(f"assess: the reference has shape {ca.shape}, the complex has {nr} residues ([{nr},3] expected; chains of "
                         "another length need a sequence alignment, which is out of scope)")
    ref = np.zeros((na + nr, 3), dtype=np.float32)
    ref[na:] = ca
    return ref, False


def _structural_reference(align_to):
    """The [m,3] C-alpha coordinates that ``generate_samples(align_to=..., correspondence="structure")`` aligns to by structure: the
    residues of a ``Protein`` whose C-alpha is marked in ``atom_mask[:,1]``, or the rows of an ``[m,3]`` array.  From host data alone;
    ValueError for a request that cannot be served."""
    from .tmalign import MAX_N
    if isinstance(align_to, str) or align_to is None:
        raise ValueError(f"correspondence='structure' needs a reference structure in align_to (a Protein or an [m,3] array), got {align_to!r}: "
                         "the correspondence to 'input' and to 'first' is known, use correspondence='index'")
    if isinstance(align_to, Protein):
        ca = np.asarray(align_to.atom_mask)[:, 1] > 0.5
        if int(ca.sum()) < 5:
            raise ValueError(f"align_to: the reference has {int(ca.sum())} residues with a C-alpha marked in atom_mask[:,1], "
                             "an alignment by structure needs at least 5")
        ref = np.asarray(align_to.atom_pos, dtype=np.float32)[:, 1]
    else:
        ref = np.asarray(align_to, dtype=np.float32)
        if ref.ndim != 2 or ref.shape[1] != 3 or ref.shape[0] < 5:
            raise ValueError(f"align_to: the reference has shape {ref.shape}, an [m,3] array of at least 5 C-alpha coordinates is expected")
        ca = np.ones(ref.shape[0], bool)
    if ref.shape[0] > MAX_N:
        raise ValueError(f"align_to: the reference has {ref.shape[0]} residues, an alignment by structure takes at most {MAX_N} (PRD_TMALIGN_MAX_N)")
    if not bool((ref[ca] != 0).any()):
        raise ValueError("align_to: the C-alpha coordinates of the reference are all zero (a protein built from its sequence alone?)")
    return ref, ca


def check_scaffold_structure(data: Mapping[str, Any], scaffold) -> None:
    """ValueError unless the featurised complex carries what ``scaffold`` (conditioning.Scaffold) holds rows to: C-alpha coordinates
    for any scaffold, ligand positions where the ligand is kept or the rows are chosen by their distance to it.  Host data only."""
    from .conditioning import Scaffold
    if not isinstance(scaffold, Scaffold):
        raise TypeError(f"scaffold must be a conditioning.Scaffold, got {type(scaffold).__name__}")
    what = _ca_trace_problem(data)
    if what is not None:
        raise ValueError("a scaffold keeps rows at, or starts from, the complex's own coordinates: " + what
                         + "; an input without a structure cannot be conditioned on")
    if scaffold.needs_ligand and (int(data.get("num_atoms", 0)) < 1 or "atom_pos" not in data
                                  or torch.as_tensor(data["atom_pos"]).shape[0] < 1):
        raise ValueError("Scaffold(ligand=True) and Scaffold.beyond need the ligand's coordinates: there is no ligand atom with a position")


def check_sequence_options(data: Mapping[str, Any], sequence_rules, decode) -> None:
    """The refusals of ``sequence_rules`` / ``decode`` that host data alone decides: the types, a bias table that does not fit the
    ``num_atoms + num_residues`` rows of the complex, and ``Decode(against="input")`` on an input whose ``residue_type`` is all unknown."""
    from .sequence import Decode, SequenceRules
    if sequence_rules is not None:
        if not isinstance(sequence_rules, SequenceRules):
            raise TypeError(f"sequence_rules must be a sequence.SequenceRules, got {type(sequence_rules).__name__}")
        n = int(data["num_atoms"]) + int(data["num_residues"])
        if sequence_rules.bias.shape[-2] != n:
            raise ValueError(f"sequence_rules: a bias table of {sequence_rules.bias.shape[-2]} rows does not fit the complex's {n} "
                             f"({int(data['num_atoms'])} ligand atoms + {int(data['num_residues'])} residues)")
    if decode is not None:
        if not isinstance(decode, Decode):
            raise TypeError(f"decode must be a sequence.Decode, got {type(decode).__name__}")
        if decode.against == "input" and not bool((torch.as_tensor(data["residue_type"]) >= 0).any()):
            raise ValueError("Decode(against='input') counts the recovery of the input's sequence: every residue_type of the input is "
                             "unknown (a protein without a sequence?)")


def _references(model, data, redesign, align_to, correspondence, assess, scaffold=None, sequence_rules=None, decode=None, handedness=None):
    """Stage (a) of generate_samples: every refusal that host data alone decides, in the order callers rely on, before ``model.device``
    is read; those of ``scaffold`` come after the references' and before the model's own design region is looked up.  Returns (structural reference or None, index-wise alignment reference or None, quality
    reference or None, redesign spec)."""
    if handedness is not None:                  # the type first, then what it may not be combined with
        from .chirality import Handedness
        if Handedness.of(handedness).fix and scaffold is not None:
            raise ValueError("handedness='fix' cannot be combined with a scaffold: the kept rows pin the frame and the hand of a sample, and a "
                             "reflection would move them off the input; use handedness='report' with a scaffold")
    if correspondence not in ("index", "structure"):
        raise ValueError(f"correspondence must be 'index' or 'structure', got {correspondence!r}")
    struct_ref = _structural_reference(align_to) if correspondence == "structure" else None
    if struct_ref is not None:
        from .tmalign import MAX_N
        rows = int(data["num_atoms"]) + int(data["num_residues"])
        if rows > MAX_N:                        # the sample side of the alignment: refused now, not after the samples are drawn
            raise ValueError(f"correspondence='structure': the complex has {rows} rows (ligand atoms + residues), an alignment by "
                             f"structure takes at most {MAX_N} (PRD_TMALIGN_MAX_N)")
    align_ref = _alignment_reference(data, align_to) if align_to is not None and struct_ref is None else None
    quality_ref = _quality_reference(data, assess) if assess is not None else None
    if scaffold is not None:                    # before the model is asked for its own design region: host data alone decides
        check_scaffold_structure(data, scaffold)
    if sequence_rules is not None or decode is not None:
        check_sequence_options(data, sequence_rules, decode)
    spec = redesign if redesign is not None else getattr(model, "redesign", None)
    if spec is not None and spec.needs_structure:
        check_complex_structure(data)
    return struct_ref, align_ref, quality_ref, spec


def _draw(model, data, num_samples, batch_size, seed, spec, device, keep_on_device, scaffold=None, sequence_rules=None, keep_logits=False,
          solver=None, guidance=None):
    """Stage (b): the sampling loop, with no synchronisation beyond its copies to the host; ``scaffold``, ``sequence_rules``,
    ``solver`` and ``guidance`` reach ``model.sample`` only when given.  Returns (positions per batch -- left on the
    device if ``keep_on_device``, for the stages that score them there --, logits per batch on the host -- on the device if
    ``keep_logits``, for the decoding there --, the first prepared batch, the keyed noise source of every sample as sample() left it)."""
    from .synthetic import NoiseSource, batch_to
    positions, logits, first_batch, used = [], [], None, []
    cond = {} if scaffold is None else {"scaffold": scaffold}
    if sequence_rules is not None:
        cond["sequence_rules"] = sequence_rules
    if solver is not None:
        cond["solver"] = solver
    if guidance is not None:
        cond["guidance"] = guidance
    for start in range(0, num_samples, batch_size):
        idx = list(range(start, min(start + batch_size, num_samples)))
        batch = collate_fn([data] * len(idx))
        batch = batch_to({k: v for k, v in batch.items() if torch.is_tensor(v)}, device)
        sources = [NoiseSource(seed, k) for k in idx]
        pos, lg = model.sample(batch, sources=sources, redesign=spec, **cond)
        if first_batch is None:
            first_batch = batch                 # sample() prepared it in place: it carries the mask that was used
        positions.append(pos if keep_on_device else pos.cpu())
        logits.append(lg if keep_logits else lg.cpu())
        used += sources
    return positions, logits, first_batch, used


def _assess(pos, first_batch, quality_ref, na, nr):
    """Stage (c): the quality scores of the samples as model.sample returned them (distances do not see align_to's transform), as numpy"""
    from . import quality as QL
    ref = torch.from_numpy(quality_ref[0]).to(pos.device) if quality_ref is not None else None
    scores = QL.assess(pos.float()[:, : na + nr], first_batch, ref, num_atoms=na, num_residues=nr,
                       ref_has_ligand=quality_ref is not None and quality_ref[1])
    scores["pocket"] = scores["pocket"][:, na:]
    return {k: v.cpu().numpy() for k, v in scores.items()}


def _superpose(pos, data, struct_ref, align_ref, mirror, na, nr):
    """Stage (d): fit every sample to the reference (by structure, index-wise, or to the first sample), score the samples among themselves
    and move whole rows into the reference's frame.  Returns (moved positions, the alignment dict), both still on the device."""
    from . import align as AL
    pos, device = pos.float(), pos.device
    n = pos.shape[1]
    ca_mask = torch.zeros(n)
    ca_mask[na: na + nr] = (torch.as_tensor(data["residue_atom_mask"])[:, 1] > 0.5).float()
    ca_mask = ca_mask.to(device)
    if struct_ref is not None:
        from . import tmalign as TM
        fit = TM.align(pos, torch.from_numpy(struct_ref[0]).to(device), ca_mask, torch.from_numpy(struct_ref[1].astype(np.float32)).to(device),
                       mirror=mirror)
    else:
        if align_ref is None:
            warnings.warn("Using the first sample as a reference. The resulting structures may be mirror images.", UserWarning)
            ref = pos[0].clone()
        else:
            ref = torch.zeros(n, 3)
            ref[na: na + nr] = torch.from_numpy(align_ref)
            ref = ref.to(device)
        fit = AL.superimpose(pos, ref, ca_mask, mirror=mirror)
    div = AL.diversity(pos, ca_mask, mirror=mirror)
    moved = AL.apply(pos, fit.rotation, fit.translation)
    alignment = {"tmscore": fit.tm, "rmsd": fit.rmsd, "mirrored": fit.mirrored, "rotation": fit.rotation, "translation": fit.translation,
                 "diversity": div}
    if struct_ref is not None:
        alignment["n_aligned"] = fit.n_aligned
        alignment["mapping"] = fit.mapping[:, na: na + nr]          # rows of the reference ARE its residue indices
    return moved, alignment


def _decode_on_device(data, logits, sources, decode, ruled, design_mask, na, nr):
    """Stage (e'), ``decode=``: one prd_sequence_decode over all samples (Gumbel noise of each sample's own keyed source when the
    temperature is not 0), one prd_sequence_census over the residue rows, then the one copy to the host.  ``logits`` [S,N,21] on the
    device, ``ruled``: sequence rules were applied to them (their banned entries hold BANNED).  Returns the dict of numpy arrays."""
    from . import sequence as SQ
    S, N, _ = logits.shape
    device = logits.device
    logits = logits.float().contiguous()
    residues = torch.zeros(N)
    residues[na: na + nr] = 1.0
    residues = residues.to(device)
    rows = residues.unsqueeze(0).expand(S, N).contiguous()
    # the bans of the rules, read off the returned logits: one elementwise expression, no bias (it is in the logits already)
    bans = torch.where(logits <= SQ.BANNED, torch.full_like(logits, SQ.BANNED), torch.zeros_like(logits)) if ruled else None
    gumbel = None
    if decode.temperature > 0.0:
        gumbel = torch.stack([s.gumbel(N, SQ.N_CLS) for s in sources]).to(device)
    tokens, logp, entropy = SQ.decode(logits, rows, bias=bans, gumbel=gumbel, temperature=decode.temperature)
    ref = None
    if decode.against == "input":
        ref = torch.full((N,), -1, dtype=torch.int32)
        ref[na: na + nr] = torch.as_tensor(data["residue_type"]).to(torch.int32) + 1        # class 0 is X
        ref[ref == 0] = -1                                                                  # an unknown residue recovers nothing
        ref = ref.to(device)
    identity, recovery, profile = SQ.census(tokens, residues, ref)
    tokens, logp, entropy = (t[:, na: na + nr].cpu().numpy() for t in (tokens, logp, entropy))
    ident = identity.cpu().numpy().astype(np.float64) / nr
    out = {"tokens": tokens, "sequences": ["".join(SQ.ALPHABET[c] if c >= 0 else "X" for c in row) for row in tokens], "logp": logp,
           "entropy": entropy, "identity": ident,
           "diversity": float(1.0 - (ident.sum() - np.trace(ident)) / (S * (S - 1))) if S > 1 else float("nan"),
           "profile": profile[na: na + nr].cpu().numpy()}
    if ref is not None:
        known = ref[na: na + nr].cpu().numpy() >= 0
        design = known & (design_mask[na: na + nr] > 0.5) if design_mask is not None else known
        same = (tokens == (ref[na: na + nr].cpu().numpy())[None]) & known[None]
        out["recovery"] = recovery.cpu().numpy().astype(np.float64) / max(int(known.sum()), 1)
        out["recovery_design"] = (same & design[None]).sum(axis=1).astype(np.float64) / max(int(design.sum()), 1)
    return out


def _decode(data, positions, logits, na, nr, tokens=None):
    """Stage (e): (proteins, ligand positions) of the samples, every protein with its decoded sequence -- the host argmax of the logits,
    or ``tokens`` [S,nr] decoded on the device --; warns of undetermined residues"""
    template = Protein(np.asarray(data["residue_chain_index"]), np.asarray(data["residue_index"]),
                       np.asarray(data["residue_type"]), np.asarray(data["residue_atom_pos"], dtype=np.float32),
                       np.asarray(data["residue_atom_mask"], dtype=np.float32))
    proteins, ligands = [], []
    for k, (pos, lg) in enumerate(zip(positions, logits)):
        prot, lig = update_pos(template, na, pos)
        seq = predict_seq(lg[na: na + nr]) if tokens is None else [("X" + "".join(RESIDUE_TYPES))[max(int(c), 0)] for c in tokens[k]]
        prot = dataclasses.replace(prot, aatype=np.array([RESIDUE_TYPES.index(s) if s != "X" else -1 for s in seq], dtype=np.int64))
        proteins.append(prot)
        ligands.append(lig)
    undetermined = [k for k, p in enumerate(proteins) if (p.aatype < 0).any()]
    if undetermined:
        warnings.warn(f"samples {undetermined} decode to 'X' at some residues; those are written as UNK", UserWarning)
    return proteins, ligands


def _guidance_report(guidance, data, pos, first_batch, na, nr):
    """Stage (c'), ``guidance=``: the spec's terms, the clash and restraint energy [S,2] of the samples as model.sample returned them
    (``guidance.energy``: one launch, distances only) and, when the input has coordinates, the same energy of the input structure --
    what an unguided evaluation of it gives.  Returns the dict of numpy values."""
    from . import guidance as GD
    out = guidance.describe()
    one = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in first_batch.items()}     # every sample is the same complex
    out["energy"] = GD.energy(pos.float(), one, guidance).cpu().numpy()
    if _ca_trace_problem(data) is None and (na == 0 or "atom_pos" in data):
        given = torch.zeros(1, pos.shape[1], 3)
        given[0, na: na + nr] = torch.as_tensor(data["residue_atom_pos"], dtype=torch.float32)[:, 1]
        if na > 0:
            given[0, :na] = torch.as_tensor(data["atom_pos"], dtype=torch.float32)
        out["input_energy"] = GD.energy(given.to(pos.device), one, guidance).cpu().numpy()[0]
    return out


def _handedness_report(spec, data, pos, first_batch, na, nr):
    """Stage (b'), ``handedness=``: one census over all samples as model.sample returned them (``chirality.census``: one launch), under
    ``spec.fix`` the reflection of the samples judged mirrored, in place and with the verdict still on the device, and, when the input
    has C-alpha coordinates, the same census of the input structure.  The ligand's centres are compared with the input's own when the
    input has ligand coordinates.  Returns the dict of numpy values; ``pos`` [S,N,3] fp32 is changed in place under ``fix``."""
    from . import chirality as CH
    device, n = pos.device, pos.shape[1]
    one = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in first_batch.items()}     # every sample is the same complex
    mask, link = (t[:n].contiguous() for t in CH.trace_links(one, 0, na, nr))
    centres, atoms = CH.ligand_centres(collate_fn([{k: v for k, v in data.items() if k in ("num_atoms", "num_residues", "atom_feats", "bond_distance")}]))
    has_ligand = na > 0 and "atom_pos" in data and bool((torch.as_tensor(data["atom_pos"]) != 0).any())
    ref = None
    if has_ligand and len(centres):
        centres, ref = CH.centre_reference(torch.as_tensor(data["atom_pos"], dtype=torch.float32), centres, spec.vmin)
        atoms = centres[:, 0].to(torch.int64)
    listed = CH.upload(centres, device) if len(centres) else None
    ref = ref.to(device) if ref is not None and len(centres) else None
    got = CH.census(pos, mask, link, centres=listed, centre_ref=ref, **spec.thresholds())
    flipped = (got.verdict < 0) if spec.fix else torch.zeros_like(got.verdict, dtype=torch.bool)
    if spec.fix:
        CH.reflect(pos, flipped)
    out = {"verdict": got.verdict, "basis": got.basis, "flipped": flipped, "helix_fraction": got.helix_fraction,
           "extended_fraction": got.extended_fraction, "tau": got.tau[:, na: na + nr], "classes": got.classes[:, na: na + nr],
           "ligand_volume": got.volume}
    for k, name in enumerate(CH.COUNT_COLUMNS):
        out[CH.RESULT_NAMES.get(name, name)] = got.counts[:, k]
    if _ca_trace_problem(data) is None:
        given = torch.zeros(1, n, 3)
        given[0, na: na + nr] = torch.as_tensor(data["residue_atom_pos"], dtype=torch.float32)[:, 1]
        if has_ligand:
            given[0, :na] = torch.as_tensor(data["atom_pos"], dtype=torch.float32)
        own = CH.census(given.to(device), mask, link, centres=listed if has_ligand else None, centre_ref=ref if has_ligand else None,
                        **spec.thresholds())
        out.update(input_verdict=own.verdict[0], input_basis=own.basis[0], input_counts=own.counts[0])
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["ligand_centres"] = atoms.numpy()
    return out


def _backbone_atoms(spec, pos, first_batch, na, nr):
    """Stage (d'), ``backbone=``: N, C, O and CB of every residue of every sample from the C-alpha trace (``backbone.build``: one launch),
    on the samples in their final frame and on their final hand -- after the handedness fix and after ``align_to``.  Returns the dict of
    numpy values: the residue rows of the launch's outputs, then the spec's table and geometry -- and, for the stage that consumes the
    atoms on the device (``secondary=``), the launch's own tensors with the mask and the links it took."""
    from . import backbone as BB
    from . import chirality as CH
    n = pos.shape[1]
    one = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in first_batch.items()}     # every sample is the same complex
    mask, link = (t[:n].contiguous() for t in CH.trace_links(one, 0, na, nr))
    got = BB.build(pos.float(), mask, link, BB.upload(spec, pos.device))
    flags = got.flags[:, na: na + nr]
    out = {"atoms": got.atoms[:, na: na + nr], "built": flags,
           "unbuilt_residues": (~(flags[:, :, 0] & flags[:, :, 2] & flags[:, :, 4])).sum(1)}    # a residue without its N, its C or its O
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out.update(spec.describe())
    return out, (got, mask, link)


def _secondary_structure(spec, data, on_device, na, nr):
    """Stage (d''), ``secondary=``: the hydrogen bonds and the DSSP classes of every sample (``dssp.assign``: three launches) on the
    device tensors of ``backbone.build`` as the stage before left them, their census, and -- when the input has N, CA, C and O -- the
    same two calls on the input's own atoms and the share of residues a sample classes as the input does.  Returns the dict of numpy
    values, partner rows re-based to residue indices."""
    from . import dssp as DS
    got, mask, link = on_device
    device, n = got.atoms.device, got.atoms.shape[1]
    found = DS.assign(got.atoms, got.built, link, None, spec)          # no donor mask: proline donates
    counted = DS.census(found, mask, spec)
    rebase = lambda t: torch.where(t >= 0, t - na, t)[:, na: na + nr]          # noqa: E731
    out = {"classes": found.classes[:, na: na + nr], "partner": rebase(found.partner), "energy": found.energy[:, na: na + nr],
           "bridge": rebase(found.bridge), **counted}
    ram, rap = torch.as_tensor(data["residue_atom_mask"]), torch.as_tensor(data["residue_atom_pos"], dtype=torch.float32)
    has = ram[:, :5] > 0.5
    whole = has[:, 0] & has[:, 1] & has[:, 2] & has[:, 4]         # marked, and with coordinates (an input from its sequence alone has none)
    if _ca_trace_problem(data) is None and bool(whole.any()) and bool((rap[whole][:, [0, 2, 4]] != 0).any()):
        atoms, built = torch.zeros(1, n, 5, 3), torch.zeros(1, n, dtype=torch.int32)
        atoms[0, na: na + nr] = torch.where(has[:, :, None], rap[:, :5], torch.zeros(()))
        built[0, na: na + nr] = (has.to(torch.int32) << torch.arange(5, dtype=torch.int32)).sum(1).to(torch.int32)
        built = built.to(device)
        own = DS.assign(atoms.to(device), built, link, None, spec)
        both = ((got.built & 2) != 0) & ((built & 2) != 0) & (mask > 0.5)       # [S,n]: the residues classed in both
        total = both.sum(1).to(torch.float32)
        share = lambda a, b: torch.where(total > 0, ((a == b) & both).sum(1) / total.clamp(min=1), torch.full_like(total, float("nan")))   # noqa: E731
        out.update(input_classes=own.classes[0, na: na + nr], q8=share(found.classes, own.classes),
                   q3=share(DS.three_state(found.classes), DS.three_state(own.classes)))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["strings"] = DS.strings(out["classes"])
    return out


def _accessibility(spec, data, on_device, pos, first_batch, na, nr):
    """Stage (d'''), ``accessibility=``: the Shrake-Rupley counts of the built atoms and the ligand rows of every sample
    (``sasa.measure``: two launches) on the device tensors of ``backbone.build`` as the stage before left them and on ``pos[:, :na]``,
    and -- when the input has N, CA, C and O -- the same call on the input's own atoms and the share of residues a sample calls
    buried or exposed as the input does.  Returns the dict of numpy values."""
    from . import sasa as SA
    got, mask, _ = on_device
    device = got.atoms.device
    elements = first_batch["atom_feats"][0, :na, 0]
    rows = mask[na: na + nr]
    up = SA.upload(spec, device)
    found = SA.measure(got.atoms[:, na: na + nr], got.built[:, na: na + nr], pos[:, :na].float(), elements, rows, up)
    out = dict(found)
    ram, rap = torch.as_tensor(data["residue_atom_mask"]), torch.as_tensor(data["residue_atom_pos"], dtype=torch.float32)
    has = ram[:, :5] > 0.5
    whole = has[:, 0] & has[:, 1] & has[:, 2] & has[:, 4]         # marked, and with coordinates (an input from its sequence alone has none)
    if _ca_trace_problem(data) is None and bool(whole.any()) and bool((rap[whole][:, [0, 2, 4]] != 0).any()):
        atoms = torch.where(has[:, :, None], rap[:, :5], torch.zeros(()))[None].contiguous()
        built = (has.to(torch.int32) << torch.arange(5, dtype=torch.int32)).sum(1).to(torch.int32)[None]
        has_ligand = na > 0 and "atom_pos" in data and bool((torch.as_tensor(data["atom_pos"]) != 0).any())
        ligand = torch.as_tensor(data["atom_pos"], dtype=torch.float32)[None, :na] if has_ligand else torch.zeros(1, 0, 3)
        own = SA.measure(atoms.to(device), built.to(device), ligand.to(device), elements[: ligand.shape[1]], rows, up)
        both = found["complete"] & own["complete"]                # [S,nr]: the residues whole in both
        total = both.sum(1).to(torch.float64)
        agree = ((found["buried"] == own["buried"]) & both).sum(1) / total.clamp(min=1)
        out.update(input_relative=own["relative"][0], burial_agreement=torch.where(total > 0, agree, torch.full_like(total, float("nan"))))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out.update(spec.describe())
    return out


def _with_backbone(proteins, built):
    """the proteins with the built atoms in ``atom_pos`` / ``atom_mask`` (atom37 indices 0 .. 4: N, CA, C, CB, O); CA stays what
    ``update_pos`` made it, and CB is left out of a residue decoded as G or left undetermined"""
    no_cb = {RESIDUE_TYPES.index("G"), -1}
    out = []
    for k, prot in enumerate(proteins):
        atom_pos, atom_mask = prot.atom_pos.copy(), prot.atom_mask.copy()
        have = built["built"][k].copy()
        have[:, 3] &= ~np.isin(prot.aatype, list(no_cb))
        for a in (0, 2, 3, 4):
            atom_pos[:, a] = np.where(have[:, a, None], built["atoms"][k][:, a], 0.0)
            atom_mask[:, a] = have[:, a]
        out.append(dataclasses.replace(prot, atom_pos=atom_pos, atom_mask=atom_mask))
    return out


def _write(output_dir, proteins, ligands, used_mask, alignment, quality, scaffold=None, sequences=None, guided=None, handed=None, built=None,
           secondary=None, accessibility=None):
    """Stage (f): the files of ``output_dir``"""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    proteins_to_pdb_file(proteins, out / "sample_protein.pdb")
    np.save(out / "sample_ligand_pos.npy", np.stack(ligands))
    if used_mask is not None:
        np.save(out / "sample_redesign_mask.npy", used_mask)
    if alignment is not None:
        with open(out / "sample_tmscores.txt", "w") as f:
            for tmscore in alignment["tmscore"]:
                f.write(str(float(tmscore)) + "\n")
        np.savez(out / "sample_alignment.npz", **alignment)
    if quality is not None:
        from .quality import SCALAR_COLUMNS
        cols = [c for c in SCALAR_COLUMNS if c in quality]
        np.savez(out / "sample_quality.npz", **quality)
        with open(out / "sample_quality.txt", "w") as f:
            f.write("# " + " ".join(cols) + "\n")
            for k in range(len(proteins)):
                f.write(" ".join(str(quality[c][k].item()) for c in cols) + "\n")
    if scaffold is not None:
        np.savez(out / "sample_scaffold.npz", keep=scaffold["keep"], ligand=scaffold["ligand"], sequence=scaffold["sequence"],
                 start=-1 if scaffold["start"] is None else scaffold["start"])
    if guided is not None:
        np.savez(out / "sample_guidance.npz", **guided)
    if handed is not None:
        from .chirality import RESULT_NAMES, TEXT_COLUMNS
        np.savez(out / "sample_handedness.npz", **handed)
        with open(out / "sample_handedness.txt", "w") as f:
            f.write("# " + " ".join(TEXT_COLUMNS) + "\n")
            for k in range(len(proteins)):
                f.write(" ".join(str(int(handed[RESULT_NAMES.get(c, c)][k])) for c in TEXT_COLUMNS) + "\n")
    if built is not None:
        np.savez(out / "sample_backbone.npz", **built)
    if secondary is not None:
        np.savez(out / "sample_secondary.npz", **{k: (np.array(v) if k == "strings" else v) for k, v in secondary.items()})
        with open(out / "sample_secondary.txt", "w") as f:
            f.write("# one line per sample, one letter per residue: - coil, H alpha helix, B bridge, E strand, G 3-10 helix, I pi helix, T turn, S bend\n")
            for line in secondary["strings"]:
                f.write(line + "\n")
    if accessibility is not None:
        from .sasa import SCALAR_COLUMNS as AREA_COLUMNS
        cols = [c for c in AREA_COLUMNS if c in accessibility]
        np.savez(out / "sample_accessibility.npz", **accessibility)
        with open(out / "sample_accessibility.txt", "w") as f:
            f.write("# " + " ".join(cols) + "\n")
            for k in range(len(proteins)):
                f.write(" ".join(str(accessibility[c][k].item()) for c in cols) + "\n")
    if sequences is not None:
        np.savez(out / "sample_sequences.npz", **{k: (np.array(v) if k == "sequences" else v) for k, v in sequences.items()})
        with open(out / "sample_sequences.fasta", "w") as f:
            for k, seq in enumerate(sequences["sequences"]):
                recovered = f" recovery={sequences['recovery'][k]:.4f}" if "recovery" in sequences else ""
                f.write(f">sample_{k} mean_logp={float(sequences['logp'][k].mean()):.4f}{recovered}\n{seq}\n")


@torch.inference_mode()
def generate_samples(model, data: Mapping[str, Any], num_samples: int, batch_size: int = 1, seed: int = 0,
                     output_dir: Optional[Union[str, Path]] = None, redesign=None, align_to=None, mirror: bool = True,
                     correspondence: str = "index", assess=None, scaffold=None, sequence_rules=None, decode=None, solver=None,
                     guidance=None, backbone=None, secondary=None, accessibility=None, handedness=None):
    """Draw ``num_samples`` samples of one featurised complex ``data`` (the dict of ligand_to_data ∪ protein_to_data).

    Returns (positions [S,N,3] in Angstrom, logits [S,N,21], proteins, ligand_positions).  With ``output_dir`` the CA
    models go to ``sample_protein.pdb`` and the ligand coordinates to ``sample_ligand_pos.npy`` (the reference writes an
    SDF through rdkit and aligns every sample with TM-align first -- both out of scope here).

    Every sample carries its DECODED sequence (generate.py:83-91 decodes every sample): residues decoded as 'X' become
    aatype -1 and are written as UNK; the input sequence is never silently kept.  The reference strips leading / trailing X
    and raises on an inner one (``RESIDUE_TYPES.index("X")``); keeping the length and marking the residue instead keeps the
    CA trace and the sequence aligned.  A ``UserWarning`` names the samples that contain undetermined residues.

    ``redesign`` (masking.Redesign; default None: the model's own ``redesign`` attribute, else the reference's random subset): the
    residues to redesign -- the pocket within a radius of the ligand, the fraction nearest to it, or explicit positions.  A pocket
    spec on an input without coordinates (``protein_from_sequence``) is refused here, on the host data, before anything is
    uploaded.  With a spec (keyword or attribute) the return value has a FIFTH element, the mask actually used -- [N] 0/1 over
    the collated row, the same for every sample of the complex -- and ``output_dir`` also receives ``sample_redesign_mask.npy``.

    ``align_to`` (default None: nothing below happens, every return value and file is what it was): superimpose every sample on a
    reference and score it, as generate.py:163-195 does with TM-align -- here with the TM-score superposition search of
    ``protein_redesign_amd.align`` on the device, on the samples as ``model.sample`` returned them, before they are copied to the
    host.  ``"input"``: the complex's own C-alpha coordinates (refused, before anything is uploaded, for an input without
    coordinates such as ``protein_from_sequence``); ``"first"``: the first sample, the reference's fallback (a ``UserWarning``: the
    structures may then all be mirror images); a ``Protein``; or an ``[nr,3]`` array of C-alpha coordinates.  The positions that
    count are the residues whose C-alpha is marked in ``residue_atom_mask``.  ``mirror`` (default True): also fit the mirror image
    of the sample and keep the better one, as the reference does.  The transform is applied to whole rows -- the C-alpha trace and
    the ligand atoms -- so ``positions``, ``proteins`` and ``ligand_positions`` come back in the reference's frame.  The return
    value gains one trailing ``dict``: ``tmscore`` [S], ``rmsd`` [S], ``mirrored`` [S], ``rotation`` [S,3,3], ``translation`` [S,3]
    (``reference ~ translation + sample @ rotation``) and ``diversity``, the mean pairwise TM-score of the S samples among themselves (a
    float; NaN for S = 1).  ``output_dir`` also receives ``sample_tmscores.txt`` (one score per line) and ``sample_alignment.npz``.

    ``correspondence`` (default ``"index"``: residue i of the sample against residue i of the reference, everything above, a reference
    of another length is refused): ``"structure"`` aligns to a reference of ANY length -- a ``Protein`` (its residues with a C-alpha
    marked in ``atom_mask[:,1]``) or an ``[m,3]`` array, m <= 2048 -- by structure, as TM-align does, with
    ``protein_redesign_amd.tmalign`` on the device; ``"input"`` and ``"first"`` are refused (their correspondence is known), so are,
    before the model is touched, a reference with fewer than 5 C-alphas, all-zero coordinates or more than 2048 residues.  The scores
    are then TM-align's: ``tmscore`` is normalised by the reference and ``rmsd`` runs over the aligned pairs; the dict and
    ``sample_alignment.npz`` gain ``n_aligned`` [S] and ``mapping`` [S,nr] (the residue index into the reference aligned to residue
    i of the complex, -1 for none).

    ``assess`` (default None: nothing below happens, every return value and file is what it was): score every sample WITHOUT a
    superposition, with ``protein_redesign_amd.quality`` on the device, before the samples are copied to the host.  ``"self"``: the
    reference-free metrics of ``quality.assess`` -- ``ca_clashes``, ``ligand_clashes``, ``ligand_self_clashes``,
    ``ligand_bond_outliers``, ``chain_breaks``, ``pocket_size`` (each [S]) and ``pocket`` [S,nr], the residues that line the sample's
    pocket.  ``"input"``: also the metrics against the complex's own coordinates -- ``lddt_ca`` [S], ``lddt_ca_per_residue`` [S,nr] and,
    when the input has ligand positions, ``lddt_pli``, ``lddt_ligand`` and ``pocket_recall`` [S]; refused, before anything is uploaded,
    for an input without coordinates such as ``protein_from_sequence``.  A ``Protein`` of the same length: ``lddt_ca`` and
    ``lddt_ca_per_residue`` against it.  The samples are scored as ``model.sample`` returned them; every metric is built from distances,
    which the transform of ``align_to`` leaves as they are (up to its fp32 rounding), so the order of the two does not matter -- and for
    the same reason a mirror image scores like the original (``handedness`` below tells the two apart).  The return value gains one more
    trailing ``dict`` of numpy arrays, after the alignment dict when both are requested.  ``output_dir`` also receives ``sample_quality.npz`` (the dict) and
    ``sample_quality.txt``: a ``#`` line naming the columns, then one line per sample holding the scalar metrics in the order of
    ``quality.SCALAR_COLUMNS`` (those present).

    ``scaffold`` (conditioning.Scaffold, keyword only, default None: nothing below happens, every return value and file is what it was):
    keep rows of the complex where the input has them -- the residues outside the design region, those beyond a radius of the ligand,
    an explicit mask, optionally the ligand pose -- and / or start the loop from the input noised to a chosen level, and optionally
    hold the known residues' sequence rows at every step (``diffusion_model.ReverseDiffusion``).  The samples then come back in the
    INPUT's frame, the kept rows at the input's own coordinates (``align_to`` then moves them as it moves every row).  Refused, before anything is uploaded, for an input without
    coordinates such as ``protein_from_sequence``, and for ``ligand=True`` / ``Scaffold.beyond`` without ligand positions.  The return
    value gains one more trailing ``dict``, after all of the above: ``keep`` ([N] 0/1 over the collated row, the rows that were kept,
    the same for every sample of the complex), ``ligand``, ``sequence`` and ``start`` of the spec.  ``output_dir`` also receives
    ``sample_scaffold.npz`` with the same entries (``start`` is -1 there when it is None).

    ``sequence_rules`` (sequence.SequenceRules, keyword only, default None: nothing changes): which residue classes the ruled residues
    may take and an additive bias on their logits -- ``SequenceRules.for_residues(na, nr, omit="C", allow={57: "AVLI"}, bias={"G": 1.5})``
    -- applied to the sequence state after every step of the loop and to the returned logits (``diffusion_model.ReverseDiffusion``), so
    the rules show in ``logits`` and in the decoded proteins.  Refused, before the model is touched, if the table does not fit the
    ``num_atoms + num_residues`` rows of the complex.  The return value gains no element for it.

    ``decode`` (sequence.Decode, keyword only, default None: nothing below happens, decoding stays the host argmax): the logits stay on
    the device until they are decoded there by ``protein_redesign_amd.sequence`` -- the argmax at ``temperature == 0``, otherwise a draw
    from softmax(logits / temperature) by Gumbel-max, the noise coming from each sample's own keyed ``NoiseSource`` after ``sample()`` has
    returned (every earlier draw is what it was) -- and the decoded sequences are counted there.  The proteins carry the decoded tokens
    (class 0 is aatype -1, as above).  The return value gains one more trailing ``dict`` of numpy arrays, after all of the above:
    ``tokens`` [S,nr], ``sequences`` (a list of str), ``logp`` [S,nr] (the log-probability of each token at temperature 1), ``entropy``
    [S,nr] (nats), ``identity`` [S,S] (the fraction of the residues two samples share), ``diversity`` (1 - the mean off-diagonal
    identity; NaN for S = 1), ``profile`` [nr,21] (how many samples carry each class) and, with ``against="input"``, ``recovery`` [S]
    (the fraction of the input's known residues a sample reproduces) and ``recovery_design`` [S] (the same over the redesigned residues
    only); ``against="input"`` is refused, before anything is uploaded, for an input whose ``residue_type`` is all unknown.
    ``output_dir`` also receives ``sample_sequences.fasta`` (one record per sample, the header carrying the mean ``logp`` and the
    recovery) and ``sample_sequences.npz`` (the dict).

    ``solver`` (solver.Solver, keyword only, default None: nothing changes): the levels the loop visits and the update between them --
    ``Solver.ddim(50)``, ``Solver.ancestral(100)``, explicit ``timesteps`` -- handed to ``model.sample`` unchanged
    (``diffusion_model.ReverseDiffusion``): K network evaluations per sample instead of ``num_steps``.  Refused, before the model is
    touched, if it is no ``Solver``.  The return value gains no element and ``output_dir`` no file for it.

    ``guidance`` (guidance.Guidance, keyword only, default None: nothing below happens, every return value and file is what it was):
    distance restraints between rows of the complex and clash repulsion, evaluated on every step's clean-structure estimate and added to
    the predicted noise (``diffusion_model.ReverseDiffusion``).  Refused, before the model is touched, if it is no ``Guidance`` or a
    restraint names a row outside the complex's ``num_atoms + num_residues``.  The return value gains one more trailing ``dict``, after
    all of the above: the spec's terms (``restraints`` [R,2], ``restraint_bounds`` [R,3] = lo, hi, weight in Angstrom, ``clash`` = the
    three floors and the weight, ``scale``, ``cap``, ``from_level`` (-1 for None), ``schedule``), ``energy`` [S,2] -- the clash and the
    restraint energy of the samples as the model returned them, from ``guidance.energy`` -- and, when the input has coordinates,
    ``input_energy`` [2], the same of the input structure.  ``output_dir`` also receives ``sample_guidance.npz`` (the dict).

    ``handedness`` (``"report"``, ``"fix"`` or a chirality.Handedness, keyword only, default None: nothing below happens, every launch,
    draw, return value and file is what it was): tell mirror-image samples from their natural hand WITHOUT a reference, with
    ``protein_redesign_amd.chirality`` on the device -- a census of the C-alpha trace's virtual dihedrals (right- against left-handed
    helical turns, the twist of extended stretches) and of the signed volumes at the ligand's tagged stereocentres, compared with the
    input's own when the input has ligand coordinates -- and a verdict per sample.  The census runs once over all samples as
    ``model.sample`` returned them, before they are copied to the host.  Under ``"fix"`` the samples judged mirrored (verdict -1) are
    reflected in place, exactly (the x coordinate negated): the network is reflection-equivariant, so the mirror image of a sample is an
    equally valid sample.  ``assess``, the guidance report, ``align_to`` and the decoding then see the result: distance metrics do not
    change, and ``alignment["mirrored"]`` reports on the fixed sample.  Refused, before the model is touched: any other value, and
    ``"fix"`` together with a ``scaffold`` (the kept rows pin the hand; ``"report"`` is allowed).  The return value gains one more
    trailing ``dict`` of numpy values, after all of the above: ``verdict`` (+1 natural, -1 mirrored, 0 undecided), ``basis`` (the rule
    that decided: 1 helices, 2 ligand centres, 3 extended stretches, 0 none) and ``flipped``, each [S]; ``helix_right``, ``helix_left``,
    ``extended_native``, ``extended_mirror``, ``quads``, ``ligand_kept``, ``ligand_inverted``, ``ligand_flat`` [S]; ``helix_fraction``,
    ``extended_fraction`` [S]; ``tau`` (radians, NaN where a residue starts no quad) and ``classes`` [S,nr]; ``ligand_centres`` [C] (atom
    indices) and ``ligand_volume`` [S,C]; and, when the input has C-alpha coordinates, ``input_verdict``, ``input_basis`` and
    ``input_counts`` [8] of the input structure.  The census values describe the samples AS DRAWN; ``flipped`` says which were
    reflected, and by the exact symmetry a flipped sample's counts are the swapped ones.  ``output_dir`` also receives
    ``sample_handedness.npz`` (the dict) and ``sample_handedness.txt``: a ``#`` line naming the columns, then one line per sample holding
    verdict, basis, flipped and the eight counts.  Nothing is claimed about how often a real sample is decided.

    ``backbone`` (``"build"`` or a backbone.Backbone, keyword only, default None: nothing below happens, every launch, draw, return
    value and file is what it was): build N, C, O and CB of every residue from the C-alpha trace, with ``protein_redesign_amd.backbone``
    on the device -- a rigid planar trans peptide between consecutive C-alphas, turned about the CA-CA axis by an angle read off a table
    of the C-alpha virtual dihedral (include/prd_backbone.h).  It is the LAST stage on the device: after the handedness fix, ``assess``,
    the guidance report and ``align_to``, which may have reflected the sample, so the atoms come back in the final frame and on the
    final hand.  The residues are L-residues whatever the trace: without ``handedness`` a ``UserWarning`` says that mirrored samples get
    L-residues on a D-trace (a ``scaffold`` pins the hand, and nothing is refused with one).  The proteins' ``atom_pos`` / ``atom_mask``
    then carry N, CA, C, O and CB (no CB on a residue decoded as G or left undetermined), and ``sample_protein.pdb`` holds them.  Only
    chain stretches of at least 4 residues with virtual bonds inside the spec's window are built; elsewhere a residue keeps its CA alone.
    Refused, before the model is touched: any other value.  The return value gains one more trailing ``dict`` of numpy values, after all
    of the above: ``atoms`` [S,nr,5,3] (N, CA, C, CB, O; zeros where not built), ``built`` [S,nr,5] (bool, as the launch decided: CB is
    marked on G too), ``unbuilt_residues`` [S] (residues without their N, C or O), ``table`` [73] (radians) and the geometry (``L0``,
    ``plane_C``, ``plane_O``, ``plane_N``, ``cb``, ``bond``, ``min_angle``).  ``output_dir`` also receives ``sample_backbone.npz`` (the
    dict).  Nothing is claimed about accuracy on real proteins.

    ``secondary`` (``"assign"`` or a dssp.Dssp, keyword only, default None: nothing below happens, every launch, draw, return value and
    file is what it was): the secondary structure of every sample, with ``protein_redesign_amd.dssp`` on the device -- the Kabsch-Sander
    hydrogen-bond energy between every C=O and every N-H, then turns, helices, bridges and ladders read off the bond pattern
    (include/prd_dssp.h, which lists its three deviations from DSSP proper).  It needs the atoms: ``secondary`` without ``backbone`` is
    refused before the model is touched (use ``backbone="build"``), and so is any other value.  The stage runs directly after the
    backbone stage, on the device tensors ``backbone.build`` left.  The donor mask is NOT derived from the decoded sequence: proline
    donates like every other residue.  The return value gains one more trailing ``dict`` of numpy values, after the backbone's:
    ``classes`` [S,nr] (uint8 codes into ``"-HBEGITS"``), ``strings`` (a list of str), ``partner`` and ``energy`` [S,nr,4] (the two best
    acceptors of a residue as donor, then its two best donors as acceptor; residue indices, -1 for none; kcal/mol), ``bridge`` [S,nr,2],
    ``counts`` [S,8], ``helix_fraction`` (H, G, I), ``strand_fraction`` (E, B) and ``hbonds`` [S].  When the input's
    ``residue_atom_mask`` has N, CA, C and O, also ``input_classes`` [nr] -- the same two calls on the input's own atoms -- and ``q3`` /
    ``q8`` [S], the share of residues whose three-state / eight-state class equals the input's, over the residues classed in both.
    ``output_dir`` also receives ``sample_secondary.npz`` (the dict) and ``sample_secondary.txt``: a ``#`` line, then one class string
    per sample.  Every quantity is a function of distances, so a mirror image is classed like the original.  Nothing is claimed about
    accuracy on real proteins: off the builder's anchor conformations its oxygen is off by up to 1.2 Angstrom, and strand pairing from
    BUILT atoms is expected to be fragile.

    ``accessibility`` (``"measure"`` or a sasa.Accessibility, keyword only, default None: nothing below happens, every launch, draw,
    return value and file is what it was): how buried every residue is, how much of the ligand's surface the protein covers and the area
    of their interface, with ``protein_redesign_amd.sasa`` on the device -- Shrake and Rupley's point count (include/prd_sasa.h) on the
    built atoms N, CA, C, CB and O of every residue and the ligand rows ``positions[:, :na]``, each with its van der Waals radius plus the
    probe, the ligand's by the element of ``atom_feats[..., 0]``.  It needs the atoms: ``accessibility`` without ``backbone`` is refused
    before the model is touched (use ``backbone="build"``), and so is any other value.  The stage runs after the backbone stage (and
    after ``secondary``), on the device tensors ``backbone.build`` left; a residue that kept its C-alpha alone contributes that C-alpha,
    and CB takes part on every built residue -- the decoded sequence is NOT consulted.  The return value gains one more trailing ``dict``
    of numpy values, after the secondary-structure dict: ``atom_area`` [S,nr,5] (Angstrom^2), ``residue_area``, ``relative`` (the
    residue's area over ``sasa.REFERENCE_AREA``, the same residue in an extended chain), ``buried`` (relative < buried_below) and
    ``complete`` (N, CA, C and O present), each [S,nr]; ``ligand_area`` and ``ligand_area_free`` [S,na] (in the complex / the ligand
    alone); ``ligand_buried_fraction`` [S]; ``interface_area`` [S] (what both partners lose on complexation); ``interface_residues``
    [S,nr] (residues that lose area to the ligand); ``total_area`` and ``buried_residues`` [S]; and the spec (``probe``, ``points``,
    ``buried_below``, ``backbone_radii``, ``ligand_radii`` [119], ``reference_area``).  When the input's ``residue_atom_mask`` has N, CA,
    C and O, also ``input_relative`` [nr] -- the same call on the input's own atoms (with its ligand, when it has coordinates) -- and
    ``burial_agreement`` [S], the share of residues called buried or exposed as in the input, over the residues whole in both.
    ``output_dir`` also receives ``sample_accessibility.npz`` (the dict) and ``sample_accessibility.txt``: a ``#`` line naming the
    columns, then one line per sample holding the scalar columns of ``sasa.SCALAR_COLUMNS`` (those present).  The counts are exact
    integers; nothing is claimed about real proteins: without side chains beyond CB the areas are those of a poly-alanine-like model
    and overestimate exposure.  The point lattice is not mirror-symmetric: a mirror image gets nearly, not exactly, the same areas."""
    if guidance is not None:
        from .guidance import check_guidance
        check_guidance(guidance)
        guidance.check_rows(int(data["num_atoms"]) + int(data["num_residues"]), "the complex's num_atoms + num_residues rows")
    if solver is not None:
        from .solver import Solver
        if not isinstance(solver, Solver):
            raise TypeError(f"solver must be a solver.Solver, got {type(solver).__name__}")
    if backbone is not None:
        from .backbone import Backbone
        backbone = Backbone.of(backbone)
    if secondary is not None:
        from .dssp import Dssp
        secondary = Dssp.of(secondary)
        if backbone is None:
            raise ValueError("secondary= assigns secondary structure from N, C and O, which the samples do not have: use it with backbone=\"build\"")
    if accessibility is not None:
        from .sasa import Accessibility
        accessibility = Accessibility.of(accessibility)
        if backbone is None:
            raise ValueError("accessibility= measures the surface of N, CA, C, CB and O, which the samples do not have: use it with backbone=\"build\"")
    struct_ref, align_ref, quality_ref, spec = _references(model, data, redesign, align_to, correspondence, assess, scaffold,
                                                           sequence_rules, decode, handedness)
    device = model.device
    if handedness is not None:
        from .chirality import Handedness
        handedness = Handedness.of(handedness)
    if sequence_rules is not None:
        sequence_rules = sequence_rules.to(device)      # the table is uploaded once, not per batch
    if scaffold is not None:
        scaffold = scaffold.to(device)          # a keep mask is uploaded once, not per batch
    if spec is not None:
        spec = spec.to(device)                  # a positions mask is uploaded once, not per batch
    na, nr = int(data["num_atoms"]), int(data["num_residues"])
    scored = align_to is not None or assess is not None or guidance is not None or handedness is not None or backbone is not None     # then the samples stay on the device until they are scored
    drawn, logits, first_batch, sources = _draw(model, data, num_samples, batch_size, seed, spec, device, keep_on_device=scored,
                                                scaffold=scaffold, sequence_rules=sequence_rules, keep_logits=decode is not None,
                                                solver=solver, guidance=guidance)
    # every sample of the complex shares the mask: read from the first prepared batch, after the loop (no synchronisation inside it)
    used_mask = first_batch["residue_inv_extra_mask"][0].cpu().numpy() if spec is not None and first_batch is not None else None
    kept = None
    if scaffold is not None:                    # like the mask: read from the first prepared batch, after the loop
        from .conditioning import BATCH_KEY
        kept = {"keep": first_batch[BATCH_KEY][0].cpu().numpy(), "ligand": scaffold.ligand, "sequence": scaffold.sequence,
                "start": scaffold.start}
    pos = torch.cat(drawn)
    handed = None
    if handedness is not None:
        pos = pos.float().contiguous()          # what torch.cat made already, said once: the reflection works in place
        handed = _handedness_report(handedness, data, pos, first_batch, na, nr)
    quality = _assess(pos, first_batch, quality_ref, na, nr) if assess is not None else None
    guided = _guidance_report(guidance, data, pos, first_batch, na, nr) if guidance is not None else None
    pos, alignment = _superpose(pos, data, struct_ref, align_ref, mirror, na, nr) if align_to is not None else (pos, None)
    built = assigned = surface = None
    if backbone is not None:
        if handedness is None and scaffold is None:
            warnings.warn("backbone= without handedness=: the builder places L-residues whatever the trace, so a mirror-image sample gets "
                          "L-residues on a D-trace; use handedness='fix'", UserWarning)
        built, on_device = _backbone_atoms(backbone, pos, first_batch, na, nr)
        if secondary is not None:
            assigned = _secondary_structure(secondary, data, on_device, na, nr)
        if accessibility is not None:
            surface = _accessibility(accessibility, data, on_device, pos, first_batch, na, nr)
    sequences = None
    if decode is not None:
        design = first_batch.get("residue_inv_extra_mask") if first_batch is not None else None      # the prepared batch carries it
        design = design[0].cpu().numpy() if design is not None else None
        on_device = torch.cat(logits)
        sequences = _decode_on_device(data, on_device, sources, decode, sequence_rules is not None, design, na, nr)
        logits = [on_device.cpu()]
    positions, logits = pos.cpu().numpy(), torch.cat(logits).numpy()       # the one copy of scored samples; unscored ones are on the host
    if alignment is not None:
        alignment = {k: float(v.cpu()) if k == "diversity" else v.cpu().numpy() for k, v in alignment.items()}
    proteins, ligands = _decode(data, positions, logits, na, nr, sequences["tokens"] if sequences is not None else None)
    if built is not None:
        proteins = _with_backbone(proteins, built)
    if output_dir is not None:
        _write(output_dir, proteins, ligands, used_mask, alignment, quality, kept, sequences, guided, handed, built, assigned, surface)
    result = (positions, logits, proteins, ligands) + ((used_mask,) if spec is not None else ())
    result = result + ((alignment,) if alignment is not None else ()) + ((quality,) if quality is not None else ())
    result = result + ((kept,) if kept is not None else ()) + ((sequences,) if sequences is not None else ())
    result = result + ((guided,) if guided is not None else ()) + ((handed,) if handed is not None else ())
    result = result + ((built,) if built is not None else ()) + ((assigned,) if assigned is not None else ())
    return result + ((surface,) if surface is not None else ())
