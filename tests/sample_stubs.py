"""Stand-ins shared by the CPU tests of the sample post-processing path (pipeline.generate_samples and its side libraries)."""
import os

import torch

from conftest import ROOT
from protein_redesign_amd import _lib


def header_entries(name):
    """the parsed prototypes of include/prd_<name>.h"""
    with open(os.path.join(ROOT, "include", f"prd_{name}.h")) as f:
        return _lib.parse_header(f.read())


class _NoDevice:
    """A model stand-in whose every attribute access fails: generate_samples must refuse before it touches the model."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the input was checked")


class _Stub:
    """a model whose samples are a function of the keyed noise source alone; a ``redesign`` with a positions mask is written into the
    batch as ``residue_inv_extra_mask``, where the real model leaves the mask it used"""
    device = torch.device("cpu")

    def sample(self, batch, sources, redesign=None):
        n = batch["atom_mask"].shape[1]
        if redesign is not None:
            batch["residue_inv_extra_mask"] = batch["residue_mask"] * redesign.mask
        return (torch.stack([torch.randn(n, 3, generator=s.g) for s in sources]), torch.stack([torch.randn(n, 21, generator=s.g) for s in sources]))
