"""CPU: the host-only answers of the general-layout triangle-attention entries (prd_tri_attn_heads_supported /
prd_tri_attn_heads_workspace_bytes), their declarations against the ctypes binding table, and the Python-side layout check."""
import os
import re

import pytest

from conftest import ROOT
from protein_redesign_amd import _lib, ops

ENTRIES = ("prd_tri_attn_heads_supported", "prd_tri_attn_heads_workspace_bytes", "prd_tri_attn_core_heads")


def test_header_and_binding_entries():
    text = open(os.path.join(ROOT, "include", "prd_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(prd_\w+)\s*\(", text, flags=re.M))
    for n in ENTRIES:
        assert n in declared, n
        assert n in _lib.SIGNATURES, n
        assert hasattr(_lib.lib(), n), n
    assert _lib.lib().prd_version() == 101


@pytest.mark.parametrize("arith", [0, 1])
def test_supported_set(arith):
    L = _lib.lib()
    raw = L._cdll.prd_tri_attn_heads_supported
    for H in range(0, 10):
        for c in range(0, 130, 2):
            for P in (16, 32, 48, 64, 128):
                want = int(1 <= H <= 8 and 4 <= c <= 64 and c % 4 == 0 and P in (32, 64))
                assert raw(97, P, H, c, arith) == want, (H, c, P)
    assert raw(0, 64, 8, 32, arith) == 0
    assert raw(1, 64, 8, 32, arith) == 1
    assert raw(100000, 32, 1, 4, arith) == 1            # no row limit
    assert raw(97, 64, 8, 32, 7) == -1                  # an invalid arithmetic word
    assert ops.tri_attn_heads_supported(320, 64, 4, 16)    # the 4 x 16 layout too


def test_workspace_bytes():
    L = _lib.lib()
    assert L.prd_tri_attn_heads_workspace_bytes(2, 97, 64, 8, 32) == 2 * 97 * 97 * 256 * 4
    assert L.prd_tri_attn_heads_workspace_bytes(1, 1100, 64, 8, 64) == 1100 * 1100 * 512 * 4    # beyond 2^31 bytes
    assert L.prd_tri_attn_heads_workspace_bytes(1, 30, 32, 3, 20) == 30 * 30 * 60 * 4
    for bad in ((0, 30, 64, 8, 32), (1, 0, 64, 8, 32), (1, 30, 48, 8, 32), (1, 30, 64, 9, 32), (1, 30, 64, 4, 18)):
        assert L.prd_tri_attn_heads_workspace_bytes(*bad) == 0, bad
    assert ops.tri_attn_heads_ws_floats(2, 97, 64, 8, 32) == 2 * 97 * 97 * 256


def test_layout_check_names_the_supported_set():
    for H, c, P in ((8, 32, 64), (1, 4, 32), (5, 12, 64), (4, 64, 32)):
        ops.check_head_layout(H, c, P)
    for H, c, P in ((4, 18, 64), (4, 128, 64), (9, 16, 64), (0, 16, 64), (4, 16, 16)):
        with pytest.raises(ValueError, match=r"num_heads 1\.\.8, head_dim a multiple of 4 up to 64, pair_dim 32/64"):
            ops.check_head_layout(H, c, P)
    assert ops.default_head_layout(4, 16) and not ops.default_head_layout(8, 32) and not ops.default_head_layout(2, 32)
