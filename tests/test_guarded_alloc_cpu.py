"""The guarded-buffer harness (tests/guarded_alloc.py) has teeth -- shown on CPU tensors, without a GPU -- and no allocation of the
package escapes it (source-level check)."""
import ast
import glob
import os
import struct

import pytest
import torch

import guarded_alloc as GA
from guarded_alloc import G, HUGE, check_written, guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pattern_value_is_the_float_of_four_0x7f_bytes():
    assert struct.unpack("<f", b"\x7f\x7f\x7f\x7f")[0] == HUGE == float(torch.tensor([0x7F7F7F7F], dtype=torch.int32).view(torch.float32))
    assert HUGE == (1 + 0x7F7F7F * 2.0 ** -23) * 2.0 ** 127 and 3.396e38 < HUGE < 3.397e38      # exponent 0xFE, mantissa 0x7F7F7F: finite


@pytest.mark.parametrize("poison", ["nan", "huge"])
def test_planted_writes_outside_the_interior_are_reported(poison):
    from protein_redesign_amd import ops
    with guarded(poison, cpu=True) as g:
        assert ops.torch is g.torch
        t = g.torch
        a = t.empty(3, 5)
        b = t.empty(7, dtype=torch.int64)
        c = t.zeros(2, 3)
        assert g.intact(), g.report()
        raw, n = g.records[1][:2]
        assert n == 56 and raw.numel() == 2 * G + 56 and raw.data_ptr() + G == b.data_ptr()
        raw[G - 1] = 0                                  # one byte before b
        assert not g.intact()
        assert len(g.violations) == 1 and "allocation #1 [7] torch.int64" in g.report() and "before the tensor" in g.report()
        assert "offset -1 " in g.report()
        raw[G - 1] = g.byte
        assert g.intact()
        raw0, n0 = g.records[0][:2]
        raw0[G + n0] = 1                                # the first byte after a: no rounding up to 16
        assert not g.intact()
        assert len(g.violations) == 1 and "allocation #0 [3, 5] torch.float32" in g.report() and "after the tensor" in g.report()
        assert "offset +0 " in g.report()
        assert "test_planted_writes" in g.report()      # where it was allocated
        raw0[G + n0] = g.byte
        raw2, n2 = g.records[2][:2]
        raw2[-1] = 3                                    # the last guard byte of c
        assert not g.intact() and "allocation #2 [2, 3]" in g.report() and f"offset +{G - 1} " in g.report()
        del a, c
    assert ops.torch is torch and not set(GA._REAL_NEW) & set(vars(torch.Tensor))       # everything is as it was


def test_unwritten_interior_elements_show_the_poison():
    with guarded("nan", cpu=True) as g:
        x = g.torch.empty(4, 6)
        x[:, :5] = 1.0                                  # the "kernel" leaves the last column unwritten
        assert not torch.isfinite(x[:, 5]).any() and torch.isfinite(x[:, :5]).all()
        with pytest.raises(AssertionError, match=r"x \[4, 6\]: 4 of 24 elements"):
            check_written("x", x)
        check_written("x", x[:, :5])
        assert g.intact()
        assert not torch.isfinite(g.torch.empty_like(x)).any()
    with guarded("huge", cpu=True) as g:
        x = g.torch.empty(4, 6)
        x[:, :5] = 1.0
        assert torch.isfinite(x).all()
        assert bool((x[:, 5] == HUGE).all()) and float(x[0, 5]) == HUGE
        with pytest.raises(AssertionError, match="first at \\[\\[0, 5\\], \\[1, 5\\]"):
            check_written("x", x)
        check_written("x", x[:, :5]), check_written("none", None), check_written("ints", torch.full((3,), 0x7F7F7F7F))
        assert g.intact()
        y = x.new_empty(3)
        assert bool((y == HUGE).all()) and len(g.records) == 2
        i = g.torch.empty(5, dtype=torch.int32)
        assert bool((i == 0x7F7F7F7F).all())


@pytest.mark.parametrize("poison", ["nan", "huge"])
def test_filled_factories_keep_their_values_inside_poisoned_guards(poison):
    with guarded(poison, cpu=True) as g:
        t = g.torch
        like = torch.randn(3, 4)
        outs = [t.zeros(5, 3), t.zeros_like(like), t.zeros(6, dtype=torch.int32), like.new_zeros(2, 2)]
        for z in outs:
            assert bool((z == 0).all())
        assert bool((t.ones(3) == 1).all()) and bool((t.full((2, 3), 2.5) == 2.5).all()) and bool((like.new_ones(4) == 1).all())
        assert bool((t.full_like(like, float("inf")) == float("inf")).all()) and bool((like.new_full((2,), 7.0) == 7).all())
        assert len(g.records) == 9
        for raw, n, *_ in g.records:
            assert bool((raw[:G] == g.byte).all()) and bool((raw[G + n:] == g.byte).all())
        assert g.intact()


def test_views_equal_the_unpatched_calls():
    base = torch.randn(4, 5, 6)
    permuted = base.permute(2, 0, 1)                    # dense, not contiguous: empty_like keeps its strides
    calls = [
        ("empty", (3, 5), {}), ("empty", ((2, 7),), {"dtype": torch.int64}), ("empty", (2, 3, 4), {"dtype": torch.float64}),
        ("zeros", (9,), {"dtype": torch.int32}), ("ones", (2, 2), {}), ("full", ((3, 3), 1.5), {}),
        ("empty_like", (base,), {}), ("empty_like", (permuted,), {}), ("zeros_like", (base[:, 1],), {}),
        ("empty_like", (base,), {"dtype": torch.int64}), ("empty", (1, 1), {"dtype": torch.uint8}), ("empty", (7,), {"dtype": torch.float16}),
        ("empty_strided", ((3, 4), (1, 3)), {}),
    ]
    with guarded("nan", cpu=True) as g:
        for name, args, kw in calls:
            want = getattr(torch, name)(*args, **kw)
            got = getattr(g.torch, name)(*args, **kw)
            assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device, name
            assert got.stride() == want.stride() and got.is_contiguous() == want.is_contiguous(), name
            assert got.data_ptr() % 64 == 0, name       # the interior keeps the allocator's alignment (G = 4096)
        assert len(g.records) == len(calls)
        for name, args in (("new_empty", (3, 2)), ("new_zeros", (4,)), ("new_ones", (2, 2))):
            want, got = GA._REAL_NEW[name](base, *args), getattr(base, name)(*args)
            assert got.shape == want.shape and got.dtype == want.dtype and got.is_contiguous()
        assert len(g.records) == len(calls) + 3
        # not carved: empty tensors, an out= call, CPU tensors without the flag (below)
        assert g.torch.empty(0, 3).numel() == 0 and len(g.records) == len(calls) + 3
        x = g.put(base[:, :, 2])
        assert x.is_contiguous() and torch.equal(x, base[:, :, 2]) and g.records[-1][4] == "put"
        assert g.intact()
    with guarded("nan") as g:
        assert torch.equal(g.torch.zeros(3), torch.zeros(3)) and not g.records


def test_caches_are_emptied_and_restored():
    from protein_redesign_amd import ops
    sentinel = object()
    lin = torch.nn.Linear(2, 2)
    ops._GEMM_WS["k"] = sentinel
    lin.__dict__["_prd_pack_cache"] = {"x": 1}
    try:
        with guarded("nan", modules=[lin], cpu=True):
            assert not ops._GEMM_WS and not ops._QUEUES and not ops._PAIR_BARS and "_prd_pack_cache" not in lin.__dict__
            ops._GEMM_WS["inside"] = 1
            lin.__dict__["_prd_pack_cache"] = {"y": 2}
        assert ops._GEMM_WS == {"k": sentinel} and "_prd_pack_cache" not in lin.__dict__
    finally:
        ops._GEMM_WS.pop("k", None)


# every torch factory that returns a new tensor whose contents do not come from another tensor
ALLOCATING = {"empty", "empty_like", "empty_strided", "empty_permuted", "zeros", "zeros_like", "ones", "ones_like", "full", "full_like"}


def test_no_allocation_of_the_package_escapes_the_harness():
    """Every ``torch.<allocating factory>(`` and every ``.new_<name>(`` call in protein_redesign_amd/*.py is in the harness's wrapped
    set, and reaches it: the factories are called as attributes of the module-level ``torch`` (which the harness replaces), never
    imported by name."""
    files = sorted(glob.glob(os.path.join(ROOT, "protein_redesign_amd", "*.py")))
    assert len(files) > 10
    seen = set()
    for path in files:
        tree = ast.parse(open(path).read(), path)
        name = os.path.basename(path)
        top_torch = any(isinstance(n, ast.Import) and any(a.name == "torch" and a.asname is None for a in n.names) for n in tree.body)
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module == "torch":
                assert not {a.name for a in node.names} & (ALLOCATING | GA.WRAPPED), f"{name}:{node.lineno} imports a factory by name"
            if isinstance(node, ast.Import) and not any(node is n for n in tree.body):
                assert all(a.name != "torch" for a in node.names), f"{name}:{node.lineno}: a local 'import torch' bypasses the harness"
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
                continue
            attr = node.func.attr
            if isinstance(node.func.value, ast.Name) and node.func.value.id == "torch" and attr in ALLOCATING:
                assert attr in GA.WRAPPED, f"{name}:{node.lineno}: torch.{attr} is not wrapped by tests/guarded_alloc.py"
                assert top_torch, f"{name}: torch.{attr} is used but torch is not imported at module level"
                seen.add(attr)
            elif attr.startswith("new_") and attr != "new_tensor":
                assert attr in GA.WRAPPED, f"{name}:{node.lineno}: .{attr} is not wrapped by tests/guarded_alloc.py"
                seen.add(attr)
    assert {"empty", "empty_like", "zeros", "zeros_like"} <= seen          # the parser found the calls it is about
    for mod in GA.MODULES:
        assert os.path.join(ROOT, "protein_redesign_amd", mod + ".py") in files
