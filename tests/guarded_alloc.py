"""Guarded, poisoned device buffers for the operator tests (a helper module, imported by tests; not a conftest).

``guarded(poison)`` is a context manager.  For its duration every allocation the package makes through the factories in
``WRAPPED`` (``torch.empty`` / ``empty_like`` / ``zeros`` / ... and ``Tensor.new_*``) is carved out of a larger ``uint8`` buffer

    [ G guard bytes | the tensor's bytes | G guard bytes ]          G = 4096

filled with the poison byte: the tensor the package gets is the interior viewed as the requested dtype and shape.  The trailing
guard starts at the first byte after the tensor (no rounding), so a ragged row finished with a full float4 store lands in it.  A
kernel that writes outside its buffer changes guard bytes (``intact()``); an element it never writes keeps the poison; a read of
memory nobody wrote returns the poison instead of what the caching allocator happened to hand back.

Two patterns (``POISON``): 0xFF -- every float32 reads as NaN; 0x7F -- every float32 reads as 3.396e38, finite: ``v_max_f32`` /
``fmaxf`` drop a NaN operand, so an uninitialised value fed to a softmax running maximum is invisible under NaN and dominant
under the huge pattern.

The factories are replaced by binding a proxy ``torch`` into the package's modules (``import torch`` at module level), so the
allocations of the test itself and of PyTorch's own Python code stay as they are; ``Tensor.new_*`` is patched on the class.
Filled factories (``zeros``, ``ones``, ``full``) get their values in the interior and poisoned guards.  Every carved buffer
stays alive until the manager exits, so a late overrun cannot hide in a freed block.  The package's cached device buffers
(``ops._GEMM_WS``, ``ops._QUEUES``, ``ops._PAIR_BARS``) are emptied for the duration -- they are re-made guarded -- and restored
afterwards; what ``ops.cached_pack`` hangs on the ``modules`` given is reset on entry and on exit.

Limits.  (1) Only factory calls are carved.  A buffer the package makes with ``.clone()``, ``.contiguous()``, ``.to(device)``,
``torch.cat`` / ``stack`` or torch arithmetic has no guards, although kernels may write it in place: ``ReverseDiffusion.z`` /
``seq_t`` / ``noise``, the ``cached_pack`` results; model weights are plain allocations too, so a read past the end of a weight
does not meet poison.  Test inputs get guards through ``put``.  (2) 0x7F is finite for float32 (and bfloat16) only: read as
float16, 0x7F7F is a NaN, so for a buffer a kernel reads as packed fp16 planes both patterns are NaN and the second adds nothing;
``check_written`` compares float32 tensors with the float32 value.  (3) Under ``torch.cuda.graph`` the poison fills (and the copies
of the filled factories) are captured with the step: the guarded graph has more launches than the shipped one, and every replay
re-poisons every carved buffer before the step's kernels run (an overrun of the last replay is still there afterwards).
"""
import contextlib
import importlib
import struct
import sys
import types

import torch

G = 4096
POISON = {"nan": 0xFF, "huge": 0x7F}
HUGE = struct.unpack("<f", b"\x7f" * 4)[0]          # the float32 with all four bytes 0x7F: 3.3961514e38

# factories that allocate a tensor without taking its data from another one
UNFILLED = ("empty", "empty_like", "empty_strided")
FILLED = ("zeros", "zeros_like", "ones", "ones_like", "full", "full_like")
NEW_UNFILLED = ("new_empty", "new_empty_strided")
NEW_FILLED = ("new_zeros", "new_ones", "new_full")
WRAPPED = frozenset(UNFILLED + FILLED + NEW_UNFILLED + NEW_FILLED)

# the modules that must be covered; every other loaded module of the package that imported torch is covered as well
MODULES = ("ops", "trunk", "af2_blocks", "diffusion_model", "training", "masking")

_REAL = {name: getattr(torch, name) for name in UNFILLED + FILLED}
_REAL_NEW = {name: getattr(torch.Tensor, name) for name in NEW_UNFILLED + NEW_FILLED}


def _dense(t) -> bool:
    """True when ``t`` covers exactly numel elements of storage (contiguous in some permutation of its dimensions)."""
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


class _TorchProxy(types.ModuleType):
    """``torch`` with the allocating factories replaced; everything else is the real module's."""

    def __init__(self, table):
        super().__init__("torch")
        self.__dict__.update(table)

    def __getattr__(self, name):
        return getattr(torch, name)


class Guard:
    def __init__(self, poison="nan", cpu=False):
        self.byte = POISON[poison]
        self.cpu = cpu
        self.records = []               # (raw uint8 buffer, interior bytes, shape, dtype, where)
        self.violations = []

    # -- carving ---------------------------------------------------------------------------------------------------------------
    def _wanted(self, r) -> bool:
        return (type(r) is torch.Tensor and r.layout == torch.strided and r.numel() > 0 and not r.requires_grad
                and not r.dtype.is_complex and (r.device.type == "cuda" or (self.cpu and r.device.type == "cpu")) and _dense(r))

    def carve(self, like, fill=False, where=""):
        """A tensor of ``like``'s shape, strides, dtype and device inside a guarded buffer of its own: the interior holds ``like``'s
        values with ``fill``, else the poison."""
        n = like.numel() * like.element_size()
        raw = _REAL["full"]((G + n + G,), self.byte, dtype=torch.uint8, device=like.device)
        out = raw[G:G + n].view(like.dtype).as_strided(like.shape, like.stride())
        if fill:
            out.copy_(like)
        self.records.append((raw, n, tuple(like.shape), like.dtype, where))
        return out

    def _wrap(self, real, fill):
        def factory(*args, **kwargs):
            r = real(*args, **kwargs)
            if kwargs.get("out") is not None or not self._wanted(r):
                return r
            f = sys._getframe(1)                        # the caller: names the allocation in a report
            return self.carve(r, fill, f"{real.__name__} in {f.f_code.co_name}:{f.f_lineno}")
        factory.__name__ = getattr(real, "__name__", "factory")
        return factory

    def put(self, tensor, device=None):
        """A copy of a test input in a guarded buffer of its own (contiguous, on ``device`` if given): a read past its end meets
        poison too."""
        src = tensor.detach()
        src = (src.to(device) if device is not None else src).contiguous()
        if src.numel() == 0:
            return src
        return self.carve(src, True, "put")

    def empty(self, *shape, dtype=torch.float32, device=None):
        """A poisoned output buffer for a test that passes ``out=`` itself."""
        return self.carve(_REAL["empty"](*shape, dtype=dtype, device=device), False, "test")

    # -- checking --------------------------------------------------------------------------------------------------------------
    def intact(self) -> bool:
        """True when no guard byte of any buffer carved so far has changed.  Reduced on the device: one flag is read back per
        device; only after a violation are the buffers looked at one by one (``violations`` then names each: allocation order,
        shape, dtype, where it was allocated, the side and the offset of the first changed byte)."""
        self.violations = []
        by_dev = {}
        for k, (raw, n, *_rest) in enumerate(self.records):
            by_dev.setdefault(raw.device, []).append((k, raw, n))
        for dev, items in by_dev.items():
            guards = torch.stack([g for _, raw, n in items for g in (raw[:G], raw[G + n:])])
            bad = (guards != self.byte).any(dim=1)
            if not bool(bad.any()):
                continue
            for row in bad.nonzero().flatten().tolist():
                k, raw, n = items[row // 2]
                _, _, shape, dtype, where = self.records[k]
                side = "before" if row % 2 == 0 else "after"
                changed = (guards[row] != self.byte).nonzero().flatten()
                first = int(changed[0]) if side == "after" else int(changed[-1]) - G       # the changed byte nearest to the tensor
                self.violations.append(f"allocation #{k} {list(shape)} {dtype} ({where}): {int(changed.numel())} guard bytes changed "
                                       f"{side} the tensor, nearest at byte offset {first:+d} from its "
                                       f"{'end' if side == 'after' else 'start'}")
        return not self.violations

    def report(self) -> str:
        return "; ".join(self.violations) if self.violations else "all guards intact"


def check_written(name, t):
    """Raises AssertionError unless the tensor ``t`` (None and integer tensors pass) is finite and free of the 0x7F pattern value:
    an element a kernel never wrote, or one computed from memory nobody wrote."""
    if t is None or not t.is_floating_point():
        return
    bad = ~torch.isfinite(t) | (t == HUGE)
    assert not bool(bad.any()), (f"{name} {list(t.shape)}: {int(bad.sum())} of {t.numel()} elements are non-finite or hold the poison pattern; "
                                 f"first at {bad.nonzero()[:4].tolist()}")


def _package_modules():
    for name in MODULES:
        importlib.import_module("protein_redesign_amd." + name)
    return [m for name, m in sorted(sys.modules.items())
            if name.startswith("protein_redesign_amd.") and m is not None and getattr(m, "torch", None) is torch]


def _reset_packs(modules):
    for root in modules:
        for m in root.modules():
            m.__dict__.pop("_prd_pack_cache", None)


@contextlib.contextmanager
def guarded(poison="nan", modules=(), cpu=False):
    """See the module docstring.  ``modules``: the nn.Modules used inside (their ``ops.cached_pack`` entries are reset);
    ``cpu``: carve CPU allocations too (the harness's own CPU test)."""
    from protein_redesign_amd import ops
    g = Guard(poison, cpu)
    table = {name: g._wrap(_REAL[name], name in FILLED) for name in UNFILLED + FILLED}
    proxy = _TorchProxy(table)
    g.torch = proxy
    patched = _package_modules()
    caches = [(c, dict(c)) for c in (ops._GEMM_WS, ops._QUEUES, ops._PAIR_BARS)]
    try:
        for c, _ in caches:
            c.clear()
        _reset_packs(modules)
        for m in patched:
            m.torch = proxy
        for name, real in _REAL_NEW.items():
            setattr(torch.Tensor, name, g._wrap(real, name in NEW_FILLED))
        yield g
    finally:
        for name in _REAL_NEW:
            if name in vars(torch.Tensor):      # (the methods live on the base class: dropping the override restores them)
                delattr(torch.Tensor, name)
        for m in patched:
            m.torch = torch
        for c, saved in caches:
            c.clear()
            c.update(saved)
        _reset_packs(modules)
