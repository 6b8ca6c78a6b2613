"""Run by tests/test_ab_build.py in a child process with PRD_LIB = libprd_hip_ab.so: the superseded forms of the second-generation attention
cores that only the A/B library carries -- key-loop forms 1-3 and the round-3 phase 1 of the short-row core, the round-3 phase 1 and the
next-row prefetch of the long-row core -- against the default form (same arithmetic, other summation orders: < 2e-6); and the two
contraction forms of the triangle multiplication that only this library carries (16 waves, three chunks in flight), against float64 and
bit for bit against the default form."""
import sys

import torch

from protein_redesign_amd import _lib, ops

lib = _lib.lib()
assert lib.prd_set_gemm_mode(1) == 0
tune0 = lib.prd_get_tune()
H, c, P = 4, 16, 64
worst = 0.0
for N, arms in ((320, {"NO_GV": 1 << 21, "KL1": (1 << 21) | (1 << 6) | (2 << 7), "KL2": (1 << 21) | (1 << 6) | (4 << 7), "KL3": (1 << 21) | (1 << 6) | (6 << 7),
                       "prio+remap": (1 << 6) | (17 << 7)}),
                (449, {"NO_GV": 1 << 21, "prefetch": (1 << 6) | (9 << 7)})):
    g = torch.Generator().manual_seed(N)
    pair = torch.randn(1, N, N, P, generator=g).cuda()
    mask = torch.ones(1, N).cuda()
    mask[0, N - 11:] = 0
    wts = [(torch.randn(64, P, generator=g) / 8).cuda() for _ in range(4)] + [torch.zeros(64).cuda()]
    for ending in (False, True):
        lib.prd_set_tune(tune0)
        ref = ops.tri_attn_core_v2(pair, mask, wts, H, c, ending=ending).clone()
        for name, bits in arms.items():
            lib.prd_set_tune(tune0 | bits)
            got = ops.tri_attn_core_v2(pair, mask, wts, H, c, ending=ending)
            err = float((got - ref).norm() / ref.norm())
            worst = max(worst, err)
            assert torch.isfinite(got).all() and err < 2e-6, (N, ending, name, err)
lib.prd_set_tune(tune0)

# the contraction forms of the triangle multiplication that only this library carries: 16 waves (PRD_TUNE_TMS_NW16) and three chunks of
# operands in flight (PRD_TUNE_TMS_DEPTH3), called directly as test_triangle_multiplication_contraction_direct calls the 12-wave form --
# against float64 (split operands: 22 bits) and BIT FOR BIT against the default form: the K order of an output element does not depend
# on how the sub-tiles are dealt or on how many chunks are in flight.  (64, 1, 200): ragged tiles; (32, 1, 449): nine tiles per channel.
worst64 = 0.0
for P, b, N in ((64, 1, 200), (32, 1, 449)):
    g = torch.Generator().manual_seed(1000 + N + b)
    ldn = (N + 31) // 32 * 32
    ab = torch.zeros(b, 2 * P, N, ldn)
    ab[..., :N] = torch.randn(b, 2 * P, N, N, generator=g)
    want = torch.einsum("bpmk,bpnk->bpmn", ab[:, :P, :, :N].double(), ab[:, P:, :, :N].double())
    dab = ab.cuda()
    outs = {}
    for name, bits in (("default", 0), ("TMS_NW16", _lib._TUNE["TMS_NW16"]), ("TMS_DEPTH3", _lib._TUNE["TMS_DEPTH3"])):
        lib.prd_set_tune(tune0 | bits)
        o = torch.full((b, P, N, ldn), float("nan"), device="cuda")
        _lib.check(lib.prd_tri_mul_contract(_lib.dptr(o), _lib.dptr(dab), b, N, P, _lib.stream()), "prd_tri_mul_contract")
        outs[name] = o[..., :N].cpu()
        lib.prd_set_tune(tune0)
        err = float((outs[name].double() - want).norm() / want.norm())
        worst64 = max(worst64, err)
        assert torch.isfinite(outs[name]).all() and err < 2e-6, (P, b, N, name, err)
        assert torch.equal(outs[name], outs["default"]), (P, b, N, name, "differs from the default form")
lib.prd_set_tune(tune0)
print(f"ab contraction forms ok, worst rel-L2 vs float64 {worst64:.2e}")
print(f"ab forms ok, worst rel-L2 vs the default form {worst:.2e}")
sys.exit(0)
