"""The fused head of the pair track against the three launches it fuses, bit for bit, on the GPU in split-16 arithmetic (the fused
head exists only there).

pair_head_h2_kernel calls the row-stage functions of csrc/prd_pair.hip -- rbf_rowgemm, pair_init_finish, product_rowgemm, opm_finish,
bias_heads -- that pair_init_kernel<P, true>, opm_pair_kernel<P, true> and pair_bias_kernel call, in the same order, on the same
operands, and the row is rounded to fp32 between the stages in either form.  So ops.pair_head(...) must EQUAL
ops.pair_init -> ops.opm_pair(residual=True) -> ops.pair_bias2 in all three outputs, not merely agree within a tolerance.

Shapes, the smallest at which the task decode of the fused head (a task = one row i and 32 columns j) and that of the separate
kernels (32 consecutive positions) differ in every way they can: b = 2; N = 33 (a 32-block and a block of one column) and 70 (two
blocks and a partial one; the flat tasks of the separate kernels straddle rows and the batch boundary); pair_dim 32 and 64;
dist_dim = C = 128; the last three positions of the second sample masked; the OPM mask applied and not; one bias-head set with the
LayerNorm affine pair and one without, of 1 and 8 heads."""
import math

import pytest
import torch

from protein_redesign_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, DK, C, HA, HB = 2, 128, 128, 1, 8


@pytest.fixture(autouse=True)
def split16():
    prev = _lib.lib().prd_get_gemm_mode()
    assert _lib.lib().prd_set_gemm_mode(1) == 0
    yield
    assert _lib.lib().prd_set_gemm_mode(prev) == 0


def head_inputs(N, P, seed):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().to(DEV).contiguous()

    mask = torch.ones(B, N)
    mask[B - 1, N - 3:] = 0
    a = dict(sp=rnd(B, N, N, P), z=rnd(B, N, 3, scale=3.0), mask=mask.to(DEV), centers=torch.linspace(0, 2, DK).to(DEV),
             w_dist=rnd(P, DK, scale=1 / math.sqrt(DK)), eb=rnd(B, P), ab=rnd(B, N, 2 * C), w_out=rnd(P, C, scale=1 / math.sqrt(C)),
             b_out=rnd(P, scale=0.3))
    # (w, bvec, gamma, beta): set a with the LayerNorm affine pair, set b without
    a["set_a"] = (rnd(HA, P, scale=1 / math.sqrt(P)), rnd(HA, scale=0.3), 1 + rnd(P, scale=0.1), rnd(P, scale=0.1))
    a["set_b"] = (rnd(HB, P, scale=1 / math.sqrt(P)), rnd(HB, scale=0.3), None, None)
    return a


@pytest.mark.parametrize("apply_mask", [False, True])
@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("N", [33, 70])
def test_fused_head_equals_its_three_launches_bit_for_bit(N, P, apply_mask):
    assert ops.pair_head_supported(P, DK, C)
    a = head_inputs(N, P, 1000 * N + P)
    want = ops.pair_init(a["sp"], a["z"], a["mask"], a["centers"], a["w_dist"], a["eb"])
    want = ops.opm_pair(want, a["ab"], a["mask"], a["w_out"], a["b_out"], residual=True, apply_mask=apply_mask)
    want_a, want_b = ops.pair_bias2(want, a["set_a"], a["set_b"])
    got = ops.pair_head(a["sp"], a["z"], a["mask"], a["centers"], a["w_dist"], a["eb"], a["ab"], a["w_out"], a["b_out"],
                        apply_mask=apply_mask, set_a=a["set_a"], set_b=a["set_b"])
    torch.cuda.synchronize()
    for name, x, y in zip(("pair", "bias_a", "bias_b"), got, (want, want_a, want_b)):
        assert torch.isfinite(y).all(), name
        print(f"N {N} P {P} apply_mask {apply_mask} {name}: largest element difference {float((x - y).abs().max()):.3e}")
        assert torch.equal(x, y), name
