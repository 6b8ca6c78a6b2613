"""GPU: ops.rows_linear is ops.pair_linear where the row kernel serves the call (rows >= ops.WGRAD_MIN_ROWS = 8192) and the
written-out ops.linear call where it does not, bit for bit, in both arithmetics; ``fallback_arith`` reaches the fallback alone."""
import pytest
import torch

from protein_redesign_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = [8192, 8191]         # the row kernel's first row count (it serves split-16 only), and the last one of the GEMM fallback


@pytest.fixture(params=["fp32", "split16"])
def gemm_mode(request):
    prev = _lib.lib().prd_get_gemm_mode()
    assert _lib.lib().prd_set_gemm_mode(_lib.GEMM_MODES[request.param]) == 0
    yield request.param
    assert _lib.lib().prd_set_gemm_mode(prev) == 0


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("rows", ROWS)
def test_ln_relu_form(rows, gemm_mode):
    """K = 64 -> OUT = 256 with ln_in, xn_out, act=1 (the recompute of a LayerNorm-linear-ReLU); the LN rows are compared too."""
    x, w, b = randn(1, rows, 64) * 3 + 0.5, randn(2, 256, 64) / 8, randn(3, 256)
    xn, xn_want = torch.full_like(x, 1.0), torch.full_like(x, 2.0)
    got = ops.rows_linear(x, w, b, ln_in=True, xn_out=xn, act=1)
    want = ops.pair_linear(x, w, b, ln_in=True, xn_out=xn_want, act=1)
    assert (want is not None) == (rows == 8192 and gemm_mode == "split16")
    if want is None:
        want = ops.linear(x, w, b, act=1, ln_a=True, ln_a_out=xn_want)
    assert got.shape == (rows, 256)
    assert torch.equal(got, want)
    assert torch.equal(xn, xn_want)
    assert float(got.min()) == 0.0 and float(got.max()) > 0.0


@pytest.mark.parametrize("rows", ROWS)
def test_transposed_relu_mask_form(rows, gemm_mode):
    """K = 256 -> OUT = 64 with transposed=True and a relu_mask (an activation gradient through a stored [K, OUT] weight)."""
    x, w, m = randn(4, rows, 256), randn(5, 256, 64) / 16, randn(6, rows, 64)
    got = ops.rows_linear(x, w, transposed=True, relu_mask=m)
    want = ops.pair_linear(x, w.t(), relu_mask=m)
    assert (want is not None) == (rows == 8192 and gemm_mode == "split16")
    if want is None:
        want = ops.linear(x, w.t().contiguous(), relu_mask=m)
    assert got.shape == (rows, 64)
    assert torch.equal(got, want)
    assert bool((got[m <= 0] == 0).all()) and bool((got[m > 0] != 0).any())


@pytest.mark.parametrize("rows", ROWS)
def test_fallback_arith_pins_the_fallback_alone(rows):
    """Under split-16, fallback_arith=0: the GEMM fallback is ops.linear inside arithmetic(0); the row kernel's call is untouched; the
    arithmetic in force afterwards is split-16 again."""
    x, w, m = randn(7, rows, 256), randn(8, 256, 64) / 16, randn(9, rows, 64)
    with _lib.arithmetic("split16"):
        got = ops.rows_linear(x, w, transposed=True, relu_mask=m, fallback_arith=0)
        assert _lib.arith() == 1
        if rows == 8192:
            want = ops.pair_linear(x, w.t(), relu_mask=m)
        else:
            with _lib.arithmetic(0):
                want = ops.linear(x, w.t().contiguous(), relu_mask=m)
    assert want is not None
    assert torch.equal(got, want)
