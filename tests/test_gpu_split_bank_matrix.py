"""Every instantiation of k_conv_split32 the product ships, and every K loop inside it, bit for bit.

The product library holds the kernel for NT = 1..5 n-tiles per workgroup x {three bfloat16 parts, two binary16 parts} x {uniform bank,
size group of a mixed bank} (tests/test_kernel_census.py), each with one hand-scheduled K loop per MV = 1..4 M-tiles of a wavefront.  The
banks of tests/exact_bank_cases.py MATRIX_BANKS / MATRIX_MIXED and the two small frames MATRIX_FRAMES reach all 80 loops, both parities
of the filter ring on odd NT (an even tap count leaves through the loop's condition, an odd one through its break), every remainder launch
behind a full group of five, a second group, and loops of one and two taps — tests/test_split_bank_matrix_cpu.py proves that from the
launchers' arithmetic.  Families A1-A3 (five placement rounds each) and B2 on both split banks, each with its own kind of operands;
np.array_equal on values against the float64 correlation, every plane of every level, no tolerance."""
import pytest

from tests import exact_bank_cases as X
from tests.test_gpu_exact_banks import run_bank

pytestmark = pytest.mark.gpu
FAMILIES = ("A1", "A2", "A3", "B2")
SPLIT_BANKS = ["bf16x6", "f16x3"]        # test_gpu_exact_banks.BANKS: PBD_CONV_SPLIT on kind "f32", PBD_CONV_SPLIT_F16 on kind "f16"


@pytest.mark.parametrize("bank", SPLIT_BANKS)
@pytest.mark.parametrize("nf,kh,kw", X.MATRIX_BANKS)
def test_uniform_banks(gpu_required, bank, nf, kh, kw):
    diff = run_bank(bank, [(kh, kw)] * nf, only=FAMILIES, frames=X.MATRIX_FRAMES)
    assert diff is None, diff


@pytest.mark.parametrize("bank", SPLIT_BANKS)
def test_mixed_bank(gpu_required, bank):
    """pbd_create_sized, groups of 65 / 97 / 161 / 16 / 33 filters in a shuffled caller's order: NT = 3, 4, 5 and a remainder of 1, 1 on an
    even tap count, 2 on one tap"""
    diff = run_bank(bank, X.matrix_mixed_sizes(), only=FAMILIES, frames=X.MATRIX_FRAMES)
    assert diff is None, diff
