"""Every documented filter size (include/pbd_c.h: kh, kw in 1..9), bit for bit, on every bank.

33 filters of each of the 81 sizes on the six banks of test_gpu_exact_banks.BANKS — the ordered fp32 / fp64 chains (k_conv_exact_generic,
k_conv_exact for 5 x 5), the fp32 / fp64 MFMA chains (k_conv_mfma16 with run-time tap loops), six bfloat16 products and three binary16
products (k_conv_split32) —, every family the bank runs elsewhere (A1-A3 in five placement rounds, B1-B3, AF on the double handles), on
one frame whose levels (11 x 11 down to 3 x 3 cells) are all smaller than a 16 x 16 unit: the halo of the large sizes is wider than the level.
This pins the anchor (kh / 2, kw / 2) of even sides, the border constant on every side and the tap loops from one tap to 81.
np.array_equal on values against the float64 correlation, no tolerance."""
import pytest

from tests import exact_bank_cases as X
from tests.test_gpu_exact_banks import BANKS, run_bank

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bank", list(BANKS))
@pytest.mark.parametrize("kh,kw", X.SWEEP_SIZES, ids=[f"{kh}x{kw}" for kh, kw in X.SWEEP_SIZES])
def test_every_size_on_every_bank(gpu_required, bank, kh, kw):
    diff = run_bank(bank, [(kh, kw)] * X.SWEEP_FILTERS, frames=[X.SWEEP_FRAME])
    assert diff is None, diff
