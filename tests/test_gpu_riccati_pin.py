"""GPU: the pin of the Riccati backward sweep (tests/_rictwin.py: cases, long-double reference, check()) on the device, through
hb_riccati_gains, with hb_config.reserved = RIC_BWD_ONE (k_ric_bwd), RIC_BWD_FOUR (k_ric_bwd4) and 0 (the product's choice).

  * each form through check(): structure exact, forward and backward error of K~, k~ per stage within 8 x the float64 family's distance;
  * the three forms give identical K~, k~, ric_fail;
  * neighbour independence: with the failing cases 8 and 9 replaced by copies of case 0, every other instance's gains stay bit-identical;
  * position independence: case 3 alone in a call of one instance equals its rows in the batch bit for bit.
One context per form, three launches of at most 12 x 24 stages each."""
import numpy as np
import pytest

import _rictwin as tw
from hunter_bipedal_control_amd import abi

pytestmark = pytest.mark.gpu

FORMS = {"one wavefront": abi.FORM.RIC_BWD_ONE, "four wavefronts": abi.FORM.RIC_BWD_FOUR, "automatic": 0}
SWAPPED = tuple(0 if i in tw.FLAG_CASES else i for i in range(tw.NCASES))


@pytest.fixture(scope="module")
def device(params):
    """per form: the batch of twelve, the batch with cases 8 and 9 swapped for case 0, and case 3 alone"""
    from hunter_bipedal_control_amd.solver import HunterSolver
    assert int(tw.SENTINEL_BITS) == abi.RIC_GAINS_SENTINEL_BITS
    out = {}
    for name, code in FORMS.items():
        s = HunterSolver(params, batch=tw.B, max_nodes=tw.NMAX, reserved=code)
        try:
            out[name] = dict(batch=s.riccati_gains(*tw.arrays()), swapped=s.riccati_gains(*tw.arrays(SWAPPED)), alone=s.riccati_gains(*tw.arrays((3,))))
        finally:
            s.close()
    return out


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("form", list(FORMS))
def test_device_sweep_meets_every_check_on_all_twelve_cases(device, form):
    ratios = tw.check(*device[form]["batch"], form)
    print(f"{form}: worst ratio per case:", " ".join(f"{v:.2f}" for v in ratios.max(axis=1)))


def test_the_forms_give_identical_gains(device):
    K, k, fail = device["one wavefront"]["batch"]
    for form in ("four wavefronts", "automatic"):
        K2, k2, fail2 = device[form]["batch"]
        assert _same(K, K2) and _same(k, k2) and np.array_equal(fail, fail2), form


@pytest.mark.parametrize("form", list(FORMS))
def test_a_failed_neighbour_changes_nothing(device, form):
    (K, k, fail), (K2, k2, fail2) = device[form]["batch"], device[form]["swapped"]
    assert fail2.tolist() == [0] * tw.NCASES
    for i in range(tw.NCASES):
        j = SWAPPED[i]
        assert _same(K2[i], K[j]) and _same(k2[i], k[j]), f"{form}: instance {i} (case {j}) differs once cases 8 and 9 no longer fail next to it"


@pytest.mark.parametrize("form", list(FORMS))
def test_case_3_alone_equals_its_rows_in_the_batch(device, form):
    (K, k, fail), (K1, k1, fail1) = device[form]["batch"], device[form]["alone"]
    assert K1.shape[0] == 1 and _same(K1[0], K[3]) and _same(k1[0], k[3]) and fail1[0] == fail[3] == 0, form
