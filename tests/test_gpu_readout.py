"""The kernels that read results out of the trees (stan4bart_amd/csrc/dev_hip.hip) on the device, at the shapes that select their branches:
  * k_predict — predict() of every kept draw at new rows, live and stored samplers: one thread per (row, draw), at most 4096 workgroups of 256, so the
    grid-stride loop and its idx / nT split only run beyond 1 048 576 elements; the response scale of the DRAW;
  * k_test_fits_few (up to 65 536 test rows and 4 * T * 8 <= 48 KiB of LDS: 4 rows per workgroup, a lane walks more than one tree for T > 64, the loop
    with its two barriers goes round beyond 8 192 rows) and k_test_fits (beyond either limit; grid-stride beyond 524 288 rows);
  * k_var_counts, k_draw_k — one workgroup, loops of stride 256 over predictors and trees.
Every case names its branch, builds the shape that selects it, asserts from the branch functions of tests/readout_cases.py (constants READ from
dev_hip.hip) that it was selected, and compares with a vectorised numpy walk of the flattened trees over the RAW rows — a reference that shares no code
with the kernels or the host's binning — within 4 x the bound DERIVED in readout_cases.py; two device results formed by the same arithmetic in the same
order (live / stored sampler; bart.test / predict_bart of the same rows) must be EQUAL.  The test rows are not training rows: rows exactly on the cut
values of the chain's own rules, one double above and below them, at +-inf, +-1e300, far outside the training range, plus uniform draws.
The cases, the reference and the checks are shared with the CPU twin tests/test_readout.py (the same data over the emulated device layer).
Every case prints which kernel / branch it was for and the largest |device - reference| / bound it saw (profiles/readout_gpu.txt)."""
import numpy as np
import pytest

import readout_cases as rc

pytestmark = pytest.mark.gpu


def _report(line):
    print(line)


@pytest.mark.parametrize("name", sorted(rc.PREDICT_CASES))
def test_predictions(hip_lib, name):
    rc.assert_prediction_case(name, rc.check_prediction(hip_lib, "s4b_", name, _report))


def test_per_draw_scale(hip_lib):
    rc.check_per_draw_scale(hip_lib, "s4b_", _report)


@pytest.mark.parametrize("name", sorted(rc.TEST_FIT_CASES))
def test_test_row_fits(oracle_lib, hip_lib, name):
    rc.check_test_fits(hip_lib, "s4b_", oracle_lib, name, _report)


@pytest.mark.parametrize("name", sorted(rc.COUNT_CASES))
def test_var_counts_and_k(oracle_lib, hip_lib, name):
    r = rc.check_counts(hip_lib, "s4b_", oracle_lib, name, _report)
    if name == "predictors-299":
        assert np.flatnonzero(r["varcount"].sum(axis=1)).max() >= 256          # rules on predictors beyond the first round of the clearing loop were accepted


def test_more_predictors_than_a_rule_can_name_are_refused(hip_lib):
    rc.check_predictor_limit(hip_lib, "s4b_")
