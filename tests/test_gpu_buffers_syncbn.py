"""The buffer contract (tests/buffer_contract.py) for the entry points of include/sgcdet_amd_syncbn.h: every output and workspace
pre-filled with NaN and with a large finite value, every input inside NaN guards -- each case of tests/buffer_cases_syncbn.py writes
all of its outputs (the packed statistics with their count, the sums, the device scalar 1 / N), nothing beyond them, and the same bits
under both fills.  No case restricts an extent: the header declares every output fully written."""
import pytest

from buffer_cases_syncbn import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_output_element_is_written_and_nothing_beyond(case, gpu_ops):
    from buffer_contract import run_case
    run_case(case, gpu_ops, "cuda", ref_ops=None)
