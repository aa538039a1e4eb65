"""The buffer contract (tests/buffer_contract.py) for the entry points of include/sgcdet_amd_level_train.h: every output and workspace
pre-filled with NaN and with a large finite value, every input inside NaN guards -- each case of tests/buffer_cases_level_train.py
writes all of its output (the zero padding columns of grad_proj included), nothing beyond it, and the same bits under both fills."""
import pytest

from buffer_cases_level_train import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_output_element_is_written_and_nothing_beyond(case, gpu_ops):
    from buffer_contract import run_case
    run_case(case, gpu_ops, "cuda", ref_ops=None)
