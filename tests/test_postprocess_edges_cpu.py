"""tests/postprocess_edge_contract.py on the CPU oracle: the decision edges of aligned NMS, rotated IoU / NMS and target
assignment are decidable by their references alone -- the oracle meets every one of them, so a miss of the HIP library in
tests/test_gpu_postprocess_edges.py is the library's."""
import pytest

import postprocess_edge_contract as pc


@pytest.mark.parametrize("n", pc.BLOCK_SIZES + (4095, 4096))
def test_aligned_nms_block_edges(n, oracle_ops):
    pc.check_aligned_sizes(oracle_ops, "cpu", n)


def test_aligned_nms_identical_boxes(oracle_ops):
    pc.check_aligned_identical(oracle_ops, "cpu")


def test_aligned_nms_iou_exactly_at_the_threshold(oracle_ops):
    pc.check_aligned_exact_threshold(oracle_ops, "cpu")


def test_aligned_nms_zero_volume_boxes(oracle_ops):
    pc.check_aligned_zero_volume(oracle_ops, "cpu")


@pytest.mark.parametrize("n,all_equal", [(200, False), (129, True)], ids=["quarter_equal", "all_equal"])
def test_aligned_nms_tied_scores(n, all_equal, oracle_ops):
    pc.check_aligned_ties(oracle_ops, "cpu", n, all_equal)


def test_aligned_nms_dirty_workspace(oracle_ops):
    pc.check_aligned_dirty_workspace(oracle_ops, "cpu")


def test_box_iou_rotated_on_touching_pairs(oracle_ops):
    pc.check_iou_touching(oracle_ops, "cpu")


@pytest.mark.parametrize("name", pc.ROTATED_CASES)
def test_nms_rotated_decision_edges(name, oracle_ops):
    pc.check_rotated_case(oracle_ops, "cpu", name)


def test_nms_rotated_max_num_cut_with_ties(oracle_ops):
    pc.check_max_num_cut(oracle_ops, "cpu")


def test_nms_rotated_dirty_workspace(oracle_ops):
    pc.check_rotated_dirty_workspace(oracle_ops, "cpu")


def test_targets_fixture_is_not_vacuous():
    pc.check_targets_fixture_is_not_vacuous()


@pytest.mark.parametrize("name", pc.target_case_names())
def test_assign_targets_edges(name, oracle_ops):
    pc.check_target_case(oracle_ops, "cpu", name)
