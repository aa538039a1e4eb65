"""The HIP kernels that decide -- ``sgc_aligned_nms3d``, ``sgc_nms_rotated_bev``, ``sgc_box_iou_rotated``,
``sgc_assign_targets`` -- on their decision edges (tests/postprocess_edge_contract.py): 64-row block edges of both sweeps,
empty and single-candidate classes next to full ones, a full 64 x 64 pair list, the disjointness pre-test on pairs within
+-0.3 % of touching, tied scores, zero-volume boxes, an IoU exactly at the threshold, ties at the selected centerness rank,
duplicate ground-truth boxes.  Every check is an equality; tests/test_postprocess_edges_cpu.py runs the same checks on the
oracle."""
import pytest

import postprocess_edge_contract as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", pc.BLOCK_SIZES + (4095, 4096))
def test_aligned_nms_block_edges(n, gpu_ops):
    pc.check_aligned_sizes(gpu_ops, "cuda", n)


def test_aligned_nms_identical_boxes(gpu_ops):
    pc.check_aligned_identical(gpu_ops, "cuda")


def test_aligned_nms_iou_exactly_at_the_threshold(gpu_ops):
    pc.check_aligned_exact_threshold(gpu_ops, "cuda")


def test_aligned_nms_zero_volume_boxes(gpu_ops):
    pc.check_aligned_zero_volume(gpu_ops, "cuda")


@pytest.mark.parametrize("n,all_equal", [(200, False), (129, True)], ids=["quarter_equal", "all_equal"])
def test_aligned_nms_tied_scores(n, all_equal, gpu_ops):
    pc.check_aligned_ties(gpu_ops, "cuda", n, all_equal)


def test_aligned_nms_dirty_workspace(gpu_ops):
    pc.check_aligned_dirty_workspace(gpu_ops, "cuda")


def test_box_iou_rotated_on_touching_pairs(gpu_ops):
    pc.check_iou_touching(gpu_ops, "cuda")


@pytest.mark.parametrize("name", pc.ROTATED_CASES)
def test_nms_rotated_decision_edges(name, gpu_ops):
    pc.check_rotated_case(gpu_ops, "cuda", name)


def test_nms_rotated_max_num_cut_with_ties(gpu_ops):
    pc.check_max_num_cut(gpu_ops, "cuda")


def test_nms_rotated_dirty_workspace(gpu_ops):
    pc.check_rotated_dirty_workspace(gpu_ops, "cuda")


@pytest.mark.parametrize("name", pc.target_case_names())
def test_assign_targets_edges(name, gpu_ops):
    pc.check_target_case(gpu_ops, "cuda", name)


@pytest.mark.parametrize("name", pc.target_case_names())
def test_assign_targets_edges_equal_the_oracle(name, gpu_ops, oracle_ops):
    pc.check_target_case_against_oracle(gpu_ops, oracle_ops, "cuda", name)
