"""Pins the oracle (C kernels + oracle/ref_path.py restatement) to the golden vectors made
by the REFERENCE's own Python modules (tests/golden/make_golden.py).  CPU only."""
import pytest
import torch

from golden_util import load, img_meta, depth_pyramid, max_err
from oracle.ref_path import RefPath


def test_reference_autograd_composition(oracle_ops):
    """MultiScale3DDeformableAttnFunction_fp32 (two ext calls + python grad merge) == fused oracle."""
    d, _ = load("op_autograd")
    out, score = oracle_ops.dfa3d_forward(d["value"], d["dist"], d["shapes3"], d["lsi"], d["loc"], d["attn"], want_score=True)
    assert torch.equal(out, d["out"]) and torch.equal(score, d["score"])
    gv, gd, gl, ga = oracle_ops.dfa3d_backward(d["value"], d["dist"], d["shapes3"], d["lsi"], d["loc"], d["attn"], d["grad_out"])
    assert max_err(gv, d["grad_value"]) < 1e-6 and max_err(gd, d["grad_dist"]) < 1e-5
    assert max_err(gl, d["grad_loc"]) < 1e-4 and max_err(ga, d["grad_attn"]) < 1e-6


def _voxel_cfg(d, C=32):
    return dict(embed_dims=C, n_voxels_list=[tuple(int(v) for v in g) for g in d["grids"]],
                voxel_size_list=[tuple(float(v) for v in s) for s in d["sizes"]],
                topk_list=[int(v) for v in d["topk"]], dbound=(0.2, 5.0), num_heads=8, num_points=4)


def test_point_sampling_matches_reference_torch(oracle_ops):
    """VoxFormerEncoder_DFA3D.point_sampling run by the reference on torch-CPU vs the oracle's
    fixed-order projection: mask identical, coordinates within fp32 rounding."""
    d, _ = load("point_sampling")
    meta = img_meta(d)
    rp = RefPath({}, dict(dbound=(float(d["dbound"][0]), float(d["dbound"][1]))))
    ref_cam, mask = rp.project(d["ref_3d"].float(), meta)
    g_cam = d["ref_cam"][:, 0, :, 0]
    g_mask = d["mask"][:, 0, :, 0]
    assert torch.equal(mask, g_mask)
    assert 0.1 < g_mask.float().mean() < 0.9
    assert max_err(ref_cam, g_cam) < 2e-6


def test_point_sampling_near_plane_rule_matches_reference_torch(oracle_ops):
    """Cameras inside the grid (tests/golden/make_golden_near.py): 48 in-image voxels lie 0 .. 0.2 m in front of a
    camera.  The reference drops them -- its depth test runs on the slice it has just overwritten with the
    normalised depth (encoder.py:203-213) -- and so must the oracle: mask identical, and none of the band's points
    visible."""
    d, _ = load("point_sampling_near")
    meta = img_meta(d)
    rp = RefPath({}, dict(dbound=(float(d["dbound"][0]), float(d["dbound"][1]))))
    ref_cam, mask = rp.project(d["ref_3d"].float(), meta)
    g_cam, g_mask = d["ref_cam"][:, 0, :, 0], d["mask"][:, 0, :, 0]
    assert int(d["n_band"]) >= 8
    assert torch.equal(mask, g_mask)
    u, v, zn = g_cam[..., 0], g_cam[..., 1], g_cam[..., 2]
    inside = (u > 1e-5) & (u < 1 - 1e-5) & (v > 1e-5) & (v < 1 - 1e-5)
    band = inside & (zn <= 1e-5) & (zn > -0.2 / 4.8 + 1e-4)          # in front of the camera, closer than d_near
    assert int(band.sum()) >= 8 and not g_mask[band].any()
    # u, v of points almost in the camera plane are huge (division by ~1 cm): compare where the mask can be 1
    assert max_err(ref_cam[inside], g_cam[inside]) < 2e-6


def test_voxel_head_restatement_matches_reference():
    d, sd = load("voxel_head")
    meta = img_meta(d)
    rp = RefPath(sd, _voxel_cfg(d))
    feats = [d[f"feat{i}"] for i in range(4)]
    dpts = depth_pyramid(d["dpt"])
    lvl0, _ = rp.dense_head(0, feats[2][:, :, :, :59 // 16, :80 // 16], dpts[2][:, :, :, :59 // 16, :80 // 16], meta)
    assert max_err(lvl0, d["level0_volume"]) < 2e-5
    volume, valid, occ = rp.adaptive_sparse_head(feats, meta, dpts)
    assert torch.equal(valid, d["valid"])                       # top-k voxel sets: bit-exact
    assert max_err(occ, d["occ"]) < 1e-5
    assert max_err(volume, d["volume"]) < 5e-5


def test_neck_restatement_matches_reference():
    d, sd = load("neck")
    outs = RefPath(sd, {}).neck(d["x"])
    for i, o in enumerate(outs):
        assert o.shape == d[f"out{i}"].shape
        assert max_err(o, d[f"out{i}"]) < 1e-4 * max(1.0, d[f"out{i}"].abs().max().item())


@pytest.mark.parametrize("tag,n_cls", [("scannet", 18), ("sunrgbd", 17)])
def test_head_restatement_matches_reference(tag, n_cls):
    d, sd = load("head_" + tag)
    rp = RefPath(sd, dict(head=tag, n_classes=n_cls, nms_pre=int(d["nms_pre"])))
    ctr, reg, cls = rp.head([d["f0"], d["f1"], d["f2"]])
    for i in range(3):
        assert max_err(ctr[i], d[f"ctr{i}"]) < 1e-5 and max_err(cls[i], d[f"cls{i}"]) < 1e-5
        assert max_err(reg[i], d[f"reg{i}"]) < 1e-5 * max(1.0, d[f"reg{i}"].abs().max().item())
    boxes, scores = rp.decode(ctr, reg, cls, d["valid"], img_meta(d), tuple(float(v) for v in d["voxel_size"]))
    assert boxes.shape == d["boxes"].shape
    assert max_err(scores, d["scores"]) < 1e-6
    assert max_err(boxes, d["boxes"]) < 1e-4


def test_oracle_nms_reproduces_reference_aligned_3d_nms(oracle_ops):
    """tests/golden/nms_aligned.npz: kept indices of the reference's own aligned_3d_nms (make_golden_nms.py),
    including zero-volume / inverted boxes (NaN IoU) -- the oracle follows the same loop, bit-exact indices."""
    import numpy as np
    import os
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "nms_aligned.npz"))
    for k in range(int(d["n_cases"])):
        boxes, scores, labels = (torch.from_numpy(d[f"{n}{k}"]) for n in ("boxes", "scores", "labels"))
        keep = oracle_ops.aligned_nms3d(boxes, scores, labels, float(d[f"thr{k}"]))
        assert torch.equal(keep, torch.from_numpy(d[f"keep{k}"])), k
    assert oracle_ops.aligned_nms3d(torch.zeros(0, 6), torch.zeros(0), torch.zeros(0, dtype=torch.int64), 0.25).numel() == 0


def _plane_sweep_case(d, k):
    f_mvs = torch.from_numpy(d[f"f_mvs{k}"])
    N, C, H, W = f_mvs.shape
    rows = f_mvs.permute(0, 2, 3, 1).reshape(N, H * W, C).contiguous()
    rel = torch.from_numpy(d[f"rel{k}"])
    nbr = torch.from_numpy(d[f"nbr{k}"]).to(torch.int32).contiguous()
    return f_mvs, rows, nbr, rel.reshape(N, rel.shape[1], 12).contiguous(), torch.from_numpy(d[f"depth{k}"]), (H, W)


def test_oracle_rotated_nms_reproduces_reference_multiclass_glue(oracle_ops):
    from nms_rotated_contract import check_multiclass_golden
    check_multiclass_golden(oracle_ops, "cpu")


def test_oracle_rotated_iou_matches_float64_polygon_clip(oracle_ops):
    from nms_rotated_contract import check_iou_against_float64_clip, check_mask_sweep_equals_textbook_loop
    check_iou_against_float64_clip(oracle_ops, "cpu")
    check_mask_sweep_equals_textbook_loop(oracle_ops, "cpu")


def test_oracle_target_assignment_reproduces_reference_get_targets(oracle_ops):
    from targets_contract import check_targets_golden
    check_targets_golden(oracle_ops, "cpu")


def test_oracle_plane_sweep_reproduces_reference_cost_volume(oracle_ops):
    """tests/golden/plane_sweep.npz: correlation volume of the reference's own homo_warping + cost-volume loop
    (make_golden_planesweep.py) -- the oracle never builds the warped features and agrees to 1e-5."""
    import numpy as np
    import os
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "plane_sweep.npz"))
    for k in range(int(d["n_cases"])):
        f_mvs, rows, nbr, rt, depth, (H, W) = _plane_sweep_case(d, k)
        corr = oracle_ops.plane_sweep_corr(rows, nbr, rt, depth, H, W)
        want = torch.from_numpy(d[f"corr{k}"])
        assert corr.shape == want.shape
        assert float((corr - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max())), k


def test_plane_sweep_host_glue_matches_reference_neighbours_and_projections():
    """closest_frame_ids / relative_projections (product host code) == the reference's get_closest_frame_ids /
    collect_proj + homo_warping's matmul-inverse, from the golden fixture."""
    import numpy as np
    import os
    from sgcdet_amd.plugin.plane_sweep import closest_frame_ids, relative_projections
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "plane_sweep.npz"))
    for k in range(int(d["n_cases"])):
        nbr = torch.from_numpy(d[f"nbr{k}"])
        assert torch.equal(closest_frame_ids(nbr.shape[0], nbr.shape[1]), nbr)
        rel = relative_projections(torch.from_numpy(d[f"w2c{k}"]), torch.from_numpy(d[f"intr{k}"]), nbr)
        assert float((rel - torch.from_numpy(d[f"rel{k}"])).abs().max()) < 1e-4


def test_rotated_iou_restatement_matches_the_references_own_header(oracle_ops):
    """oracle sgc_box_iou_rotated vs tests/golden/box_iou_rotated.npz, made by the REFERENCE's own
    box_iou_rotated_utils.hpp (compiled from /root/reference into oracle/_ref, tests/golden/make_golden_iou.py) --
    its ``__CUDACC__`` branch, the one the reference's GPU NMS runs.  The restatement keeps the header's fp32 operation
    order: equal to 1e-6 (bit-equal on most pairs).  (The header's std::sort branch, ``iou_cpu_branch``, is off by
    0.026 on one pair of this fixture against both the CUDA branch and an exact polygon clip; it is not the yardstick.)"""
    d, _ = load("box_iou_rotated")
    got = oracle_ops.box_iou_rotated(d["a"], d["b"])
    assert got.shape == d["iou"].shape
    assert max_err(got, d["iou"]) <= 1e-6
    assert float((got == d["iou"]).float().mean()) > 0.95
    assert (d["iou"] > 0.05).float().mean() > 0.1          # the fixture really overlaps


def test_rotated_iou_against_live_reference_build_when_present(oracle_ops):
    """Seeded random boxes through the reference's header and through the oracle.  Where oracle/_ref has been built (it
    needs the reference tree) the header runs live and must reproduce its recorded result
    (tests/golden/box_iou_rotated_self.npz, tests/golden/make_golden_iou_self.py); elsewhere the recorded result is the
    yardstick."""
    import numpy as np
    import oracle
    rng = np.random.RandomState(5)
    a = np.concatenate([rng.uniform(-1, 1, (64, 2)), rng.uniform(0.1, 1.5, (64, 2)), rng.uniform(-4, 4, (64, 1))], 1).astype(np.float32)
    d, _ = load("box_iou_rotated_self")
    assert np.array_equal(d["a"].numpy(), a)
    ref = oracle.ref_box_iou_rotated(a, a, variant="cuda")
    if ref is not None:
        assert max_err(torch.from_numpy(ref), d["iou"]) <= 1e-6
    ref = torch.from_numpy(ref) if ref is not None else d["iou"]
    got = oracle_ops.box_iou_rotated(torch.from_numpy(a), torch.from_numpy(a))
    assert max_err(got, ref) <= 1e-6
