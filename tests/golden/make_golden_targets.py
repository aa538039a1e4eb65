#!/usr/bin/env python3
"""Generates tests/golden/head_targets.npz: outputs of the reference's own ``get_targets``
(/root/reference/mmdet3d_plugin/models/dense_heads/imvoxel_head_v2.py:361-435 ScanNetImVoxelHeadV2, :485-561
SunRgbdImVoxelHeadV2, ``get_points`` :237-247) on seeded ground-truth boxes, and of the vendored
``axis_aligned_bbox_overlaps_3d`` (packages/mmdetection3d/mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py)
that AxisAlignedIoULoss thresholds; and tests/golden/head_targets_edges.npz: the same ``get_targets`` on small grids where
its decisions are ties and edges (``edges`` below).  Build-container only; the stub machinery of make_golden.py is reused.  The
ground-truth container is a 10-line stand-in for mmdet3d's DepthInstance3DBoxes exposing what get_targets reads
(``volume``, ``gravity_center``, ``tensor``, ``device``, ``len``) with mmdet3d's definitions (bottom-centre z +
half height, w*l*h).  Nothing of the reference is copied: the fixture holds inputs and outputs."""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


class Boxes:
    """tensor [n,7] = (x, y, z_bottom, dx, dy, dz, yaw) as DepthInstance3DBoxes stores them"""

    def __init__(self, tensor):
        self.tensor = tensor

    def __len__(self):
        return self.tensor.shape[0]

    @property
    def device(self):
        return self.tensor.device

    @property
    def volume(self):
        return self.tensor[:, 3] * self.tensor[:, 4] * self.tensor[:, 5]

    @property
    def gravity_center(self):
        bc = self.tensor[:, :3]
        gc = torch.zeros_like(bc)
        gc[:, :2] = bc[:, :2]
        gc[:, 2] = bc[:, 2] + self.tensor[:, 5] * 0.5
        return gc


def scene_boxes(n, seed, with_yaw):
    g = torch.Generator().manual_seed(seed)
    ctr = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([5.0, 5.0, 1.0]) + torch.tensor([0.0, 0.0, 0.3])
    size = 0.25 + torch.rand(n, 3, generator=g) ** 2 * torch.tensor([2.5, 2.5, 1.6])
    if n >= 3:
        size[0] = torch.tensor([0.12, 0.12, 0.12])         # smaller than a voxel: may own no point at all
        ctr[1], size[1] = ctr[2] + 0.05, size[2] * 0.6       # nested boxes: minimal volume wins
    yaw = (torch.rand(n, 1, generator=g) - 0.5) * 6.0 if with_yaw else torch.zeros(n, 1)
    return torch.cat([ctr, size, yaw], dim=1).float()


# ---- head_targets_edges.npz: ties and edges --------------------------------------------------------------------------
# Voxel size 0.25 and origin (0, 0, 0.5): every point coordinate is exact in fp32, so points that mirror each other in a
# box centred on a grid point have EQUAL centerness -- ties at the selected rank -- and a face can lie exactly on points.
EDGE_VOXEL = (.25, .25, .25)
EDGE_ORIGIN = (0.0, 0.0, 0.5)
EDGE_GRIDS = ([(8, 8, 4), (4, 4, 2), (2, 2, 1)], [(6, 5, 3)])            # 292 points in 3 scales; 90 points, one scale
YAWS = (0.0, 0.3, float(np.pi / 2), -2.9)

SCENES = {   # rows: gravity centre, dims; labels
    # one box centred on a grid point: 75 / 9 / 0 points inside at the three scales, mirror images tie
    "sym": ([[0, 0, 0.5, 1.1, 1.1, 0.6]], [4]),
    # the same, not square: under a yaw only the point reflection through the centre stays an exact symmetry
    "symr": ([[0, 0, 0.5, 1.1, 0.9, 0.6]], [4]),
    # two duplicates with different labels, two crossing boxes of equal volume, a box smaller than a voxel that holds no
    # point, a box that holds every point
    "mixed": ([[-0.3, -0.2, 0.45, 0.7, 0.6, 0.6], [-0.3, -0.2, 0.45, 0.7, 0.6, 0.6],
               [0.35, 0.3, 0.5, 0.8, 0.4, 0.7], [0.35, 0.3, 0.5, 0.4, 0.8, 0.7],
               [0.1, 0.1, 0.6, 0.05, 0.05, 0.05], [0, 0, 0.5, 10, 10, 10]], [3, 7, 1, 2, 5, 9]),
    # the same make-up off the grid, for the rotated head: no point within 1e-4 of a face under any of YAWS
    "mixedr": ([[-0.31, -0.17, 0.47, 0.73, 0.61, 0.57], [-0.31, -0.17, 0.47, 0.73, 0.61, 0.57],
                [0.33, 0.3, 0.52, 0.83, 0.43, 0.71], [0.33, 0.3, 0.52, 0.43, 0.83, 0.71],
                [0.11, 0.13, 0.61, 0.05, 0.05, 0.05], [0, 0, 0.5, 10, 10, 10]], [3, 7, 1, 2, 5, 9]),
    # faces at x, y = +-0.5 and z = 0.25, 0.75: exactly on grid points, which `> 0` counts outside
    "face": ([[0, 0, 0.5, 1.0, 1.0, 0.5]], [6]),
}

EDGE_CASES = (      # name, scene, grid, limit, centerness_topk   (axis-aligned head)
    [(f"sym_topk{k}", "sym", 0, 27, k) for k in (0, 1, 3, 7, 18, 100)]
    + [(f"sym_limit{l}", "sym", 0, l, 18) for l in (1, 5, 1000)]
    + [("mixed", "mixed", 0, 27, 18), ("mixed_topk3", "mixed", 0, 27, 3), ("mixed_limit1", "mixed", 0, 1, 18),
       ("mixed_limit1000", "mixed", 0, 1000, 18), ("face", "face", 0, 27, 18), ("face_topk100", "face", 0, 27, 100),
       ("one_scale_sym", "sym", 1, 27, 18), ("one_scale_sym_topk3", "sym", 1, 27, 3), ("one_scale_mixed", "mixed", 1, 27, 18)])
ROTATED_CASES = [   # the same scenes under every yaw; `face` is left to the axis-aligned head: see face_margin
    (f"{name}_yaw{yi}", scene, grid, limit, topk, yaw)
    for name, scene, grid, limit, topk in (("symr", "symr", 0, 27, 18), ("symr_topk3", "symr", 0, 27, 3), ("mixed", "mixedr", 0, 27, 18),
                                           ("mixed_limit1", "mixedr", 0, 1, 18), ("one_scale_symr", "symr", 1, 27, 18),
                                           ("one_scale_mixed", "mixedr", 1, 27, 18))
    for yi, yaw in enumerate(YAWS)]


def face_margin(points, boxes):
    """float64: the smallest distance of any point to any face plane of any box (yaw about z through the centre)"""
    p, b = points.double()[:, None, :], boxes.double()[None]
    s = p - b[..., :3]
    c, sn = torch.cos(-b[..., 6]), torch.sin(-b[..., 6])
    local = torch.stack((s[..., 0] * c - s[..., 1] * sn, s[..., 0] * sn + s[..., 1] * c, s[..., 2]), -1)
    return float((local.abs() - b[..., 3:6] / 2).abs().min())


def edges(head_mod):
    from npz_util import save_npz
    out = {}
    names = []
    grids = []
    probe = head_mod.ScanNetImVoxelHeadV2(n_classes=18, n_channels=8, n_reg_outs=6, n_scales=3, limit=27, centerness_topk=18)
    probe.voxel_size = EDGE_VOXEL
    for gi, sizes in enumerate(EDGE_GRIDS):
        pts = probe.get_points(sizes, EDGE_ORIGIN, torch.device("cpu"))
        grids.append(pts)
        out[f"g{gi}_points"] = torch.cat(pts).numpy()
        out[f"g{gi}_scales"] = torch.cat([torch.full((len(p),), i, dtype=torch.int32) for i, p in enumerate(pts)]).numpy()
        assert out[f"g{gi}_points"].dtype == np.float32
    assert len(out["g0_points"]) == 292 and len(out["g1_points"]) == 90
    todo = [(n, s, g, l, k, False, 0.0) for n, s, g, l, k in EDGE_CASES] + [(n, s, g, l, k, True, y) for n, s, g, l, k, y in ROTATED_CASES]
    for ci, (name, scene, gi, limit, topk, rotated, yaw) in enumerate(todo):
        rows, labels = SCENES[scene]
        b = torch.tensor(rows, dtype=torch.float32)
        b = torch.cat([b, torch.full((len(rows), 1), yaw, dtype=torch.float32)], 1)
        labels = torch.tensor(labels, dtype=torch.int64)
        n_scales = len(EDGE_GRIDS[gi])
        cls_name, n_reg = ("SunRgbdImVoxelHeadV2", 7) if rotated else ("ScanNetImVoxelHeadV2", 6)
        bh = getattr(head_mod, cls_name)(n_classes=18, n_channels=8, n_reg_outs=n_reg, n_scales=n_scales, limit=limit,
                                         centerness_topk=topk)
        bh.voxel_size = EDGE_VOXEL
        stored = b.clone()
        stored[:, 2] = b[:, 2] - b[:, 5] / 2                             # bottom-centre storage
        gravity = torch.cat((Boxes(stored).gravity_center, stored[:, 3:]), 1)
        margin = face_margin(torch.cat(grids[gi]), gravity)
        if rotated:      # the device's sinf / cosf must not be able to flip an inside test
            assert margin > 1e-4, f"{name}: a point lies {margin:.2e} from a face"
        ct, bt, lb, occ = bh.get_targets(grids[gi], Boxes(stored), labels)
        k = f"c{ci}_"
        out[k + "cfg"] = np.array([gi, n_scales, limit, topk, int(rotated)])
        out[k + "boxes_gravity"], out[k + "gt_labels"] = gravity.numpy(), labels.numpy()
        out[k + "centerness"], out[k + "bbox"], out[k + "labels"], out[k + "occ"] = ct.numpy(), bt.numpy(), lb.numpy(), occ.numpy()
        names.append(("rot_" if rotated else "ax_") + name)
        print(f"{names[-1]:28s} boxes {len(rows)} positives {int((lb >= 0).sum()):3d} inside any {int(occ.sum()):3d} "
              f"labels {sorted(set(lb[lb >= 0].tolist()))} closest face {margin:.1e}")
    out["names"] = np.array(names, dtype="S32")
    path = os.path.join(HERE, "head_targets_edges.npz")
    save_npz(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(names)} cases)")


def main(which):
    ml = mg.install_stubs()
    head_mod = importlib.import_module("mmdet3d_plugin.models.dense_heads.imvoxel_head_v2")
    if "edges" in which:
        edges(head_mod)
    if "base" not in which:
        return
    out = {}
    sizes = [(40, 40, 16), (20, 20, 8), (10, 10, 4)]
    origin = (0.0, 0.0, 0.5)
    for tag, cls_name, n_reg, with_yaw in (("scannet", "ScanNetImVoxelHeadV2", 6, False), ("sunrgbd", "SunRgbdImVoxelHeadV2", 7, True)):
        bh = getattr(head_mod, cls_name)(n_classes=18, n_channels=8, n_reg_outs=n_reg, n_scales=3, limit=27,
                                         centerness_topk=18)
        bh.voxel_size = (.16, .16, .2)
        points = bh.get_points(sizes, origin, torch.device("cpu"))
        for case, (n, seed) in enumerate(((14, 3), (1, 4), (40, 5))):
            b = scene_boxes(n, seed, with_yaw)
            gc = b.clone()
            stored = b.clone()
            stored[:, 2] = gc[:, 2] - gc[:, 5] / 2                      # bottom-centre storage
            g = torch.Generator().manual_seed(seed + 100)
            labels = torch.randint(0, 18, (n,), generator=g)
            ct, bt, lb, occ = bh.get_targets(points, Boxes(stored), labels)
            k = f"{tag}{case}_"
            out[k + "boxes_gravity"] = torch.cat((Boxes(stored).gravity_center, stored[:, 3:]), 1).numpy()
            out[k + "gt_labels"] = labels.numpy()
            out[k + "centerness"], out[k + "bbox"], out[k + "labels"], out[k + "occ"] = ct.numpy(), bt.numpy(), lb.numpy(), occ.numpy()
            print(tag, case, "boxes", n, "positives", int((lb >= 0).sum()), "inside any", int(occ.sum()))
    out["points"] = torch.cat(points).numpy()
    out["scales"] = torch.cat([torch.full((len(p),), i, dtype=torch.int32) for i, p in enumerate(points)]).numpy()
    out["cfg"] = np.array([3, 27, 18])
    # vendored axis-aligned IoU (is_aligned=True), the quantity of AxisAlignedIoULoss
    spec = importlib.util.spec_from_file_location(
        "_ref_iou3d", os.path.join(mg.REF, "packages/mmdetection3d/mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py"))
    src = open(spec.origin).read()
    mod = {}
    start = src.index("def axis_aligned_bbox_overlaps_3d")
    exec(compile("import torch\n" + src[start:], spec.origin, "exec"), mod)           # the function only (no mmdet imports)
    g = torch.Generator().manual_seed(77)
    c = (torch.rand(64, 3, generator=g) - 0.5) * 2
    s = 0.2 + torch.rand(64, 3, generator=g)
    a = torch.cat([c - s / 2, c + s / 2], 1)
    c2 = c + torch.randn(64, 3, generator=g) * 0.3
    s2 = s * (0.6 + torch.rand(64, 3, generator=g))
    b2 = torch.cat([c2 - s2 / 2, c2 + s2 / 2], 1)
    out["iou_a"], out["iou_b"] = a.numpy(), b2.numpy()
    out["iou_aligned"] = mod["axis_aligned_bbox_overlaps_3d"](a, b2, is_aligned=True).numpy()
    np.savez_compressed(os.path.join(HERE, "head_targets.npz"), **out)


if __name__ == "__main__":
    if not os.path.isdir(mg.REF):
        sys.exit("needs /root/reference (build container only)")
    torch.set_num_threads(1)
    # numpy stamps head_targets.npz with the time of writing: `edges` alone leaves the committed file as it is
    main(sys.argv[1:] or ["base", "edges"])
