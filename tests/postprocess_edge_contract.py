"""Decision edges of the kernels that decide instead of compute -- ``aligned_nms3d``, ``nms_rotated_bev`` (with its glue
``box3d_multiclass_nms_rotated``), ``box_iou_rotated`` and ``assign_targets`` -- shared by the CPU (oracle) and GPU (HIP
library) test modules: every check takes a TensorOps and a device.

A wrong decision exceeds no tolerance: it keeps another box or labels another voxel.  So every check here is an equality
against a reference that is decidable on its own:

  * aligned NMS: a plain loop restating mmdet3d ``aligned_3d_nms`` in fp32 torch on the CPU (ascending STABLE argsort,
    ``iou * same_class <= thr`` keeps, a NaN IoU drops);
  * rotated IoU: tests/golden/box_iou_rotated_touching.npz, the reference's own header on pairs within +-0.3 % of touching
    (make_golden_iou_touching.py) -- the table that decides the kernel's disjointness pre-test;
  * rotated NMS: a float64 greedy loop over an exact float64 polygon clip.  Inputs are seeded and fixed, and built so that
    no candidate pair's IoU lies within 1e-3 of the threshold (asserted on the CPU for every case): few detections per
    object, or one pile of nested sizes whose IoUs are area ratios.  Rectangles with parallel edges on common lines are NOT
    used here: on those the reference's intersection-point algorithm is itself far from the exact clip, in fp32 and fp64;
  * target assignment: tests/golden/head_targets_edges.npz, the reference's own ``get_targets`` on exact grids
    (make_golden_targets.py): ties at the selected centerness rank, duplicate and equal-volume boxes, a face on grid points.

Tie rules pinned here: aligned NMS processes the higher index first among equal scores, rotated NMS the lower index, the
``max_num`` cut keeps the earlier entry of the class-by-class survivor list."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK_SIZES = (1, 2, 63, 64, 65, 127, 128, 129)


# --------------------------------------------------------------------------------------------------------------------
# aligned NMS
# --------------------------------------------------------------------------------------------------------------------
def aligned_nms_ref(boxes, scores, labels, thr):
    """mmdet3d aligned_3d_nms restated in fp32 torch on the CPU; the sort is stable.  -> kept indices, descending score"""
    boxes, scores, labels = boxes.cpu().float(), scores.cpu().float(), labels.cpu()
    thr = torch.tensor(thr, dtype=torch.float32)
    x1, y1, z1, x2, y2, z2 = boxes.unbind(1)
    area = (x2 - x1) * (y2 - y1) * (z2 - z1)
    order = torch.argsort(scores, stable=True)
    zero = torch.zeros((), dtype=torch.float32)
    pick = []
    while order.numel():
        i = order[-1]
        pick.append(int(i))
        rest = order[:-1]
        il = torch.maximum(zero, torch.minimum(x2[i], x2[rest]) - torch.maximum(x1[i], x1[rest]))
        iw = torch.maximum(zero, torch.minimum(y2[i], y2[rest]) - torch.maximum(y1[i], y1[rest]))
        ih = torch.maximum(zero, torch.minimum(z2[i], z2[rest]) - torch.maximum(z1[i], z1[rest]))
        inter = il * iw * ih
        iou = inter / (area[i] + area[rest] - inter)
        iou = iou * (labels[i] == labels[rest]).float()
        order = rest[iou <= thr]                                       # a NaN compares false: dropped
    return torch.tensor(pick, dtype=torch.int64)


def clustered_aligned(n, seed, n_cls=3):
    """n boxes piled on n // 24 + 1 objects, continuous scores: members of one pile sit in every 64-row block"""
    g = torch.Generator().manual_seed(seed)
    n_obj = n // 24 + 1
    ctr = (torch.rand(n_obj, 3, generator=g) - 0.5) * torch.tensor([8.0, 8.0, 2.0])
    size = 0.5 + torch.rand(n_obj, 3, generator=g)
    obj = torch.randint(0, n_obj, (n,), generator=g)
    c = ctr[obj] + torch.randn(n, 3, generator=g) * 0.1
    s = size[obj] * (1.0 + torch.randn(n, 3, generator=g) * 0.1).clamp(0.6, 1.4)
    boxes = torch.cat([c - s / 2, c + s / 2], 1).float().contiguous()
    scores = torch.rand(n, generator=g).float()
    labels = torch.randint(0, n_cls, (n,), generator=g)
    return boxes, scores, labels


def _aligned(ops, device, boxes, scores, labels, thr):
    got = ops.aligned_nms3d(boxes.to(device), scores.to(device), labels.to(device), thr).cpu()
    want = aligned_nms_ref(boxes, scores, labels, thr)
    assert got.dtype == torch.int64
    assert torch.equal(got, want), (len(got), len(want), got[:8].tolist(), want[:8].tolist())
    return want


def check_aligned_sizes(ops, device, n):
    want = _aligned(ops, device, *clustered_aligned(n, seed=100 + n), 0.25)
    if n > 2:
        assert 0 < len(want) < n, (n, len(want))
    else:
        assert 1 <= len(want) <= n


def check_aligned_identical(ops, device):
    n = 70                                                              # two 64-row blocks
    boxes = torch.tensor([[0.25, 0.5, 0.0, 1.25, 2.0, 1.5]]).repeat(n, 1).contiguous()
    scores = torch.randperm(n, generator=torch.Generator().manual_seed(1)).float() / n
    assert len(_aligned(ops, device, boxes, scores, torch.zeros(n, dtype=torch.int64), 0.25)) == 1
    assert len(_aligned(ops, device, boxes, scores, torch.arange(n), 0.25)) == n
    # an IoU of exactly 1 at thr = 1: `<=` keeps every box
    assert len(_aligned(ops, device, boxes, scores, torch.zeros(n, dtype=torch.int64), 1.0)) == n


def check_aligned_exact_threshold(ops, device):
    """two unit cubes offset by 0.5 along x: IoU = 0.5f / 1.5f in fp32, `<= thr` keeps at equality"""
    boxes = torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0], [0.5, 0.0, 0.0, 1.5, 1.0, 1.0]])
    labels = torch.zeros(2, dtype=torch.int64)
    thr = float(np.float32(0.5) / np.float32(1.5))
    below = float(np.nextafter(np.float32(thr), np.float32(0)))
    assert below < thr
    for scores in (torch.tensor([0.9, 0.8]), torch.tensor([0.2, 0.7])):
        best = int(scores.argmax())
        assert _aligned(ops, device, boxes, scores, labels, thr).tolist() == [best, 1 - best]
        assert _aligned(ops, device, boxes, scores, labels, below).tolist() == [best]


def check_aligned_zero_volume(ops, device):
    """flat and point boxes among normal ones: 0 / 0 drops a zero-volume box under a kept zero-volume box of ANY class; a
    flat box inside a normal one has IoU 0 and stays"""
    boxes, scores, labels = clustered_aligned(100, seed=7)
    g = torch.Generator().manual_seed(8)
    idx = torch.randperm(100, generator=g)[:12]
    boxes[idx[:6], 5] = boxes[idx[:6], 2]                               # flat in z
    boxes[idx[6:], 3:] = boxes[idx[6:], :3]                             # points
    want = _aligned(ops, device, boxes.contiguous(), scores, labels, 0.25)
    flat = set(idx.tolist())
    kept_flat = [i for i in want.tolist() if i in flat]
    assert kept_flat == [int(idx[scores[idx].argmax()])], kept_flat     # the best one, which drops the other eleven
    assert len(want) > 4
    # alone among normal boxes a flat box survives: its IoU with everything is 0
    boxes2, scores2, labels2 = clustered_aligned(100, seed=7)
    boxes2[5, 5] = boxes2[5, 2]
    assert 5 in _aligned(ops, device, boxes2.contiguous(), scores2, labels2, 0.25).tolist()


def check_aligned_ties(ops, device, n, all_equal):
    boxes, scores, labels = clustered_aligned(n, seed=300 + n)
    if all_equal:
        scores = torch.full((n,), 0.5)
    else:
        scores[torch.randperm(n, generator=torch.Generator().manual_seed(n))[: n // 4]] = 0.5
    want = _aligned(ops, device, boxes, scores, labels, 0.25)
    assert 0 < len(want) < n
    if all_equal:
        assert want[0] == n - 1 and bool((want[1:] < want[:-1]).all())  # the higher index is processed first


def aligned_ragged_case():
    return clustered_aligned(200, seed=11) + (0.25,)


def check_aligned_dirty_workspace(ops, device):
    """the entry point itself with its workspace pre-filled with 0xFF bytes: the sweep reads only what the mask kernel wrote"""
    boxes, scores, labels, thr = aligned_ragged_case()
    boxes, scores, labels = boxes.to(device), scores.to(device), labels.to(device)
    want = ops.aligned_nms3d(boxes, scores, labels, thr)
    n = boxes.shape[0]
    keep = torch.empty(n, dtype=torch.int64, device=device)
    n_keep = torch.zeros(1, dtype=torch.int32, device=device)
    order = torch.argsort(scores, stable=True)
    ws = torch.full((n * ((n + 63) // 64),), -1, dtype=torch.int64, device=device)
    ops._call("sgc_aligned_nms3d", boxes, order, labels, float(thr), keep, n_keep, ws, n)
    assert torch.equal(keep[: int(n_keep.item())], want) and 0 < len(want) < n


# --------------------------------------------------------------------------------------------------------------------
# rotated IoU on pairs that almost touch
# --------------------------------------------------------------------------------------------------------------------
def check_iou_touching(ops, device, block=512):
    d = np.load(os.path.join(GOLDEN, "box_iou_rotated_touching.npz"))
    a, b = torch.from_numpy(d["a"]), torch.from_numpy(d["b"])
    ref32, ref64 = d["iou"].astype(np.float64), d["iou_f64"]
    got = []
    for s in range(0, len(a), block):
        m = ops.box_iou_rotated(a[s:s + block].contiguous().to(device), b[s:s + block].contiguous().to(device))
        got.append(torch.diagonal(m).cpu())
    got = torch.cat(got).double().numpy()
    e32, e64 = np.abs(got - ref32), np.abs(got - ref64)
    n_touch = int(d["n_touching"][0])
    print(f"{len(a)} pairs: max |got - fp32 table| {e32.max():.3e}, max |got - fp64 table| {e64.max():.3e}; of the {n_touch} "
          f"near-touching pairs got == 0 on {(got[:n_touch] == 0).sum()}, table == 0 on {(ref32[:n_touch] == 0).sum()}")
    assert (ref32 > 1e-4).sum() >= 300 and (ref32 == 0).sum() >= 300       # the table is not trivial
    assert n_touch >= 4000 and ((ref32[:n_touch] > 0) & (ref32[:n_touch] <= 1e-4)).sum() >= 100
    assert e32.max() <= 1e-6, (int(e32.argmax()), e32.max())
    assert e64.max() < 2e-5, (int(e64.argmax()), e64.max())


# --------------------------------------------------------------------------------------------------------------------
# rotated NMS: exact float64 reference
# --------------------------------------------------------------------------------------------------------------------
def _corners(b):
    x, y, w, h, a = b
    c, s = np.cos(a), np.sin(a)
    loc = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]])
    return loc @ np.array([[c, s], [-s, c]]) + np.array([x, y])         # counter-clockwise


def _clip(subject, a, b):
    """Sutherland-Hodgman: the part of polygon ``subject`` on the left of the directed line a -> b"""
    out = []
    for i in range(len(subject)):
        p, q = subject[i], subject[(i + 1) % len(subject)]
        sp = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        sq = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
        if sp >= 0:
            out.append(p)
        if (sp >= 0) != (sq >= 0):
            out.append(p + sp / (sp - sq) * (q - p))
    return out


def iou_f64(b1, b2):
    """float64 IoU of two rectangles (xc, yc, w, h, angle); an area below 1e-14 gives 0, as in the reference"""
    a1, a2 = b1[2] * b1[3], b2[2] * b2[3]
    if a1 < 1e-14 or a2 < 1e-14:
        return 0.0
    if np.hypot(b1[0] - b2[0], b1[1] - b2[1]) > 0.5 * (np.hypot(b1[2], b1[3]) + np.hypot(b2[2], b2[3])) * (1 + 1e-9):
        return 0.0                                                      # separated circumcircles
    poly, cb = list(_corners(b1)), _corners(b2)
    for i in range(4):
        poly = _clip(poly, cb[i], cb[(i + 1) % 4])
        if not poly:
            return 0.0
    p = np.array(poly)
    inter = 0.5 * abs(np.dot(p[:, 0], np.roll(p[:, 1], -1)) - np.dot(p[:, 1], np.roll(p[:, 0], -1)))
    return inter / (a1 + a2 - inter)


def bev_of(boxes):
    return torch.stack((boxes[:, 0] - boxes[:, 3] / 2, boxes[:, 1] - boxes[:, 4] / 2,
                        boxes[:, 0] + boxes[:, 3] / 2, boxes[:, 1] + boxes[:, 4] / 2, boxes[:, 6]), dim=1).contiguous()


def iou_matrix_f64(bev):
    """from the fp32 (x1, y1, x2, y2, ry) the kernels read, converted in float64"""
    b = bev.double().numpy()
    xywhr = np.stack(((b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1], b[:, 4]), 1)
    n = len(xywhr)
    m = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            m[i, j] = m[j, i] = iou_f64(xywhr[i], xywhr[j])
    return m


def rotated_nms_ref(iou, scores, score_thr, nms_thr):
    """-> per class the kept indices: candidates ``score > score_thr`` by descending score, equal scores by ascending index"""
    out = []
    for c in range(scores.shape[1]):
        s = scores[:, c]
        idx = torch.nonzero(s > score_thr)[:, 0]
        order = idx[s[idx].sort(descending=True, stable=True)[1]].tolist()
        removed, keep = set(), []
        for pi, p in enumerate(order):
            if p in removed:
                continue
            keep.append(p)
            removed.update(q for q in order[pi + 1:] if iou[p, q] > nms_thr)
        out.append(keep)
    return out


def assert_margin(iou, scores, score_thr, nms_thr, margin=1e-3):
    """no pair of candidates of one class has an IoU within ``margin`` of the threshold -- no case is left out"""
    cand = (scores > score_thr).double()
    pairs = (cand @ cand.t()).numpy() > 0
    np.fill_diagonal(pairs, False)
    near = np.abs(iou - nms_thr)[pairs]
    assert near.size == 0 or near.min() > margin, f"an IoU lies {near.min():.2e} from the threshold {nms_thr}"


def cluster_boxes(K, seed, per_obj=3, tiny=0):
    """[K,7] boxes: about ``per_obj`` jittered detections (centre 0.12, size 10 %, yaw 0.2 rad) of each of K // per_obj + 1
    objects that stand 4 m apart -- only detections of one object overlap, so a call has about K overlapping pairs and a
    seed exists for which none of their IoUs is near the threshold.  The last ``tiny`` boxes are rectangles of area 1e-16 at
    object centres."""
    g = torch.Generator().manual_seed(seed)
    n_obj = K // per_obj + 1
    size = 0.6 + torch.rand(n_obj, 3, generator=g) * 1.2
    yaw = (torch.rand(n_obj, generator=g) - 0.5) * 6.0
    o = torch.arange(n_obj)
    ctr = torch.stack(((o % 8).float() * 4.0 - 14.0, (o // 8).float() * 4.0 - 14.0, torch.zeros(n_obj)), 1)
    obj = torch.randint(0, n_obj, (K,), generator=g)
    c = ctr[obj] + torch.randn(K, 3, generator=g).clamp(-2, 2) * 0.12
    s = size[obj] * (1.0 + torch.randn(K, 3, generator=g) * 0.1).clamp(0.7, 1.3)
    a = yaw[obj] + torch.randn(K, generator=g).clamp(-2, 2) * 0.2
    boxes = torch.cat([c, s, a[:, None]], 1)
    if tiny:
        boxes[K - tiny:, :2] = ctr[obj[K - tiny:], :2]
        boxes[K - tiny:, 3:5] = 1e-8
    return boxes.float().contiguous()


def pile_boxes(K, seed):
    """[K,7] boxes of ONE pile in which every pair overlaps: five nested sizes (0.8 per step) of a 2.0 x 1.2 rectangle,
    centres within 0.015 and yaws within 0.03 rad of each other.  A smaller size lies inside a larger one, so the IoU of two
    sizes is their area ratio -- 0.64, 0.41, 0.26, 0.17 -- and the IoU within one size is above 0.8: no IoU is near 0.5."""
    g = torch.Generator().manual_seed(seed)
    scale = 0.8 ** torch.randint(0, 5, (K,), generator=g).double()
    c = (torch.rand(K, 2, generator=g).double() - 0.5) * 0.03 + torch.tensor([1.3, -0.7], dtype=torch.float64)
    a = 0.4 + (torch.rand(K, generator=g).double() - 0.5) * 0.06
    one = torch.ones(K, dtype=torch.float64)
    return torch.stack((c[:, 0], c[:, 1], 0 * one, 2.0 * scale, 1.2 * scale, one, a), 1).float().contiguous()


def distinct_scores(K, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([(torch.randperm(K, generator=g).float() + 1) / (K + 1) for _ in range(C)], 1).contiguous()


# box seeds: the first of 0, 1, 2 ... for which assert_margin holds (fixed here; the assertion runs in every test)
SEEDS = dict(k1=0, k2=0, k63=0, k64=0, k65=0, k128=0, k129=0, ragged=0, dense=0, ties=0, tiny=0, max_num=0)


@functools.lru_cache(maxsize=None)
def rotated_case(name):
    """-> boxes [K,7] fp32, scores [K,C], score_thr, nms_thr, float64 IoU matrix (computed once per process)"""
    thr = 0.15
    if name.startswith("k"):                                            # K in BLOCK_SIZES, three classes
        K = int(name[1:])
        boxes, scores = cluster_boxes(K, seed=SEEDS[name]), distinct_scores(K, 3, seed=K + 1)
        scores = scores * (torch.rand(K, 3, generator=torch.Generator().manual_seed(K + 2)) < 0.85)
        if K <= 2:
            scores = scores.clamp(min=0.1)
    elif name == "ragged":                                              # per-class counts 0, 1, 64, 65, K in one call
        K = 130
        boxes, scores = cluster_boxes(K, seed=SEEDS[name]), distinct_scores(K, 5, seed=22)
        g = torch.Generator().manual_seed(23)
        for c, count in enumerate((0, 1, 64, 65, K)):
            scores[torch.randperm(K, generator=g)[count:], c] = 0.0
    elif name == "dense":                                               # one pile: every pair overlaps
        K = 130
        boxes, scores = pile_boxes(K, seed=SEEDS[name]), distinct_scores(K, 2, seed=32)
        thr = 0.5
    elif name == "ties":                                                # three score levels within each class
        K = 100
        boxes = cluster_boxes(K, seed=SEEDS[name])
        scores = (torch.randint(0, 4, (K, 3), generator=torch.Generator().manual_seed(42)).float() * 0.25).contiguous()
    elif name == "tiny":                                                # area below 1e-14 among the candidates
        K = 70
        boxes, scores = cluster_boxes(K, seed=SEEDS[name], per_obj=5, tiny=6), distinct_scores(K, 2, seed=52)
        scores[K - 6:, 0] = torch.tensor([0.999, 0.998, 0.5, 0.4, 0.001, 0.002])
    elif name == "max_num":                                             # many survivors, few score levels
        K = 120
        boxes = cluster_boxes(K, seed=SEEDS[name])
        scores = ((torch.randint(1, 4, (K, 4), generator=torch.Generator().manual_seed(62)).float()) * 0.25).contiguous()
    else:
        raise KeyError(name)
    iou = iou_matrix_f64(bev_of(boxes))
    assert_margin(iou, scores, 0.0, thr)
    return boxes, scores, 0.0, thr, iou


def check_rotated_case(ops, device, name):
    boxes, scores, score_thr, thr, iou = rotated_case(name)
    K, C = scores.shape
    keep, n_keep = ops.nms_rotated_bev(bev_of(boxes).to(device), scores.to(device), score_thr, thr)
    want = rotated_nms_ref(iou, scores, score_thr, thr)
    keep, n_keep = keep.cpu(), n_keep.cpu()
    assert n_keep.tolist() == [len(w) for w in want], (name, n_keep.tolist(), [len(w) for w in want])
    for c in range(C):
        assert keep[c, :int(n_keep[c])].tolist() == want[c], (name, c)
    counts = (scores > score_thr).sum(0).tolist()
    if name == "ragged":
        assert counts == [0, 1, 64, 65, K] and [len(w) for w in want][:2] == [0, 1]
    if name == "dense":
        off = iou[~np.eye(K, dtype=bool)]
        assert off.min() > 0, "every pair of the pile overlaps: the 64 x 64 pair list of the off-diagonal tile is full"
        assert counts == [K, K] and all(1 < len(w) < K for w in want)
    if name == "tiny":
        tiny = list(range(K - 6, K))
        assert all(t in want[0] for t in tiny)                          # never suppressed, although inside other boxes
        big = [i for i in range(K - 6) if scores[i, 0] > 0]
        assert any(i in want[0] for i in big) and len(want[0]) < len(big) + 6   # and they suppress nothing themselves
        assert want[0][:2] == [K - 6, K - 5]
    if name == "ties":
        assert all(len(set(scores[w, c].tolist())) < len(w) for c, w in enumerate(want))      # survivors share scores
    if name.startswith("k") and K > 2:
        assert any(0 < len(w) < n for w, n in zip(want, counts)), (name, counts)
    return want


def check_max_num_cut(ops, device):
    """survivors above max_num with tied scores at the cut: a stable sort keeps the earlier entry of the class-by-class list"""
    from sgcdet_amd.plugin.bbox_head import box3d_multiclass_nms_rotated
    boxes, scores, score_thr, thr, iou = rotated_case("max_num")
    want = rotated_nms_ref(iou, scores, score_thr, thr)
    sel = torch.tensor([i for w in want for i in w])
    lab = torch.tensor([c for c, w in enumerate(want) for _ in w])
    sc = scores[sel, lab]
    order = sc.sort(descending=True, stable=True)[1]
    for max_num in (len(sel) // 2, len(sel) // 3, len(sel) + 1):
        ob, os_, ol = box3d_multiclass_nms_rotated(ops, boxes.to(device), scores.to(device), score_thr, max_num, thr)
        o = order[:max_num] if len(sel) > max_num else torch.arange(len(sel))
        assert torch.equal(ol.cpu(), lab[o]) and torch.equal(os_.cpu(), sc[o]) and torch.equal(ob.cpu(), boxes[sel[o]]), max_num
        if len(sel) > max_num:
            assert sc[order[max_num - 1]] == sc[order[max_num]], "the cut must fall inside a group of equal scores"


def check_rotated_dirty_workspace(ops, device):
    boxes, scores, score_thr, thr, _ = rotated_case("ragged")
    bev, scores = bev_of(boxes).to(device), scores.to(device)
    want_keep, want_n = ops.nms_rotated_bev(bev, scores, score_thr, thr)
    K, C = scores.shape
    keep = torch.zeros((C, K), dtype=torch.int64, device=device)
    n_keep = torch.zeros(C, dtype=torch.int32, device=device)
    st = scores.t()
    cand = st > score_thr
    counts = cand.sum(dim=1).to(torch.int32)
    order = torch.where(cand, st, torch.full_like(st, float("-inf"))).sort(dim=1, descending=True, stable=True)[1]
    ws = torch.full((C * K * ((K + 63) // 64),), -1, dtype=torch.int64, device=device)
    ops._call("sgc_nms_rotated_bev", bev, order.contiguous(), counts, float(thr), keep, n_keep, ws, K, C)
    assert torch.equal(n_keep, want_n)
    for c in range(C):
        assert torch.equal(keep[c, :int(n_keep[c])], want_keep[c, :int(want_n[c])]), c


ROTATED_CASES = tuple(f"k{k}" for k in BLOCK_SIZES if k != 127) + ("ragged", "dense", "ties", "tiny")


# --------------------------------------------------------------------------------------------------------------------
# target assignment
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def targets_fixture():
    d = np.load(os.path.join(GOLDEN, "head_targets_edges.npz"))
    return d, [n.decode() for n in d["names"]]


def target_case_names():
    return targets_fixture()[1]


def run_target_case(ops, device, name):
    d, names = targets_fixture()
    k = f"c{names.index(name)}_"
    gi, n_scales, limit, topk, rotated = (int(v) for v in d[k + "cfg"])
    t = lambda key: torch.from_numpy(d[key]).to(device).contiguous()
    got = ops.assign_targets(t(f"g{gi}_points"), t(f"g{gi}_scales"), t(k + "boxes_gravity"), t(k + "gt_labels"), bool(rotated),
                             n_scales, limit, topk)
    want = tuple(torch.from_numpy(d[k + key]) for key in ("centerness", "bbox", "labels", "occ"))
    return tuple(g.cpu() for g in got), want, bool(rotated)


def check_target_case(ops, device, name):
    (ct, bt, lb, occ), (want_c, want_b, want_l, want_o), rotated = run_target_case(ops, device, name)
    assert lb.shape[0] in (292, 90)
    pos = want_l >= 0
    assert int((lb >= 0).sum()) == int(pos.sum()) and int(occ.sum()) == int(want_o.sum()), \
        (name, int((lb >= 0).sum()), int(pos.sum()), int(occ.sum()), int(want_o.sum()))
    assert torch.equal(occ, want_o), name
    assert torch.equal(lb, want_l), (name, int((lb != want_l).sum()))
    assert torch.equal(bt, want_b), name
    if rotated:
        if bool(pos.any()):
            assert (ct[pos] - want_c[pos]).abs().max() <= 1e-5, name
    else:
        same = torch.isclose(ct, want_c, rtol=2.4e-7, atol=0, equal_nan=True)
        assert bool(same.all()), (name, int((~same).sum()))


def check_target_case_against_oracle(ops, oracle_ops, device, name):
    got, _, rotated = run_target_case(ops, device, name)
    want, _, _ = run_target_case(oracle_ops, "cpu", name)
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]), name
    assert torch.equal(got[1], want[1]), name
    if rotated:
        pos = want[2] >= 0
        if bool(pos.any()):
            assert (got[0][pos] - want[0][pos]).abs().max() <= 1e-5, name
    else:
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), name      # NaNs of background points included


def check_targets_fixture_is_not_vacuous():
    d, names = targets_fixture()
    n_pos = {n: int((d[f"c{i}_labels"] >= 0).sum()) for i, n in enumerate(names)}
    n_occ = {n: int(d[f"c{i}_occ"].sum()) for i, n in enumerate(names)}
    assert len(names) >= 40 and sum(v > 0 for v in n_pos.values()) >= len(names) - 2
    # ties at the selected rank: a strict `>` admits fewer points than the rank
    assert (n_pos["ax_sym_topk0"], n_pos["ax_sym_topk1"], n_pos["ax_sym_topk3"], n_pos["ax_sym_topk7"]) == (0, 1, 1, 5)
    assert n_pos["ax_sym_topk100"] == 75                                 # the select lands on the -1 fill: every inside point
    assert n_pos["ax_sym_limit1"] == 9 and n_pos["ax_sym_limit1000"] == 15
    assert n_occ["ax_face"] == 10 and n_occ["ax_mixed"] == 292
    for i, n in enumerate(names):
        if "mixed" in n:                                                 # of two duplicates the first wins; the tiny box owns nothing
            labels = set(d[f"c{i}_labels"].tolist())
            assert 3 in labels and 7 not in labels and 5 not in labels, (n, labels)
