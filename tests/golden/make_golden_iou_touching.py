#!/usr/bin/env python3
"""tests/golden/box_iou_rotated_touching.npz: rotated-box IoU by the REFERENCE's own code on pairs that almost touch.

The sibling of make_golden_iou.py (same oracle/_ref build of the reference's ``box_iou_rotated_utils.hpp``, CUDA branch of
its hull sort, fp32 and fp64).  The HIP kernel skips the polygon clip for pairs its ``may_overlap`` pre-test (circumcircles,
then four separating-axis tests with a 0.1 % margin) calls disjoint, claiming that the reference's IoU is exactly 0 there;
the reference has no pre-test, so this table decides the claim where it could fail:

  * 9 x 448 pairs: the second rectangle sits along a face normal of the first at ``reach * (1 - delta)`` (reach: the first's
    half extent plus the second's support along that normal), delta in DELTAS -- a gap of 0.3 % down to an overlap of
    0.01 % of the reach; sizes 0.05 .. 3 (log-uniform), orientations equal / perpendicular / equal within 1e-3 or 1e-5 rad
    / unrelated, a third of the centres up to 50 m from the origin (fp32 coordinates there carry 4e-6);
  * pairs that share an edge or a corner, identical, contained and plainly overlapping pairs, rectangles whose area is
    below the reference's 1e-14 cut (and one just above it).

On generation the CPU oracle is held to the two bounds the tests use (1e-6 against the fp32 table, 2e-5 against fp64) and
the table to its counts; a miss stops the script.  Nothing of the reference is copied: the fixture holds boxes and IoUs.
Usage:  python tests/golden/make_golden_iou_touching.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
from npz_util import save_npz  # noqa: E402

DELTAS = (-3e-3, -1.1e-3, -1e-3, -9e-4, -1e-4, -1e-6, 0.0, 1e-6, 1e-4)
PER_DELTA = 448
BLOCK = 256


def touching_pairs(rng):
    a, b = [], []
    for delta in DELTAS:
        for i in range(PER_DELTA):
            w1, h1, w2, h2 = np.exp(rng.uniform(np.log(0.05), np.log(3.0), 4))
            a1 = rng.uniform(-np.pi, np.pi)
            kind = i % 4
            a2 = (a1, a1 + np.pi / 2, a1 + rng.uniform(-1, 1) * (1e-3 if i % 8 < 4 else 1e-5), rng.uniform(-np.pi, np.pi))[kind]
            c1 = rng.uniform(-50, 50, 2) if i % 3 == 0 else rng.uniform(-3, 3, 2)
            sign = 1.0 if rng.rand() < 0.5 else -1.0
            u1, v1 = np.array([np.cos(a1), np.sin(a1)]), np.array([-np.sin(a1), np.cos(a1)])
            if rng.rand() < 0.5:
                n, tau, half1, t1 = sign * u1, v1, w1 / 2, h1 / 2
            else:
                n, tau, half1, t1 = sign * v1, u1, h1 / 2, w1 / 2
            u2, v2 = np.array([np.cos(a2), np.sin(a2)]), np.array([-np.sin(a2), np.cos(a2)])
            reach = half1 + w2 / 2 * abs(u2 @ n) + h2 / 2 * abs(v2 @ n)
            # the vertex (or face centre) of the second rectangle that points at the first lands on the face at `off`
            su = np.sign(u2 @ n) if abs(u2 @ n) > 1e-9 else 0.0
            sv = np.sign(v2 @ n) if abs(v2 @ n) > 1e-9 else 0.0
            vt = -(w2 / 2 * su * (u2 @ tau) + h2 / 2 * sv * (v2 @ tau))
            off = rng.uniform(-0.8, 0.8) * t1
            c2 = c1 + n * reach * (1.0 - delta) + tau * (off - vt)
            a.append([c1[0], c1[1], w1, h1, a1])
            b.append([c2[0], c2[1], w2, h2, a2])
    return a, b


def special_pairs(rng):
    a = [[0, 0, 1, 1, 0], [0, 0, 1, 1, 0], [0, 0, 1e-8, 1e-8, 0.1], [0, 0, 1, 1, 0], [0, 0, 1e-7, 5e-8, 0],
         [0.2, 0.1, 1e-7, 1e-6, 0.3], [0, 0, 0, 1, 0.2], [0, 0, 0, 0, 0]]
    b = [[1, 0, 1, 1, 0], [1, 1, 1, 1, 0], [0, 0, 1, 1, 0], [0, 0, 1e-8, 1e-8, 0.1], [0, 0, 1e-7, 5e-8, 0],
         [0, 0, 2, 2, 0], [0, 0, 1, 1, 0], [0, 0, 0, 0, 0]]
    for i in range(60):                                   # a shared edge / a shared corner, turned and moved
        w, h, ang = rng.uniform(0.2, 2.0), rng.uniform(0.2, 2.0), rng.uniform(-np.pi, np.pi)
        c = rng.uniform(-20, 20, 2)
        u, v = np.array([np.cos(ang), np.sin(ang)]), np.array([-np.sin(ang), np.cos(ang)])
        c2 = c + u * w if i % 2 == 0 else c + u * w + v * h
        a.append([c[0], c[1], w, h, ang])
        b.append([c2[0], c2[1], w, h, ang])
    for i in range(480):                                  # identical, contained, plainly overlapping
        w, h, ang = rng.uniform(0.1, 3.0), rng.uniform(0.1, 3.0), rng.uniform(-np.pi, np.pi)
        c = rng.uniform(-10, 10, 2)
        a.append([c[0], c[1], w, h, ang])
        if i % 3 == 0:
            b.append([c[0], c[1], w, h, ang])
        elif i % 3 == 1:
            b.append([c[0], c[1], w * 0.4, h * 0.4, ang + rng.uniform(-0.3, 0.3)])
        else:
            b.append([c[0] + rng.normal(0, 0.2 * w), c[1] + rng.normal(0, 0.2 * h), w * rng.uniform(0.7, 1.3), h * rng.uniform(0.7, 1.3),
                      ang + rng.normal(0, 0.3)])
    return a, b


def diagonal(fn, a, b):
    out = []
    for s in range(0, len(a), BLOCK):
        out.append(np.diag(fn(a[s:s + BLOCK], b[s:s + BLOCK])).copy())
    return np.concatenate(out)


def main():
    import torch
    rng = np.random.RandomState(20261)
    ta, tb = touching_pairs(rng)
    sa, sb = special_pairs(rng)
    a = np.array(ta + sa, dtype=np.float64).astype(np.float32)
    b = np.array(tb + sb, dtype=np.float64).astype(np.float32)
    if oracle.build_ref() is None:
        sys.exit("oracle/_ref is not available (build container only)")
    iou32 = diagonal(lambda x, y: oracle.ref_box_iou_rotated(x, y, variant="cuda"), a, b)
    iou64 = diagonal(lambda x, y: oracle.ref_box_iou_rotated(x.astype(np.float64), y.astype(np.float64), f64=True, variant="cuda"), a, b)
    ops = oracle.ops()
    got = diagonal(lambda x, y: ops.box_iou_rotated(torch.from_numpy(x).contiguous(), torch.from_numpy(y).contiguous()).numpy(), a, b)
    n_touch = len(ta)
    e32, e64 = np.abs(got.astype(np.float64) - iou32), np.abs(got.astype(np.float64) - iou64)
    print(f"{len(a)} pairs ({n_touch} near-touching): reference IoU > 1e-4 on {(iou32 > 1e-4).sum()}, exactly 0 on {(iou32 == 0).sum()}, "
          f"in (0, 1e-4] on {((iou32 > 0) & (iou32 <= 1e-4)).sum()}")
    print(f"near-touching: fp32 == 0 on {(iou32[:n_touch] == 0).sum()}, fp64 == 0 on {(iou64[:n_touch] == 0).sum()}, "
          f"max |fp32 - fp64| = {np.abs(iou32 - iou64).max():.2e}")
    print(f"oracle: max |got - fp32 table| = {e32.max():.2e} (bound 1e-6), max |got - fp64 table| = {e64.max():.2e} (bound 2e-5)")
    assert (iou32 > 1e-4).sum() >= 300 and (iou32 == 0).sum() >= 300
    assert e32.max() <= 1e-6, f"oracle misses the fp32 bound on pairs {np.nonzero(e32 > 1e-6)[0][:10]}"
    assert e64.max() < 2e-5, f"oracle misses the fp64 bound on pairs {np.nonzero(e64 >= 2e-5)[0][:10]}"
    path = os.path.join(HERE, "box_iou_rotated_touching.npz")
    save_npz(path, a=a, b=b, iou=iou32.astype(np.float32), iou_f64=iou64.astype(np.float64), n_touching=np.array([n_touch]))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
