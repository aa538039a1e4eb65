#!/usr/bin/env python3
"""tests/golden/box_iou_rotated_self.npz: the recorded result of
test_rotated_iou_against_live_reference_build_when_present -- the IoU of 64 seeded random boxes with themselves by the
REFERENCE's own rotated-box IoU header (oracle/_ref, CUDA branch of its hull sort, fp32), so that the test also runs
where oracle/_ref cannot be built.  The boxes are drawn exactly as the test draws them.
Usage:  python tests/golden/make_golden_iou_self.py      (needs oracle/_ref, see make_golden_iou.py)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle  # noqa: E402


def boxes():
    rng = np.random.RandomState(5)
    return np.concatenate([rng.uniform(-1, 1, (64, 2)), rng.uniform(0.1, 1.5, (64, 2)), rng.uniform(-4, 4, (64, 1))],
                          1).astype(np.float32)


def main():
    a = boxes()
    iou = oracle.ref_box_iou_rotated(a, a, variant="cuda")
    if iou is None:
        sys.exit("oracle/_ref is not available")
    path = os.path.join(HERE, "box_iou_rotated_self.npz")
    np.savez_compressed(path, a=a, iou=iou)
    print(f"wrote {path}: {a.shape[0]} x {a.shape[0]} pairs, {(iou > 0).mean():.2f} overlapping")


if __name__ == "__main__":
    main()
