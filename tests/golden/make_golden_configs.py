#!/usr/bin/env python3
"""Generates tests/golden/ref_configs.json: the ``model`` settings of the reference's four configs
(configs/SGCDet_ScanNet.py, SGCDet_ARKit.py, SGCDet_large_ScanNet200.py, SGCDet_large_ARKit.py), read with
``sgcdet_amd.mmcv_lite.Config.fromfile`` exactly as test_reference_configs_build_unchanged used to read them
in place.  The fixture holds settings only (nested dicts, lists, numbers, strings); tuples are kept as
``{"__tuple__": [...]}`` so that the test rebuilds the same Python values.

    python tests/golden/make_golden_configs.py <reference checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
NAMES = ("SGCDet_ScanNet", "SGCDet_ARKit", "SGCDet_large_ScanNet200", "SGCDet_large_ARKit")


def encode(o):
    if isinstance(o, dict):
        return {k: encode(v) for k, v in o.items()}
    if isinstance(o, tuple):
        return {"__tuple__": [encode(v) for v in o]}
    if isinstance(o, list):
        return [encode(v) for v in o]
    if o is None or isinstance(o, (bool, int, float, str)):
        return o
    raise TypeError(f"not a plain setting: {type(o)}")


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "configs")):
        sys.exit("usage: make_golden_configs.py <reference checkout holding configs/>")
    from sgcdet_amd.mmcv_lite import Config
    out = {n: encode(Config.fromfile(os.path.join(sys.argv[1], "configs", n + ".py"))["model"]) for n in NAMES}
    with open(os.path.join(HERE, "ref_configs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
